"""The branch-and-bound scan matcher on the GPU (include/visfs_scan_fast.h on device sub-maps) against its one-core host
twin, byte for byte: every level array, the result record, the incumbent, the per-level counts, the top level's bounds
and the sorted survivors.  The device sub-maps are built by the device insertion and the host sub-maps by the host one
(the CPU tests hold the twin to the independent checker on the same cases).  Where both apply, the device result also
equals the device visfs_scan_match with zero weights."""
import numpy as np
import pytest

import scan_fast_cases as cases
import scan_match_cases as smc
from visfs_amd import abi, backend
from visfs_amd import scan_fast as sf
from visfs_amd import scan_match as scm
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


def pair(solver, case):
    """Device and host sub-maps after the case's insertions; nothing is downloaded or described in between, so freezing
    is the first thing that follows the last insertion on the device."""
    dev = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]), solver=solver)
    host = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
    smc.fill(dev, case)
    smc.fill(host, case)
    return dev, host


def freeze_both(dev, host, case, depth=None):
    out = []
    for sub in (dev, host):
        st = sub.freeze(case["index"], depth or case["depth"])
        assert st.status == abi.OK, sub.last_error()
        out.append(st)
    return out


def levels_equal(sd, sh):
    a, b = sd.describe(), sh.describe()
    assert (a["device"], b["device"]) == (1, 0)
    assert {k: v for k, v in a.items() if k != "device"} == {k: v for k, v in b.items() if k != "device"}
    for h in range(a["depth"]):
        (la, ea), (lb, eb) = sd.download_level(h), sh.download_level(h)
        assert ea == eb and la.shape == lb.shape and la.tobytes() == lb.tobytes(), h


def match_both(sd, sh, case, **kw):
    out = []
    for st in (sd, sh):
        rc, r = st.match(case["guess"], case["points"], cases.params(case, **kw))
        assert rc == abi.OK, st.last_error()
        out.append((r, st.match_download()))
    (rd, hd), (rh, hh) = out
    cases.same_record(rd, rh)
    cases.same_hook(hd, hh)
    return rd, hd


def equals_exhaustive(dev, case, r):
    """The device visfs_scan_match with zero weights on the (unchanged) device sub-maps."""
    lw, aw = case["prm"][:2]
    rc, e = dev.match(case["guess"], case["points"], scm.default_params(linear_search_window=lw, angular_search_window=aw,
                      translation_delta_cost_weight=0.0, rotation_delta_cost_weight=0.0), index=case["index"])
    assert rc == abi.OK, dev.last_error()
    for k in ("matched", "scan_index", "x_offset", "y_offset", "sum", "num_scans", "num_linear"):
        assert r[k] == e[k], k
    for k in ("score", "x", "y", "yaw", "angular_step"):
        assert np.float64(r[k]).tobytes() == np.float64(e[k]).tobytes(), k


BASE = cases.base_cases()
EDGE = {c["name"]: c for c in cases.edge_cases()}


@pytest.fixture(scope="module")
def shared(solver):
    """One pair of sub-maps and stacks for the cases that share the base insertions; closed before the solver."""
    dev, host = pair(solver, BASE[0])
    sd, sh = freeze_both(dev, host, BASE[0])
    yield dev, host, sd, sh
    sd.close(); sh.close(); dev.close(); host.close()


def test_base_scene_levels_and_matches(shared):
    """Seven levels of a 200 x 200 grid; L = 13, S = 27, n = 200, H = 4; five guesses on one stack."""
    dev, host, sd, sh = shared
    levels_equal(sd, sh)
    assert sd.describe()["depth"] == 7 and sd.download_level(6)[0].shape == (263, 263)
    for case in BASE:
        r, hk = match_both(sd, sh, case)
        assert (r["num_scans"], r["num_linear"], r["depth_used"], hk["bounds"].shape) == (27, 6, 5, (27, 1))
        assert abs(r["x"] - case["truth"][0]) <= 0.05 and abs(r["y"] - case["truth"][1]) <= 0.05
        assert abs(r["yaw"] - case["truth"][2]) <= 2 * r["angular_step"]
        equals_exhaustive(dev, case, r)


SHARED_EDGES = ["n1", "n63", "n65", "n1025", "outside", "grid_edge", "many_scans"]


@pytest.mark.parametrize("name", SHARED_EDGES)
def test_edge_cases_on_the_base_stack(shared, name):
    """n = 1, 63, 65 (about a wavefront) and 1025; every read outside the grid; reads through the low-side extension and at
    indices >= nx; about 170 rotations."""
    dev, host, sd, sh = shared
    case = EDGE[name]
    assert case["limit"] == BASE[0]["limit"] and len(case["frames"]) == len(BASE[0]["frames"])      # the base insertions (fixed seeds)
    assert np.array_equal(case["frames"][-1][1][0][1], BASE[0]["frames"][-1][1][0][1])
    r, hk = match_both(sd, sh, case)
    if name.startswith("n") and name[1:].isdigit():
        assert hk["n"] == int(name[1:])
    if name == "outside":
        assert not hk["bounds"].any() and (r["scan_index"], r["x_offset"], r["y_offset"], r["sum"]) == (0, -1, -1, 0)
    if name == "many_scans":
        assert 150 <= r["num_scans"] <= 190
    equals_exhaustive(dev, case, r)
    if name == "grid_edge":                                  # the cells the exhaustive matcher's hook reports for the same search
        cells = dev.match_download()[2]
        assert cells[..., 0].max() + r["num_linear"] >= 200 and cells[..., 1].min() - r["num_linear"] < 0


@pytest.mark.parametrize("case", cases.depth_cases(), ids=[c["name"] for c in cases.depth_cases()])
def test_depths(shared, case):
    """depth 1: H = 0, every leaf scored by the top-level kernel; depths 2 and 3: the last children clipped by the window;
    depth 4: four top nodes per scan.  (2^H > L is the base stack's own case.)"""
    dev, host, _, _ = shared
    sd, sh = freeze_both(dev, host, case)
    levels_equal(sd, sh)
    r, hk = match_both(sd, sh, case)
    assert r["depth_used"] == case["depth"] and hk["bounds"].shape[1] == {1: 169, 2: 49, 3: 16, 4: 4}[case["depth"]]
    equals_exhaustive(dev, case, r)
    sd.close(); sh.close()


def test_wide_window_and_relocalisation(shared):
    """nl = 40 (L = 81, H = 6, beyond the exhaustive matcher) and a relocalisation from (1.2 m, -0.9 m, 0.4 rad) off."""
    dev, host, sd, sh = shared
    r, hk = match_both(sd, sh, cases.wide_case())
    assert (r["num_linear"], r["depth_used"], hk["bounds"].shape[1]) == (40, 7, 4)
    case = cases.reloc_cases()[0]
    r, hk = match_both(sd, sh, case)
    assert abs(r["x"] - case["truth"][0]) <= 0.05 and abs(r["y"] - case["truth"][1]) <= 0.05
    assert abs(r["yaw"] - case["truth"][2]) <= 2 * r["angular_step"]
    equals_exhaustive(dev, case, r)                          # nl = 30: still inside the exhaustive limits


@pytest.mark.parametrize("name", ["after_growth", "cropped_front", "second_submap"])
def test_fresh_sub_maps(solver, name):
    """A non-zero allocation offset (frozen right after an insertion that grew the grid), a finished and cropped front, and
    the second sub-map."""
    case = EDGE[name]
    dev, host = pair(solver, case)
    sd, sh = freeze_both(dev, host, case)
    levels_equal(sd, sh)
    r, hk = match_both(sd, sh, case)
    d = dev.describe()
    if name == "after_growth":
        assert d[0]["num_x_cells"] == 200 and sd.describe()["num_x_cells"] == 200
    if name == "cropped_front":
        assert d[0]["finished"] and len(d) == 2 and sd.describe()["num_x_cells"] == d[0]["num_x_cells"] < 200
    if name == "second_submap":
        assert len(d) == 2
    assert r["sum"] > 0
    equals_exhaustive(dev, case, r)
    sd.close(); sh.close(); dev.close(); host.close()


def test_create_from_grid_on_the_device(solver, shared):
    dev, host, sd, sh = shared
    limits, cells = cases.corner_grid()
    a = sf.ScanStack.from_grid(cells, limits, depth=6, solver=solver)
    b = sf.ScanStack.from_grid(cells, limits, depth=6)
    assert a.status == b.status == abi.OK
    levels_equal(a, b)
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-0.6, 0.6, (50, 2)), np.zeros((50, 1))], axis=1)
    case = dict(guess=(limits["max_x"] - 0.2, limits["max_y"] - 0.1, 0.3), points=pts, prm=(0.5, 0.1, 0.0, 0.0))
    match_both(a, b, case)
    a.close(); b.close()
    # a downloaded device grid gives the stack the device sub-maps give
    c = sf.ScanStack.from_grid(dev.download(0)[0], dev.describe()[0], depth=7, solver=solver)
    assert c.status == abi.OK
    levels_equal(c, sh)
    match_both(c, sh, BASE[2])
    c.close()


def test_overflow_then_a_good_call(shared):
    dev, host, sd, sh = shared
    good, over = BASE[1], cases.overflow_case()
    _, before = match_both(sd, sh, good)
    for st in (sd, sh):
        rc, _ = st.match(over["guess"], over["points"], cases.params(over, frontier_capacity=8))
        assert rc == abi.ERR_UNSUPPORTED and "frontier overflow at level 2" in st.last_error(), st.last_error()
        cases.same_hook(st.match_download(), before)        # the failed call left the hook data
    match_both(sd, sh, good)
    match_both(sd, sh, over)                                # within the default capacity: everything ties


def test_overflow_text_is_the_twin_s(shared):
    """The device single call runs the group's launch sequence with one member: its text carries no member prefix and nothing of
    an earlier call."""
    dev, host, sd, sh = shared
    over = cases.overflow_case()
    match_both(sd, sh, BASE[1])
    texts = []
    for st in (sd, sh):
        rc, _ = st.match(over["guess"], over["points"], cases.params(over, frontier_capacity=8))
        assert rc == abi.ERR_UNSUPPORTED
        texts.append(st.last_error())
    assert texts[0] == texts[1] == "frontier overflow at level 2: more than 8 nodes kept"


def test_two_stacks_have_their_own_blocks(shared):
    """A match on stack A, one on stack B with another guess and n, then A's hook: still that of A's call."""
    dev, host, sd, sh = shared
    a, b = BASE[0], dict(EDGE["n65"], guess=BASE[3]["guess"])
    bd, bh = freeze_both(dev, host, b)
    ra, ha = match_both(sd, sh, a)
    _, hb = match_both(bd, bh, b)
    assert (ha["n"], hb["n"]) == (200, 65) and a["guess"] != b["guess"]
    cases.same_hook(sd.match_download(), sh.match_download())
    cases.same_hook(sd.match_download(), ha)
    cases.same_hook(bd.match_download(), hb)
    bd.close(); bh.close()
    cases.same_hook(sd.match_download(), ha)                 # B's buffers are gone: A's are its own


def test_matches_in_a_row_reuse_and_grow_the_buffers(shared):
    """Different S, L and n on one stack: small, larger in every dimension, small again; a small capacity that holds."""
    dev, host, sd, sh = shared
    shapes = []
    for case in (EDGE["n63"], EDGE["nl10"], cases.wide_case(), EDGE["many_scans"], EDGE["n1"]):
        r, hk = match_both(sd, sh, case)
        shapes.append((hk["S"], hk["L"], hk["n"]))
    assert len(set(shapes)) == len(shapes)
    r, hk = match_both(sd, sh, BASE[0], frontier_capacity=max(hk_max(sh, BASE[0]), 4))     # exactly full: no overflow


def hk_max(sh, case):
    rc, _ = sh.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK
    return max(sh.match_download()["kept"])


def test_a_stack_outlives_its_sub_maps(solver):
    case = BASE[3]
    dev, host = pair(solver, dict(case, limit=2, frames=case["frames"][:3]))
    sd, sh = freeze_both(dev, host, case, depth=5)
    r0, h0 = match_both(sd, sh, case)
    for sub in (dev, host):
        smc.fill(sub, dict(case, frames=case["frames"][3:]))            # the front is finished, cropped and dropped
    r1, _ = match_both(sd, sh, case)
    cases.same_record(r1, r0)
    dev.close(); host.close()
    r2, h2 = match_both(sd, sh, case)
    cases.same_record(r2, r0)
    cases.same_hook(h2, h0)
    levels_equal(sd, sh)
    sd.close(); sh.close()


def test_tie_rule_and_unmatched_calls_on_the_device(solver):
    case = cases.unknown_case()
    dev, host = pair(solver, case)
    sd, sh = freeze_both(dev, host, case)
    r, hk = match_both(sd, sh, case)
    nl = r["num_linear"]
    assert (r["scan_index"], r["x_offset"], r["y_offset"], r["sum"]) == (0, -nl, -nl, 0) and hk["kept"] == hk["scored"]
    equals_exhaustive(dev, case, r)
    rc, q = sd.match(case["guess"], np.zeros((0, 3)), cases.params(case))
    assert rc == abi.OK and q["matched"] == 0 and q["num_scans"] == 0
    rc, q = sd.match(case["guess"], case["points"], cases.params(case, min_score=0.5))
    assert rc == abi.OK and q["matched"] == 0 and q["score"] == 0.1
    far = np.asarray(case["points"]).copy(); far[0, 0] = 300.0
    assert sd.match(case["guess"], far, cases.params(dict(case, prm=(0.1, 0.2, 0.0, 0.0))))[0] == abi.ERR_UNSUPPORTED    # S > 1025: nothing launched
    cases.same_hook(sd.match_download(), hk)
    sd.close(); sh.close(); dev.close(); host.close()
