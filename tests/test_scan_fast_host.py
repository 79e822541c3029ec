"""The branch-and-bound scan matcher's one-core twin (include/visfs_scan_fast.h on host sub-maps) against the independent
checker (tests/scan_fast_oracle.py: levels from their definition, the winner by brute force over every leaf) and, inside
its limits, against the exhaustive visfs_scan_match with both weights zero."""
import ctypes as C
import math

import numpy as np
import pytest

import scan_fast_cases as cases
import scan_fast_oracle as oracle
import scan_match_cases as smc
from visfs_amd import abi
from visfs_amd import scan_fast as sf
from visfs_amd import scan_match as scm
from visfs_amd import submap as sm

_built = {}


def built(case):
    """The case's host sub-maps, the checker's, and the frozen stacks by depth (built once per insertion history)."""
    key = (case["limit"], id(case["frames"][0][1][0][1]), len(case["frames"]))
    if key not in _built:
        host = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
        orc = cases.OracleSubmaps(case["limit"])
        smc.fill(host, case)
        smc.fill(orc, case)
        for i, d in enumerate(host.describe()):
            g = orc.grid(i)
            assert (d["num_x_cells"], d["num_y_cells"], d["max_x"], d["max_y"]) == (g.nx, g.ny, g.max_x, g.max_y)
            assert np.array_equal(host.download(i)[0].ravel(), np.asarray(g.cells, dtype=np.uint16))
        _built[key] = (host, orc, {}, case["frames"])
    return _built[key][:3]


def stack_of(case):
    host, orc, stacks = built(case)
    k = (case["index"], case["depth"])
    if k not in stacks:
        st = host.freeze(case["index"], case["depth"])
        assert st.status == abi.OK, host.last_error()
        stacks[k] = st
    return stacks[k], orc.grid(case["index"]), host


_checked = {}


def checker(case):
    """The brute-force result, shared among the tests (and depths) that search the same thing."""
    key = (case["limit"], id(case["frames"][0][1][0][1]), len(case["frames"]), case["index"], tuple(case["guess"]), id(case["points"]), case["prm"][:2])
    if key not in _checked:
        _, orc, _ = built(case)
        _checked[key] = (oracle.match(orc.grid(case["index"]), case["guess"], [list(p) for p in case["points"]], *case["prm"][:2]), case["points"])
    return _checked[key][0]


def assert_winner(r, o, depth):
    assert r["matched"] == 1
    assert (r["num_scans"], r["num_linear"]) == (o["S"], o["nl"])
    assert r["angular_step"] == o["step"]
    assert (r["scan_index"], r["x_offset"], r["y_offset"]) == o["winner"]
    assert r["sum"] == o["sum"]
    for k in ("score", "x", "y", "yaw"):
        assert np.float64(r[k]).tobytes() == np.float64(o[k]).tobytes(), k
    H = 0
    while H < depth - 1 and (1 << H) < o["L"]:
        H += 1
    assert r["depth_used"] == H + 1


def assert_hook(hk, r, o):
    """The counts are consistent, and the level-0 survivors are exactly the leaves with Q >= B."""
    H = r["depth_used"] - 1
    assert (hk["S"], hk["L"], hk["H"]) == (o["S"], o["L"], H)
    per = (-(-o["L"] // (1 << H))) ** 2
    assert hk["bounds"].shape == (o["S"], per) and hk["scored"][H] == o["S"] * per
    assert all(0 < k <= s for k, s in zip(hk["kept"], hk["scored"]))
    Q = o["Q"].ravel()
    assert 0 <= hk["B"] <= o["sum"] and hk["B"] in Q                      # a real leaf's sum
    want = np.flatnonzero(Q >= hk["B"])
    assert hk["survivors"][:, 0].tolist() == want.tolist()
    assert hk["survivors"][:, 1].tolist() == Q[want].tolist()
    assert o["index"] in hk["survivors"][:, 0] and hk["kept"][0] == len(want)
    # a top node's bound is the maximum over the leaves it covers, or more
    L, S, m = o["L"], o["S"], int(round(math.sqrt(per)))
    pad = np.zeros((S, m << H, m << H), dtype=np.int64)
    pad[:, :L, :L] = o["Q"]
    cover = pad.reshape(S, m, 1 << H, m, 1 << H).max(axis=(2, 4)).reshape(S, per)
    assert (hk["bounds"] >= cover).all()


def exhaustive(host, case):
    lw, aw = case["prm"][:2]
    rc, r = host.match(case["guess"], case["points"], scm.default_params(linear_search_window=lw, angular_search_window=aw,
                       translation_delta_cost_weight=0.0, rotation_delta_cost_weight=0.0), index=case["index"])
    assert rc == abi.OK, host.last_error()
    return r


def assert_equals_exhaustive(r, e):
    for k in ("matched", "scan_index", "x_offset", "y_offset", "sum", "num_scans", "num_linear"):
        assert r[k] == e[k], k
    for k in ("score", "x", "y", "yaw", "angular_step"):
        assert np.float64(r[k]).tobytes() == np.float64(e[k]).tobytes(), k


# ---------------------------------------------------------------- levels
def level_scenes():
    by = {c["name"]: c for c in cases.edge_cases()}
    return [cases.base_cases()[0], by["cropped_front"], by["after_growth"]]


@pytest.mark.parametrize("case", level_scenes(), ids=["base", "cropped_front", "after_growth"])
def test_levels_equal_their_definition(case):
    st, grid, host = stack_of(case)
    d = st.describe()
    assert (d["depth"], d["device"], d["num_x_cells"], d["num_y_cells"]) == (cases.DEPTH, 0, grid.nx, grid.ny)
    assert (d["resolution"], d["max_x"], d["max_y"]) == (grid.res, grid.max_x, grid.max_y)
    total = 0
    for h in range(cases.DEPTH):
        got, e = st.download_level(h)
        want, we = oracle.level(grid, h)
        assert e == we == (1 << h) - 1 and got.shape == want.shape == (grid.ny + e, grid.nx + e)
        assert got.tobytes() == want.tobytes(), h
        total += got.size * 2
    assert total <= d["bytes"] < total + 256 * cases.DEPTH


def test_levels_of_a_grid_known_up_to_row_0_and_column_0():
    limits, cells = cases.corner_grid()
    grid = cases.oracle_grid(limits, cells)
    st = sf.ScanStack.from_grid(cells, limits, depth=6)
    assert st.status == abi.OK
    for h in range(6):
        got, e = st.download_level(h)
        want, _ = oracle.level(grid, h)
        assert got.tobytes() == want.tobytes(), h
        if h:                                                # the extension is in use: the corner's window sees cell (0, 0) only
            assert got[0, 0] == want[0, 0] == 32767 - (int(cells[0, 0]) & 32767) > 0
            assert got[-1, -1] == 32766                      # ... and the last stored cell sees only the last cell
    assert st.download_level(0)[0][3, 5] == 32767 - (int(cells[3, 5]) & 32767)
    # a search at the grid's low corner reads the extension: it equals the checker
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-0.6, 0.6, (50, 2)), np.zeros((50, 1))], axis=1)
    guess = (limits["max_x"] - 0.2, limits["max_y"] - 0.1, 0.3)          # near cell (0, 0)
    rc, r = st.match(guess, pts, sf.default_params(linear_search_window=0.5, angular_search_window=0.1))
    assert rc == abi.OK, st.last_error()
    o = oracle.match(grid, guess, [list(p) for p in pts], 0.5, 0.1)
    assert_winner(r, o, 6)
    assert_hook(st.match_download(), r, o)
    st.close()


# ---------------------------------------------------------------- the winner
INSIDE = cases.base_cases() + cases.edge_cases()


@pytest.mark.parametrize("case", INSIDE, ids=[c["name"] for c in INSIDE])
def test_winner_inside_the_exhaustive_limits(case):
    st, grid, host = stack_of(case)
    rc, r = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK, st.last_error()
    o = checker(case)
    assert_winner(r, o, case["depth"])
    assert_hook(st.match_download(), r, o)
    e = exhaustive(host, case)
    assert_equals_exhaustive(r, e)


def test_winner_beyond_the_exhaustive_limits():
    case = cases.wide_case()
    st, grid, host = stack_of(case)
    rc, r = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK, st.last_error()
    o = checker(case)
    assert (o["nl"], r["depth_used"]) == (40, 7)
    assert_winner(r, o, case["depth"])
    hk = st.match_download()
    assert_hook(hk, r, o)
    assert hk["bounds"].shape[1] == 4 and sum(hk["scored"]) < o["Q"].size       # it pruned
    lw, aw = case["prm"][:2]
    assert host.match(case["guess"], case["points"], scm.default_params(linear_search_window=lw, angular_search_window=aw))[0] == abi.ERR_UNSUPPORTED


RELOC = cases.reloc_cases()


@pytest.mark.parametrize("case", RELOC, ids=[c["name"] for c in RELOC])
def test_relocalisation_recovers_the_pose(case):
    st, grid, host = stack_of(case)
    rc, r = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK, st.last_error()
    o = checker(case)
    assert o["nl"] == 30
    assert_winner(r, o, case["depth"])
    # geometry, not a tuned tolerance: within one cell per axis and two angular steps of the truth; the checker alone meets it
    tx, ty, tyaw = case["truth"]
    for got in (o, r):
        assert abs(got["x"] - tx) <= cases.RES and abs(got["y"] - ty) <= cases.RES, (got["x"] - tx, got["y"] - ty)
        assert abs(got["yaw"] - tyaw) <= 2 * o["step"], (got["yaw"] - tyaw, o["step"])
    assert math.hypot(case["guess"][0] - tx, case["guess"][1] - ty) > 1.0                # off by more than a metre


def test_relocalisation_guesses_reach_the_stated_errors():
    assert len(cases.RELOC_ERRORS) >= 4 and cases.RELOC_ERRORS[0] == (1.2, -0.9, 0.4)
    assert all(max(abs(e[0]), abs(e[1])) <= 1.5 and abs(e[2]) <= 0.5 for e in cases.RELOC_ERRORS)


# ---------------------------------------------------------------- depth
def test_results_do_not_depend_on_the_depth():
    ref_case = cases.base_cases()[0]
    st, _, _ = stack_of(ref_case)
    rc, ref = st.match(ref_case["guess"], ref_case["points"], cases.params(ref_case))
    assert rc == abi.OK and ref["depth_used"] == 5                         # 2^4 > L = 13
    assert st.match_download()["bounds"].shape[1] == 1
    o = checker(ref_case)
    want = {1: (1, 169), 2: (2, 49), 3: (3, 16), 4: (4, 4)}                # depth: (levels used, top nodes per scan)
    for case in cases.depth_cases():
        st, _, _ = stack_of(case)
        rc, r = st.match(case["guess"], case["points"], cases.params(case))
        assert rc == abi.OK, st.last_error()
        hk = st.match_download()
        assert (r["depth_used"], hk["bounds"].shape[1]) == want[case["depth"]]
        assert_winner(r, o, case["depth"])
        assert_hook(hk, r, o)
        assert {k: v for k, v in r.items() if k != "depth_used"} == {k: v for k, v in ref.items() if k != "depth_used"}
        if case["depth"] == 1:                                             # plain exhaustive: every leaf scored, once
            assert hk["scored"] == [o["Q"].size] and hk["bounds"].ravel().tolist() == o["Q"].ravel().tolist()
            assert hk["B"] == o["sum"]


# ---------------------------------------------------------------- ties, overflow, min_score
def test_tie_rule_index_zero_wins_on_an_unknown_grid():
    case = cases.unknown_case()
    st, grid, host = stack_of(case)
    rc, r = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK, st.last_error()
    nl, S = r["num_linear"], r["num_scans"]
    assert S > 1 and nl > 0
    assert (r["scan_index"], r["x_offset"], r["y_offset"], r["sum"], r["score"]) == (0, -nl, -nl, 0, 0.1)
    hk = st.match_download()
    assert hk["B"] == 0 and len(hk["survivors"]) == S * (2 * nl + 1) ** 2 and hk["kept"] == hk["scored"]
    assert_equals_exhaustive(r, exhaustive(host, case))


def test_overflow_is_an_error_that_leaves_the_last_hook_data():
    good = cases.base_cases()[0]
    case = cases.overflow_case()
    st, grid, host = stack_of(good)
    rc, r0 = st.match(good["guess"], good["points"], cases.params(good))
    assert rc == abi.OK
    before = st.match_download()
    rc, _ = st.match(case["guess"], case["points"], cases.params(case, frontier_capacity=8))
    assert rc == abi.ERR_UNSUPPORTED
    assert "frontier overflow" in st.last_error() and "level 2" in st.last_error()      # nl = 1: L = 3, H = 2: the top level overflows
    cases.same_hook(st.match_download(), before)
    rc, r = st.match(case["guess"], case["points"], cases.params(case))    # within the default capacity: everything ties at 0
    assert rc == abi.OK and (r["scan_index"], r["x_offset"], r["y_offset"], r["sum"]) == (0, -1, -1, 0)
    assert r["num_scans"] > 8
    rc, r1 = st.match(good["guess"], good["points"], cases.params(good))
    cases.same_record(r1, r0)


def test_min_score_above_the_winner_gives_unmatched_with_the_fields_filled():
    case = cases.base_cases()[0]
    st, _, _ = stack_of(case)
    rc, r = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK and r["matched"] == 1 and 0.1 < r["score"] < 0.9
    rc, q = st.match(case["guess"], case["points"], cases.params(case, min_score=r["score"]))
    assert rc == abi.OK and q == r                                         # not below: matched
    rc, q = st.match(case["guess"], case["points"], cases.params(case, min_score=math.nextafter(r["score"], 1.0)))
    assert rc == abi.OK and q["matched"] == 0
    assert {k: v for k, v in q.items() if k != "matched"} == {k: v for k, v in r.items() if k != "matched"}
    rc, q = st.match(case["guess"], np.zeros((0, 3)), cases.params(case))
    zero = dict(matched=0, x=case["guess"][0], y=case["guess"][1], yaw=case["guess"][2], score=0.0, sum=0, scan_index=0, x_offset=0,
                y_offset=0, num_scans=0, num_linear=0, angular_step=0.0, depth_used=0)
    assert rc == abi.OK and q == zero


# ---------------------------------------------------------------- from_grid, snapshot
def test_from_grid_round_trip_equals_the_stack_from_the_sub_maps():
    for case in (cases.base_cases()[1], {c["name"]: c for c in cases.edge_cases()}["cropped_front"]):
        st, grid, host = stack_of(case)
        d = host.describe()[case["index"]]
        st2 = sf.ScanStack.from_grid(host.download(case["index"])[0], d, depth=case["depth"])
        assert st2.status == abi.OK and st2.describe() == st.describe()
        for h in range(case["depth"]):
            a, b = st.download_level(h), st2.download_level(h)
            assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()
        ra = st.match(case["guess"], case["points"], cases.params(case))
        rb = st2.match(case["guess"], case["points"], cases.params(case))
        assert ra[0] == rb[0] == abi.OK
        cases.same_record(ra[1], rb[1])
        cases.same_hook(st.match_download(), st2.match_download())
        st2.close()


def test_a_stack_is_a_snapshot():
    case = cases.base_cases()[3]
    sub = sm.Submaps(sm.default_params(num_range_data_limit=2))           # the next insertions finish, crop and drop the front
    smc.fill(sub, dict(case, frames=case["frames"][:3]))
    st = sub.freeze(0, 5)
    assert st.status == abi.OK
    levels = [st.download_level(h)[0].copy() for h in range(5)]
    rc, r0 = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK
    h0 = st.match_download()
    before = sub.describe()
    smc.fill(sub, dict(case, frames=case["frames"][3:]))                  # further insertions: the front is finished and cropped, then dropped
    assert sub.describe() != before
    rc, r1 = st.match(case["guess"], case["points"], cases.params(case))
    cases.same_record(r1, r0)
    sub.close()                                                            # the sub-maps go
    rc, r2 = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK
    cases.same_record(r2, r0)
    cases.same_hook(st.match_download(), h0)
    assert all(st.download_level(h)[0].tobytes() == levels[h].tobytes() for h in range(5))
    st.close()


# ---------------------------------------------------------------- limits, errors, ABI
def test_limits_and_errors():
    case = cases.base_cases()[0]
    st, grid, host = stack_of(case)
    rc, r0 = st.match(case["guess"], case["points"], cases.params(case))
    assert rc == abi.OK
    ref = st.match_download()
    pts = np.asarray(case["points"])
    g = case["guess"]
    many = np.tile(pts, (83, 1))[:sf.MAX_POINTS + 1]
    bad_pt = pts.copy(); bad_pt[3, 1] = np.inf
    far = pts.copy(); far[0, 0] = 300.0                                    # step ~ 1.7e-4: 0.2 rad need more than 1025 rotations
    mid = np.tile(pts, (30, 1)); mid[0, 0] = 15.0                          # 6000 points, ~900 rotations in 1.5 rad: S n > 2^22
    P = sf.default_params
    checks = [
        (abi.ERR_UNSUPPORTED, g, many, P(linear_search_window=0.1, angular_search_window=0.1), "16384 points"),
        (abi.ERR_UNSUPPORTED, g, pts, P(linear_search_window=RES_L(513), angular_search_window=0.0), "512 cells"),
        (abi.ERR_UNSUPPORTED, g, far, P(linear_search_window=0.1, angular_search_window=0.2), "1025 rotations"),
        (abi.ERR_UNSUPPORTED, g, mid, P(linear_search_window=0.1, angular_search_window=1.5), "2^22 cells"),
        (abi.ERR_BAD_ARGUMENT, (g[0], math.nan, g[2]), pts, P(), "guess"),
        (abi.ERR_BAD_ARGUMENT, g, bad_pt, P(), "point"),
        (abi.ERR_BAD_ARGUMENT, g, pts, P(linear_search_window=-0.1), "windows"),
        (abi.ERR_BAD_ARGUMENT, g, pts, P(angular_search_window=math.inf), "windows"),
        (abi.ERR_BAD_ARGUMENT, g, pts, P(min_score=math.nan), "min_score"),
        (abi.ERR_BAD_ARGUMENT, g, pts, P(frontier_capacity=3), "frontier_capacity"),
        (abi.ERR_BAD_ARGUMENT, g, pts, P(frontier_capacity=sf.MAX_FRONTIER + 1), "frontier_capacity"),
    ]
    for want, guess, points, prm, word in checks:
        rc, _ = st.match(guess, points, prm)
        assert rc == want and word in st.last_error(), (rc, want, st.last_error())
        cases.same_hook(st.match_download(), ref)                          # the last call's hook data stay
    # a stack too shallow for its window: depth 1 scores every leaf, and 2^22 top nodes are the limit
    st1 = host.freeze(0, 1)
    rc, _ = st1.match(g, pts[:3], P(linear_search_window=RES_L(512), angular_search_window=0.1))
    assert rc == abi.ERR_UNSUPPORTED and "too shallow" in st1.last_error()
    st1.close()
    # the limits themselves are inside: nl = 512 with one rotation and three points
    rc, r = st.match(g, pts[:3], P(linear_search_window=RES_L(512), angular_search_window=0.0))
    assert rc == abi.OK and (r["num_linear"], r["num_scans"], r["depth_used"]) == (512, 1, 7), st.last_error()
    # constructors
    for depth in (0, 17, -1):
        bad = host.freeze(0, depth)
        assert bad.status == abi.ERR_BAD_ARGUMENT and bad.h is None and "depth" in host.last_error()
    assert host.freeze(1, 3).status == abi.ERR_BAD_ARGUMENT and host.freeze(-1, 3).status == abi.ERR_BAD_ARGUMENT
    empty = sm.Submaps(sm.default_params())
    assert empty.freeze(0, 3).status == abi.ERR_BAD_ARGUMENT               # no sub-map yet
    empty.close()
    limits, cells = cases.corner_grid()
    assert sf.ScanStack.from_grid(cells, dict(limits, resolution=0.0), 3).status == abi.ERR_BAD_ARGUMENT
    assert sf.ScanStack.from_grid(cells, dict(limits, max_x=math.inf), 3).status == abi.ERR_BAD_ARGUMENT
    assert sf.ScanStack.from_grid(cells, limits, 0).status == abi.ERR_BAD_ARGUMENT
    # 16 levels of a 37 x 29 grid extend it by 32767 cells: beyond 1 GiB
    assert sf.ScanStack.from_grid(cells, limits, 16).status == abi.ERR_UNSUPPORTED
    ok = sf.ScanStack.from_grid(cells, limits, 12)
    assert ok.status == abi.OK and ok.describe()["bytes"] <= sf.MAX_BYTES
    assert ok.match_download() is None                                     # no match yet
    ok.close()


def RES_L(cells):
    """A linear window of exactly `cells` cells at the default resolution."""
    return cases.RES * cells - 0.01


def test_abi_defaults_and_exports(hiplib):
    lib = sf.load()
    assert lib.visfs_scan_fast_abi_version() == sf.ABI_VERSION == 1
    assert scm.load().visfs_scan_match_abi_version() == 1 and sm.load().visfs_submap_abi_version() == 1
    p = sf.default_params()
    assert (p.linear_search_window, p.min_score, p.frontier_capacity) == (7.0, 0.0, 1 << 20)
    assert p.angular_search_window == 30.0 * math.pi / 180.0
    header = open(smc.ROOT + "/include/visfs_scan_fast.h").read()
    for name in sf.EXPORTS:
        assert hasattr(hiplib, name), name
        assert name + "(" in header, name
    for name, value in (("MAX_DEPTH", sf.MAX_DEPTH), ("MAX_BYTES", sf.MAX_BYTES), ("MAX_POINTS", sf.MAX_POINTS), ("MAX_LINEAR", sf.MAX_LINEAR),
                        ("MAX_SCANS", sf.MAX_SCANS), ("MAX_CELLS", sf.MAX_CELLS), ("MAX_TOP_NODES", sf.MAX_TOP_NODES), ("MAX_FRONTIER", sf.MAX_FRONTIER)):
        assert f"#define VISFS_SCAN_FAST_{name} {value} " in header, name
    assert C.sizeof(sf.Result) == 88 and C.sizeof(sf.Params) == 32 and C.sizeof(sf.Info) == 48
    assert C.sizeof(scm.Result) == 80 and C.sizeof(scm.Params) == 32     # the exhaustive matcher's ABI is as it was
