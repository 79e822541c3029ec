"""The correlative scan matcher on the GPU (include/visfs_scan_match.h on device sub-maps) against its one-core host twin,
byte for byte: the result record and all three hook arrays.  The device sub-maps are built by the device insertion and the
host sub-maps by the host one, from the scenes of tests/scan_match_cases.py (the CPU tests hold the twin to the
independent checker on the same scenes)."""
import numpy as np
import pytest

import scan_match_cases as cases
from visfs_amd import abi, backend
from visfs_amd import scan_match as scm
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


def params(case):
    lw, aw, tw, rw = case["prm"]
    return scm.default_params(linear_search_window=lw, angular_search_window=aw, translation_delta_cost_weight=tw,
                              rotation_delta_cost_weight=rw)


def pair(solver, case):
    """Device and host sub-maps after the case's insertions; nothing is downloaded or described in between, so the device
    match is the first thing that follows the last insertion."""
    dev = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]), solver=solver)
    host = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
    cases.fill(dev, case)
    cases.fill(host, case)
    return dev, host


def match_both(dev, host, case):
    out = []
    for sub in (dev, host):
        rc, r = sub.match(case["guess"], case["points"], params(case), index=case["index"])
        assert rc == abi.OK, sub.last_error()
        out.append((r, sub.match_download()))
    (rd, ad), (rh, ah) = out
    assert rd == rh
    for k in ("x", "y", "yaw", "score", "angular_step"):
        assert np.float64(rd[k]).tobytes() == np.float64(rh[k]).tobytes(), k
    for a, b in zip(ad, ah):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    return rd, ad


def grids_equal(dev, host):
    assert dev.describe() == host.describe()
    for i in range(len(dev.describe())):
        assert np.array_equal(dev.download(i)[0], host.download(i)[0])


BASE = cases.base_cases()
EDGE = cases.edge_cases()


@pytest.fixture(scope="module")
def shared(solver):
    """One pair of sub-maps for the cases that share the base insertions (a match does not change them); closed before the solver."""
    dev, host = pair(solver, EDGE[0])
    yield dev, host
    dev.close(); host.close()


def test_base_scene_device_equals_twin(solver):
    """L^2 = 169 (no multiple of 64), S = 27, n = 200; five guesses on one object."""
    dev, host = pair(solver, BASE[0])                       # a fresh pair: the first match follows the insertions directly
    for case in BASE:
        r, (sums, scores, cells) = match_both(dev, host, case)
        assert (r["num_scans"], r["num_linear"], sums.shape, cells.shape) == (27, 6, (27, 13, 13), (27, 200, 2))
        assert abs(r["x"] - case["truth"][0]) <= 0.05 and abs(r["y"] - case["truth"][1]) <= 0.05
        assert abs(r["yaw"] - case["truth"][2]) <= 2 * r["angular_step"]
    grids_equal(dev, host)                                   # a match changes nothing
    dev.close(); host.close()


@pytest.mark.parametrize("case", EDGE, ids=[c["name"] for c in EDGE])
def test_edge_cases_device_equals_twin(solver, shared, case):
    fresh = case["name"] in ("after_growth", "cropped_front", "second_submap")
    assert fresh or (case["frames"] is EDGE[0]["frames"] and case["limit"] == EDGE[0]["limit"])
    dev, host = pair(solver, case) if fresh else shared
    r, (sums, scores, cells) = match_both(dev, host, case)
    name = case["name"]
    if name.startswith("n") and name[1:].isdigit():
        assert cells.shape[1] == int(name[1:])
    if name == "n%d" % (cases.chunk_size() + 1):
        assert cells.shape[1] > cases.chunk_size()
    if name == "nl0":
        assert sums.shape[1:] == (1, 1)
    if name == "nl10":
        assert sums.shape[1:] == (21, 21)                   # 441 offsets: two tiles of one workgroup each
    if name == "one_scan":
        assert r["num_scans"] == 1
    if name == "many_scans":
        assert 150 <= r["num_scans"] <= 190
    if name == "outside":
        assert not sums.any() and (r["scan_index"], r["x_offset"], r["y_offset"]) == (r["num_scans"] // 2, 0, 0)
    if name == "grid_edge":
        assert cells[..., 0].max() + r["num_linear"] >= 200 and cells[..., 1].min() - r["num_linear"] < 0
    if name == "after_growth":
        assert dev.describe()[0]["num_x_cells"] == 200
    if name == "cropped_front":
        d = dev.describe()
        assert d[0]["finished"] and len(d) == 2 and sums.any()
        assert cells[..., 0].min() - r["num_linear"] < 0 and cells[..., 0].max() + r["num_linear"] >= d[0]["num_x_cells"]
    if name == "second_submap":
        assert len(dev.describe()) == 2 and sums.any()
    if fresh:
        grids_equal(dev, host)
        dev.close(); host.close()


def test_matches_in_a_row_reuse_and_grow_the_buffers(solver):
    """Different S, L and n on one object: small, larger in every dimension, small again."""
    by = {c["name"]: c for c in EDGE}
    dev, host = pair(solver, BASE[0])
    shapes = []
    for case in (by["n63"], by["nl10"], BASE[1], by["many_scans"], by["n1"], by["nl0"]):
        r, (sums, scores, cells) = match_both(dev, host, case)
        shapes.append((sums.shape, cells.shape[1]))
    assert len(set(shapes)) == len(shapes)
    dev.close(); host.close()


def test_tie_rule_and_unmatched_calls_on_the_device(solver):
    for (tw, rw) in ((0.0, 0.0), (0.1, 0.1)):
        case = cases.unknown_case(tw, rw)
        dev, host = pair(solver, case)
        r, (sums, scores, cells) = match_both(dev, host, case)
        want = (0, -r["num_linear"], -r["num_linear"]) if tw == 0.0 else (r["num_scans"] // 2, 0, 0)
        assert (r["scan_index"], r["x_offset"], r["y_offset"]) == want and not sums.any()
        dev.close(); host.close()
    dev = sm.Submaps(sm.default_params(), solver=solver)
    g = (0.3, -0.2, 0.7)
    rc, r = dev.match(g, BASE[0]["points"])                  # no sub-map yet
    assert rc == abi.OK and r["matched"] == 0 and (r["x"], r["y"], r["yaw"], r["score"]) == (g[0], g[1], g[2], 0.0)
    cases.fill(dev, BASE[0])
    rc, r = dev.match(g, np.zeros((0, 3)))
    assert rc == abi.OK and r["matched"] == 0 and r["num_scans"] == 0
    far = np.asarray(BASE[0]["points"]).copy(); far[0, 0] = 300.0
    assert dev.match(g, far)[0] == abi.ERR_UNSUPPORTED       # S > 1025: nothing launched
    assert dev.match((g[0], np.nan, g[2]), BASE[0]["points"])[0] == abi.ERR_BAD_ARGUMENT
    rc, r = dev.match(BASE[0]["guess"], BASE[0]["points"], params(BASE[0]))
    assert rc == abi.OK and r["matched"] == 1
    dev.close()
