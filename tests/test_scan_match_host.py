"""The correlative scan matcher's one-core host twin (include/visfs_scan_match.h on host sub-maps) against the independent
Python checker (tests/scan_match_oracle.py): parameters, every discretised cell, every integer sum, every score bit for
bit, the winner and the pose; the geometric condition of the base scene; the tie rule, the limits and the errors; and
visfs_scan_pretreat against a restatement of Estimator::laserPretreatment."""
import ctypes as C
import math

import numpy as np
import pytest

import scan_match_cases as cases
import scan_match_oracle as oracle
import submap_oracle
from visfs_amd import abi
from visfs_amd import scan_match as scm
from visfs_amd import submap as sm


class OracleSubmaps:
    """submap_oracle.Submaps behind the insert() of submap.Submaps."""

    def __init__(self, limit):
        self.s = submap_oracle.Submaps(limit=limit)

    def insert(self, T, rds):
        for o, ret, mis in rds:
            self.s.insert_range_data(T, list(o), [list(p) for p in ret], [list(p) for p in mis])
        return 0

    def last_error(self):
        return ""


_grids = {}


def grids(case):
    """The case's sub-maps, host twin and checker (built once per distinct insertion history)."""
    key = (case["limit"], id(case["frames"][0][1][0][1]), len(case["frames"]))
    if key not in _grids:
        host = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
        orc = OracleSubmaps(case["limit"])
        cases.fill(host, case)
        cases.fill(orc, case)
        d = host.describe()
        assert len(d) == len(orc.s.subs)
        for i, x in enumerate(d):                                   # the same grid on both sides before anything is matched
            g = orc.s.subs[i][0]
            assert (x["num_x_cells"], x["num_y_cells"], x["max_x"], x["max_y"]) == (g.nx, g.ny, g.max_x, g.max_y)
            assert np.array_equal(host.download(i)[0].ravel(), np.asarray(g.cells, dtype=np.uint16))
        _grids[key] = (host, orc, case["frames"])                   # (the frames kept alive: their id is the key)
    return _grids[key][0], _grids[key][1]


def run_both(case):
    host, orc = grids(case)
    lw, aw, tw, rw = case["prm"]
    rc, r = host.match(case["guess"], case["points"], scm.default_params(linear_search_window=lw, angular_search_window=aw,
                       translation_delta_cost_weight=tw, rotation_delta_cost_weight=rw), index=case["index"])
    assert rc == abi.OK, host.last_error()
    sums, scores, cells = host.match_download()
    o = oracle.match(orc.s.subs[case["index"]][0], case["guess"], [list(p) for p in case["points"]], lw, aw, tw, rw)
    return r, sums, scores, cells, o


def assert_exact(r, sums, scores, cells, o):
    assert r["matched"] == 1
    assert (r["num_scans"], r["num_linear"]) == (o["S"], o["nl"])
    assert r["angular_step"] == o["step"]
    assert cells.tolist() == [[list(c) for c in row] for row in o["cells"]]
    assert sums.ravel().tolist() == o["sums"]
    assert scores.ravel().tobytes() == np.asarray(o["scores"], dtype=np.float64).tobytes()
    assert (r["scan_index"], r["x_offset"], r["y_offset"]) == o["winner"]
    assert r["sum"] == o["sum"]
    for k in ("score", "x", "y", "yaw"):
        assert np.float64(r[k]).tobytes() == np.float64(o[k]).tobytes(), k


BASE = cases.base_cases()
EDGE = cases.edge_cases()


@pytest.mark.parametrize("case", BASE, ids=[c["name"] for c in BASE])
def test_base_scene_twin_equals_checker_and_finds_the_pose(case):
    r, sums, scores, cells, o = run_both(case)
    assert (o["na"], o["nl"], o["S"]) == (13, 6, 27)
    assert_exact(r, sums, scores, cells, o)
    # geometry, not a tuned tolerance: within one cell per axis and two angular steps of the truth
    res = 0.05
    tx, ty, tyaw = case["truth"]
    for got in (r, o):
        assert abs(got["x"] - tx) <= res and abs(got["y"] - ty) <= res, (got["x"] - tx, got["y"] - ty)
        assert abs(got["yaw"] - tyaw) <= 2 * o["step"], (got["yaw"] - tyaw, o["step"])


@pytest.mark.parametrize("case", EDGE, ids=[c["name"] for c in EDGE])
def test_edge_cases_twin_equals_checker(case):
    r, sums, scores, cells, o = run_both(case)
    assert_exact(r, sums, scores, cells, o)
    name = case["name"]
    if name.startswith("n") and name[1:].isdigit():
        assert cells.shape[1] == int(name[1:])
    if name == "nl0":
        assert r["num_linear"] == 0 and sums.shape[1:] == (1, 1)
    if name == "nl10":
        assert r["num_linear"] == 10
    if name == "one_scan":
        assert r["num_scans"] == 1
    if name == "many_scans":
        assert 150 <= r["num_scans"] <= 190
    if name == "outside":
        assert not sums.any() and (r["scan_index"], r["x_offset"], r["y_offset"]) == (r["num_scans"] // 2, 0, 0)
    if name == "grid_edge":
        assert cells[..., 0].max() + r["num_linear"] >= 200 and cells[..., 1].min() - r["num_linear"] < 0
    if name == "cropped_front":
        host, _ = grids(case)
        d = host.describe()
        assert d[0]["finished"] and len(d) == 2
        assert cells[..., 0].min() - r["num_linear"] < 0 and cells[..., 0].max() + r["num_linear"] >= d[0]["num_x_cells"]
        assert sums.any()
    if name == "second_submap":
        assert len(grids(case)[0].describe()) == 2
    if name == "after_growth":
        assert grids(case)[0].describe()[0]["num_x_cells"] == 200


def test_tie_rule_first_candidate_wins():
    for (tw, rw), want in (((0.0, 0.0), "first"), ((0.1, 0.1), "centre")):
        case = cases.unknown_case(tw, rw)
        r, sums, scores, cells, o = run_both(case)
        assert_exact(r, sums, scores, cells, o)
        assert not sums.any()
        S, nl = r["num_scans"], r["num_linear"]
        assert S > 1 and nl > 0
        if want == "first":
            assert len(set(scores.ravel().tolist())) == 1
            assert (r["scan_index"], r["x_offset"], r["y_offset"]) == (0, -nl, -nl)
        else:
            assert (r["scan_index"], r["x_offset"], r["y_offset"]) == (S // 2, 0, 0)


def _prm(**kw):
    return scm.default_params(**kw)


def test_no_submap_and_no_points_give_the_guess_back():
    host = sm.Submaps(sm.default_params())
    pts = cases.base_cases()[0]["points"]
    g = (0.3, -0.2, 0.7)
    rc, r = host.match(g, pts)
    assert rc == abi.OK
    zero = dict(matched=0, x=g[0], y=g[1], yaw=g[2], score=0.0, sum=0, scan_index=0, x_offset=0, y_offset=0, num_scans=0, num_linear=0,
                angular_step=0.0)
    assert r == zero
    cases.fill(host, cases.base_cases()[0])
    rc, r = host.match(g, np.zeros((0, 3)))
    assert rc == abi.OK and r == zero
    sums, scores, cells = host.match_download()
    assert sums.size == scores.size == cells.size == 0
    host.close()


def test_limits_and_errors_leave_everything_as_it_was():
    case = cases.base_cases()[0]
    host = sm.Submaps(sm.default_params())
    cases.fill(host, case)
    before = (host.describe(), [host.download(i)[0].copy() for i in range(len(host.describe()))])
    rc, r0 = host.match(case["guess"], case["points"], _prm(linear_search_window=0.1, angular_search_window=0.05))
    assert rc == abi.OK
    ref = [a.copy() for a in host.match_download()]
    pts = np.asarray(case["points"])
    g = case["guess"]
    many = np.tile(pts, (83, 1))[:scm.MAX_POINTS + 1]
    assert len(many) == scm.MAX_POINTS + 1
    bad_pt = pts.copy(); bad_pt[3, 1] = np.inf
    far = pts.copy(); far[0, 0] = 300.0                               # step ~ 1.7e-4: 20 degrees need more than 1025 rotations
    mid = pts.copy(); mid[0, 0] = 15.0                                # step ~ 3.3e-3: 1.5 rad are ~900 rotations
    checks = [
        (abi.ERR_UNSUPPORTED, g, many, _prm()),                                                  # n > 16384
        (abi.ERR_UNSUPPORTED, g, pts, _prm(linear_search_window=0.05 * 32 + 0.01)),              # nl = 33
        (abi.ERR_UNSUPPORTED, g, far, _prm()),                                                   # S > 1025
        (abi.ERR_UNSUPPORTED, g, mid, _prm(linear_search_window=1.6, angular_search_window=1.5)),  # S <= 1025, L = 65: S L^2 > 2^21
        (abi.ERR_BAD_ARGUMENT, (g[0], math.nan, g[2]), pts, _prm()),
        (abi.ERR_BAD_ARGUMENT, g, bad_pt, _prm()),
        (abi.ERR_BAD_ARGUMENT, g, pts, _prm(linear_search_window=-0.1)),
        (abi.ERR_BAD_ARGUMENT, g, pts, _prm(angular_search_window=-0.1)),
    ]
    for want, guess, points, prm in checks:
        rc, _ = host.match(guess, points, prm)
        assert rc == want, (rc, want, host.last_error())
        now = host.match_download()
        assert all(np.array_equal(a, b) for a, b in zip(now, ref))    # the last call's candidates stay
    assert host.match(g, pts, index=1)[0] == abi.ERR_BAD_ARGUMENT     # one sub-map is active: index 1 names none
    assert host.match(g, pts, index=-1)[0] == abi.ERR_BAD_ARGUMENT
    # the limits themselves are inside: nl = 32 with one rotation
    rc, r = host.match(g, pts[:3], _prm(linear_search_window=1.6, angular_search_window=0.0))
    assert rc == abi.OK and (r["num_linear"], r["num_scans"]) == (32, 1)
    after = (host.describe(), [host.download(i)[0] for i in range(len(host.describe()))])
    assert after[0] == before[0] and all(np.array_equal(a, b) for a, b in zip(after[1], before[1]))
    host.close()


def test_pretreat_equals_the_restatement():
    rng = np.random.default_rng(3)
    a, b, c = 0.3, -0.2, 0.1                                          # a non-trivial laser -> camera transform
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
    T = np.concatenate([Rz @ Ry @ Rx, np.array([[0.12], [-0.05], [0.3]])], axis=1).reshape(12)
    origin = [0.01, 0.02, -0.03]
    for n, subdiv in ((37, 5), (600, 10), (3, 7), (1, 4), (0, 3), (50, 1)):
        ang = rng.uniform(0, 2 * math.pi, n)
        rngs = rng.choice([0.03, 0.08, 0.1, 2.0, 7.5, 29.0, 30.5, 80.0], n) * rng.uniform(0.9, 1.1, n)
        pts = np.stack([rngs * np.cos(ang) + origin[0], rngs * np.sin(ang) + origin[1], rng.uniform(-0.1, 0.1, n)], -1).reshape(n, 3)
        prm = scm.default_pretreat_params(num_subdivisions=subdiv)
        got = scm.pretreat(pts, T, origin, prm)
        want = oracle.pretreat([list(p) for p in pts], list(T), origin, subdiv, prm.min_range, prm.max_range, prm.missing_ray_length)
        assert len(got) == len(want) == min(n, subdiv)
        kinds = [0, 0, 0]
        for (go, gr, gm), (wo, wr, wm) in zip(got, want):
            assert go == wo
            assert np.asarray(gr).reshape(-1, 3).tobytes() == np.asarray(wr, dtype=np.float64).reshape(-1, 3).tobytes()
            assert np.asarray(gm).reshape(-1, 3).tobytes() == np.asarray(wm, dtype=np.float64).reshape(-1, 3).tobytes()
            kinds[1] += len(wr); kinds[2] += len(wm)
        kinds[0] = n - kinds[1] - kinds[2]
        if n >= 37:
            assert all(kinds), kinds                                  # dropped, returns and misses all occur
    # the output goes straight into an insertion
    host = sm.Submaps(sm.default_params())
    rds = scm.pretreat(cases.base_cases()[0]["points"], T, origin, scm.default_pretreat_params(num_subdivisions=3))
    assert host.insert(cases.pose_T(0.0, 0.0, 0.0), rds) == abi.OK and host.describe()[0]["num_range_data"] == 3
    host.close()


def test_abi_defaults_and_exports(hiplib):
    lib = scm.load()
    assert lib.visfs_scan_match_abi_version() == scm.ABI_VERSION == 1
    assert sm.load().visfs_submap_abi_version() == 1
    p = scm.default_params()
    assert (p.linear_search_window, p.translation_delta_cost_weight, p.rotation_delta_cost_weight) == (0.1, 0.1, 0.1)
    assert p.angular_search_window == 20.0 * math.pi / 180.0
    q = scm.default_pretreat_params()
    assert (q.num_subdivisions, q.min_range, q.max_range, q.missing_ray_length) == (1, 0.1, 30.0, 5.0)
    for name in scm.EXPORTS:
        assert hasattr(hiplib, name), name
    header = open(cases.ROOT + "/include/visfs_scan_match.h").read()
    for name in scm.EXPORTS:
        assert name + "(" in header, name
    assert C.sizeof(scm.Result) == 80 and C.sizeof(scm.Params) == 32
