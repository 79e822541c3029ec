"""The pose graph's covariances on the GPU (include/visfs_pose_graph_cov.h on a visfs_ba handle: k_pose_graph_cov_setup, one
workgroup per column in k_pose_graph_cov_solve, k_pose_graph_cov_gather) against the one-core host twin, byte for byte: joint,
relative, the record and the solved columns with their iteration counts.  tests/test_pose_graph_cov.py holds the twin to the NumPy
checker on the same graphs and queries (tests/pose_graph_cov_cases.py)."""
import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_cov_cases as cc
from visfs_amd import abi, backend
from visfs_amd import pose_graph as pg
from visfs_amd import pose_graph_cov as pgc

pytestmark = pytest.mark.gpu

CASES = pc.cases()
BY_NAME = {c["name"]: c for c in CASES}
SMALL = ["n2_one_edge", "n3", "n5_fixed_in_the_middle", "n5_two_fixed", "edge_between_two_fixed", "duplicate_edges", "edges_given_j_below_i",
         "no_chain_edges", "huber_false_closure", "yaw_across_pi"]
# (case, sources or None for the case's own choice, keyword arguments)
RUNS = [(name, None, {}) for name in SMALL]
RUNS += [(name, count, {}) for name in ("rows_63", "rows_64", "rows_65") for count in (1, 2, 64)]
RUNS += [(name, None, {}) for name in ("rows_1023", "rows_1024", "rows_1025")]
RUNS += [("n4096", 2, {}), ("rows_65", 2, {"preconditioner": 0}), ("rows_65", 2, {"pcg_tolerance": 1e-8})]


def run_id(run):
    name, count, kw = run
    return name + (f"-{count}_sources" if count else "") + "".join(f"-{k}_{v}" for k, v in kw.items())


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


@pytest.fixture(scope="module")
def pair(solver):
    dev, host = pg.PoseGraph(solver), pg.PoseGraph()
    yield dev, host
    dev.close(); host.close()


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def both(pair, case, queries, **kw):
    out = []
    for g in pair:
        rc, r = pgc.covariance(g, case["poses"], case["fixed"], case["edges"], queries, **kw)
        assert rc == abi.OK, g.last_error()
        out.append(r)
    return out


@pytest.mark.parametrize("run", RUNS, ids=[run_id(r) for r in RUNS])
def test_device_equals_twin(pair, run):
    name, count, kw = run
    case = BY_NAME[name]
    dev, host = pair
    q, sources = cc.queries_for(case, count)
    kw = dict({"pcg_tolerance": 1e-13}, **kw)
    rd, rh = both(pair, case, q, **kw)
    keys = ("sources", "columns", "pcg_iterations_max", "pcg_iterations_total", "unconverged_columns", "free_vertices", "cost")
    assert rd["bytes"] == rh["bytes"], ({k: rd[k] for k in keys}, {k: rh[k] for k in keys})
    assert rd["sources"] == len(sources) and rd["pcg_iterations_total"] > 0
    same_bytes(rd["joint"], rh["joint"], "joint")
    same_bytes(rd["relative"], rh["relative"], "relative")
    assert np.all(np.isfinite(rd["joint"])) and np.abs(rd["joint"]).max() > 0.0
    n = rd["free_vertices"]
    for s in sorted({0, len(sources) // 2, len(sources) - 1}):
        (sd, Xd, itd), (sh, Xh, ith) = pgc.columns(dev, s, n), pgc.columns(host, s, n)
        assert sd == sh == abi.OK
        same_bytes(Xd, Xh, f"the columns of source {s}")
        same_bytes(itd, ith, f"the iterations of source {s}")
        assert itd.max() <= rd["pcg_iterations_max"] and np.abs(Xd).max() > 0.0
    assert pgc.last_counts(dev) == (3, 2, 1) and pgc.last_counts(host) == (0, 0, 0)


def test_unconverged_columns_equal_the_twin(pair):
    case = BY_NAME["rows_65"]
    q, _ = cc.queries_for(case, 2)
    rd, rh = both(pair, case, q, max_pcg_iterations=2)
    assert rd["bytes"] == rh["bytes"] and rd["unconverged_columns"] > 0
    same_bytes(rd["joint"], rh["joint"], "joint")


def test_a_zero_pivot_is_a_status_on_the_device(pair):
    """informations diag(1, 1, 0) on a chain: the last vertex's yaw pivot is exactly 0, an arithmetic result and no fault; launch 2
    reads the status word and leaves"""
    dev, host = pair
    c = pc.make("chain", 6, seed=40)
    edges = [(e[0], e[1], e[2], np.diag([1.0, 1.0, 0.0]), 0.0) for e in c["edges"]]
    for g in (dev, host):
        rc, r = pgc.covariance(g, c["poses"], c["fixed"], edges, [(1, 5)])
        assert rc == pgc.ERR_SINGULAR and "pivot" in g.last_error()
        assert np.all(r["joint"] == 0.0) and np.all(r["relative"] == 0.0)
    rd, rh = both(pair, c, [(1, 5)])                                          # the object works on
    assert rd["bytes"] == rh["bytes"]
    same_bytes(rd["joint"], rh["joint"], "joint")


def test_a_call_after_a_refusal(pair):
    dev, host = pair
    case = BY_NAME["n5_two_fixed"]
    q, _ = cc.queries_for(case)
    first = both(pair, case, q)[0]
    name, poses, fixed, edges, _ = pc.refusals()[0]
    assert pgc.covariance(dev, poses, fixed, edges, [(0, 1)])[0] == abi.ERR_BAD_ARGUMENT and dev.last_error() != ""
    assert pgc.covariance(dev, case["poses"], case["fixed"], case["edges"], [(0, 9)])[0] == abi.ERR_BAD_ARGUMENT
    again = both(pair, case, q)[0]
    assert again["bytes"] == first["bytes"]
    same_bytes(again["joint"], first["joint"], "joint")
    same_bytes(again["relative"], first["relative"], "relative")
    assert pgc.last_counts(dev) == (3, 2, 1)


def test_optimize_is_the_same_after_a_covariance_call(pair):
    """the covariance calls own their buffers: optimize returns the bytes it returned before, and a covariance call in between
    leaves its trace and counts"""
    dev, host = pair
    fresh = pg.PoseGraph(dev.solver)                                         # an object that never saw a covariance call
    case, other = BY_NAME["rows_65"], BY_NAME["rows_63"]
    rc, before = fresh.optimize(case["poses"], case["fixed"], case["edges"], pcg_tolerance=1e-13)
    assert rc == abi.OK
    trace = fresh.trace()
    q, _ = cc.queries_for(other, 2)
    rc, _ = pgc.covariance(fresh, other["poses"], other["fixed"], other["edges"], q)
    assert rc == abi.OK
    same_bytes(fresh.trace(), trace, "the trace of the last optimize")
    assert fresh.last_counts() == (1, 2, 1) and pgc.last_counts(fresh) == (3, 2, 1)
    rc, after = fresh.optimize(case["poses"], case["fixed"], case["edges"], pcg_tolerance=1e-13)
    assert rc == abi.OK and after["bytes"] == before["bytes"]
    same_bytes(after["poses"], before["poses"], "poses")
    same_bytes(after["chi2"], before["chi2"], "chi2")
    same_bytes(fresh.trace(), trace, "trace")
    rc, L = fresh.linearize(case["poses"], case["fixed"], case["edges"])
    rc2, Lh = host.linearize(case["poses"], case["fixed"], case["edges"])
    assert rc == rc2 == abi.OK
    same_bytes(L["edge_blocks"], Lh["edge_blocks"], "the linearize hook")
    fresh.close()
