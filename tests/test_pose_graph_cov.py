"""The covariances of the 2-D pose graph on the one-core host twin (include/visfs_pose_graph_cov.h with an object made without a
handle) against the NumPy checker (tests/pose_graph_cov_oracle.py: numpy.linalg.inv of the dense H), the checker against known
answers first, the host plan with every refusal, and the search-window helper.  tests/test_gpu_pose_graph_cov.py holds the device
to the twin byte for byte.

Bounds.  The measure is the largest deviation of the twin's `joint` from the checker's, relative to the largest |Sigma| entry among
the queried blocks of the case (and the same for `relative`, against its own largest entry); pcg_tolerance = 1e-13.  Measured on
the CPU (run this file as a script to print them), the worst case of each class:
    fewer than 1000 rows:   1.24e-13 (rows_65, 64 sources, 34 iterations at most)
    1000 rows and more:     2.44e-9 (rows_1024, 111 iterations at most; rows_1023 3.8e-11, rows_1025 1.9e-10)
The bounds asserted are 100 times that, the margin of DESIGN.md section 9p: the checker inverts H densely, the twin sums in lanes,
and the two differ at cond(H) times the rounding unit.  n4096 has no dense inverse: its columns are held to
|| H x - e ||_inf <= 1000 eps || H ||_inf || x ||_inf, a backward-stable solve with a factor for the iterations and the row's
entries (measured: 2.5e-12 to 1.7e-10, four orders below: the infinity norms overestimate the products)."""
import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_cov_cases as cc
import pose_graph_cov_oracle as co
import pose_graph_oracle as po
from visfs_amd import abi
from visfs_amd import pose_graph as pg
from visfs_amd import pose_graph_cov as pgc

CASES = pc.cases()
BY_NAME = {c["name"]: c for c in CASES}
DENSE = [c for c in CASES if c["dense"]]
EPS = 2.220446049250313e-16
TOL = 1e-13


def bound(rows):
    return 100 * (2.44e-9 if rows >= 1000 else 1.24e-13)


@pytest.fixture(scope="module")
def twin(hiplib):
    g = pg.PoseGraph()
    yield g
    g.close()


def deviation(twin, case, queries, **kw):
    """(the largest deviation of joint and of relative from the checker, each relative to the checker's largest entry; the record)"""
    rc, r = pgc.covariance(twin, case["poses"], case["fixed"], case["edges"], queries, pcg_tolerance=TOL, **kw)
    assert rc == abi.OK, (case["name"], twin.last_error())
    J, R = co.query(case["poses"], case["fixed"], case["edges"], queries)
    dj = np.abs(r["joint"] - J).max() / np.abs(J).max()
    dr = np.abs(r["relative"] - R).max() / np.abs(R).max()
    return max(dj, dr), r


# ------------------------------------------------------------------------------------------------ the checker alone, first
def chain(N, fixed_at, seed=40):
    return pc.make("chain", N, seed=seed, fixed=(fixed_at,))


@pytest.mark.parametrize("fixed_at", [0, 3, 6])
def test_checker_relative_of_a_chain_edge_is_its_inverse_information(fixed_at):
    c = chain(7, fixed_at)
    q = [(a, a + 1) for a in range(6)]
    _, R = co.query(c["poses"], c["fixed"], c["edges"], q)
    for k, (a, b) in enumerate(q):
        W = np.asarray(c["edges"][a][3])
        assert (c["edges"][a][0], c["edges"][a][1]) == (a, b)
        assert np.abs(R[k] - np.linalg.inv(W)).max() <= 1e-12 * np.abs(np.linalg.inv(W)).max() * np.linalg.cond(W) * 10


def test_checker_single_edge_with_one_end_held():
    c = pc.make("one", 2, seed=41, fixed=(0,))
    e = c["edges"][0]
    _, _, Jj = po.edge_terms(c["poses"], e)
    J, _ = co.query(c["poses"], c["fixed"], c["edges"], [(0, 1)])
    want = np.linalg.inv(Jj.T @ np.asarray(e[3]) @ Jj)
    assert np.abs(J[0][3:, 3:] - want).max() <= 1e-13 * np.abs(want).max()
    assert np.all(J[0][:3, :] == 0.0) and np.all(J[0][:, :3] == 0.0)


# ------------------------------------------------------------------------------------------------ the twin: known answers
@pytest.mark.parametrize("fixed_at", [0, 3, 6])
def test_twin_relative_of_a_chain_edge_is_its_inverse_information(twin, fixed_at):
    c = chain(7, fixed_at)
    q = [(a, a + 1) for a in range(6)]
    rc, r = pgc.covariance(twin, c["poses"], c["fixed"], c["edges"], q, pcg_tolerance=TOL)
    assert rc == abi.OK
    for k, (a, b) in enumerate(q):
        want = np.linalg.inv(np.asarray(c["edges"][a][3]))
        assert np.abs(r["relative"][k] - want).max() <= 1e-11 * np.abs(want).max()


def test_twin_single_edge_with_one_end_held(twin):
    c = pc.make("one", 2, seed=41, fixed=(0,))
    e = c["edges"][0]
    _, _, Jj = po.edge_terms(c["poses"], e)
    rc, r = pgc.covariance(twin, c["poses"], c["fixed"], c["edges"], [(0, 1)], pcg_tolerance=TOL)
    assert rc == abi.OK and (r["sources"], r["columns"], r["free_vertices"]) == (1, 3, 1)
    want = np.linalg.inv(Jj.T @ np.asarray(e[3]) @ Jj)
    assert np.abs(r["joint"][0][3:, 3:] - want).max() <= 1e-13 * np.abs(want).max()
    assert np.all(r["joint"][0][:3, :] == 0.0) and np.all(r["joint"][0][:, :3] == 0.0)


# ------------------------------------------------------------------------------------------------ the twin against the checker
@pytest.mark.parametrize("case", DENSE, ids=[c["name"] for c in DENSE])
def test_twin_equals_checker(twin, case):
    q, sources = cc.queries_for(case)
    d, r = deviation(twin, case, q)
    rows = r["free_vertices"]
    print(f"{case['name']}: rows {rows}, sources {r['sources']}, iterations max {r['pcg_iterations_max']}, deviation {d:.3e}")
    assert r["sources"] == len(sources) and r["columns"] == 3 * len(sources) and r["unconverged_columns"] == 0
    if 63 <= rows <= 65:
        assert r["sources"] == min(64, rows)
    assert abs(r["cost"] - po.linearize(case["poses"], case["fixed"], case["edges"])["cost"]) <= 1e-12 * max(r["cost"], 1.0)
    assert d <= bound(rows), d


@pytest.mark.parametrize("name", ["n5_two_fixed", "rows_65", "huber_false_closure"])
def test_joint_is_symmetric_positive_and_transposes_with_the_pair(twin, name):
    case = BY_NAME[name]
    q, _ = cc.queries_for(case)
    rc, r = pgc.covariance(twin, case["poses"], case["fixed"], case["edges"], q, pcg_tolerance=TOL)
    assert rc == abi.OK
    index = {}
    for k, (a, b) in enumerate(q):
        J = r["joint"][k]
        assert np.array_equal(J, J.T), (a, b)
        fa, fb = case["fixed"][a], case["fixed"][b]
        if fa:
            assert np.all(J[:3, :] == 0.0)
        if fb:
            assert np.all(J[3:, :] == 0.0)
        if not fa and not fb and a != b:
            assert np.linalg.eigvalsh(J).min() > 0.0, (a, b)
        if a == b:
            assert np.array_equal(J[:3, :3], J[3:, 3:]) and np.array_equal(J[:3, :3], J[:3, 3:])
        if (a, b) in index:                                                  # a repeated query: the same bytes
            assert np.array_equal(J, r["joint"][index[(a, b)]]) and np.array_equal(r["relative"][k], r["relative"][index[(a, b)]])
        if (b, a) in index:                                                  # the block transpose
            T = r["joint"][index[(b, a)]]
            assert np.array_equal(J[:3, :3], T[3:, 3:]) and np.array_equal(J[3:, 3:], T[:3, :3]) and np.array_equal(J[:3, 3:], T[3:, :3])
        index.setdefault((a, b), k)
    assert any((b, a) in index for (a, b) in index if a != b)


def test_n4096_columns_solve_the_system(twin):
    case = BY_NAME["n4096"]
    q, sources = cc.queries_for(case, count=2)
    rc, r = pgc.covariance(twin, case["poses"], case["fixed"], case["edges"], q, pcg_tolerance=TOL)
    assert rc == abi.OK and r["sources"] == 2 == len(sources) and r["unconverged_columns"] == 0
    rc, L = twin.linearize(case["poses"], case["fixed"], case["edges"])
    assert rc == abi.OK
    row, n = po.rows_of(case["fixed"])
    norm = co.norm_inf(n, row, case["edges"], L["edge_blocks"])
    for s, vtx in enumerate(sources):
        rc, X, it = pgc.columns(twin, s, n)
        assert rc == abi.OK and np.all(it > 0) and it.max() <= r["pcg_iterations_max"]
        for k in range(3):
            res = co.residual_inf(n, row, case["edges"], L["edge_blocks"], X[k], 3 * row[vtx] + k)
            limit = 1000 * EPS * norm * np.abs(X[k]).max()
            print(f"n4096 source {s} column {k}: iterations {it[k]}, residual {res:.3e}, limit {limit:.3e}")
            assert res <= limit
    # the joint is made of these columns
    a, b = sources
    Xa, Xb = pgc.columns(twin, 0, n)[1], pgc.columns(twin, 1, n)[1]
    k = q.index((a, b))
    Sab = 0.5 * (Xb[:, row[a], :].T + Xa[:, row[b], :])
    assert np.array_equal(r["joint"][k][:3, 3:], Sab)


# ------------------------------------------------------------------------------------------------ parameters
def test_an_unconverged_column_is_counted_and_used(twin):
    case = BY_NAME["rows_65"]
    q, _ = cc.queries_for(case, count=2)
    rc, r = pgc.covariance(twin, case["poses"], case["fixed"], case["edges"], q, pcg_tolerance=TOL, max_pcg_iterations=2)
    assert rc == abi.OK and r["unconverged_columns"] > 0 and r["pcg_iterations_max"] == 2
    assert np.all(np.isfinite(r["joint"])) and np.abs(r["joint"]).max() > 0.0


def test_block_jacobi_agrees_with_the_checker(twin):
    case = BY_NAME["rows_65"]
    q, _ = cc.queries_for(case, count=2)
    d, r = deviation(twin, case, q, preconditioner=0)
    d1, r1 = deviation(twin, case, q)
    print(f"rows_65 block-Jacobi: iterations max {r['pcg_iterations_max']} (tridiagonal {r1['pcg_iterations_max']}), deviation {d:.3e}")
    assert r["unconverged_columns"] == 0 and r["pcg_iterations_max"] > r1["pcg_iterations_max"]
    assert d <= bound(65)


def test_a_zero_pivot_of_the_set_up_is_singular(twin):
    """all informations diag(1, 1, 0) on a chain: nothing measures the last vertex's yaw, its pivot is exactly 0"""
    c = chain(6, 0)
    edges = [(e[0], e[1], e[2], np.diag([1.0, 1.0, 0.0]), 0.0) for e in c["edges"]]
    rc, r = pgc.covariance(twin, c["poses"], c["fixed"], edges, [(1, 5)])
    assert rc == pgc.ERR_SINGULAR and "pivot" in twin.last_error()
    assert np.all(r["joint"] == 0.0) and np.all(r["relative"] == 0.0)      # the outputs are not written
    rc, r = pgc.covariance(twin, c["poses"], c["fixed"], c["edges"], [(1, 5)])
    assert rc == abi.OK


def test_a_covariance_call_leaves_the_last_optimize_alone(twin):
    case = BY_NAME["n5_two_fixed"]
    rc, first = twin.optimize(case["poses"], case["fixed"], case["edges"])
    assert rc == abi.OK
    trace, counts = twin.trace(), twin.last_counts()
    other = BY_NAME["rows_63"]
    rc, _ = pgc.covariance(twin, other["poses"], other["fixed"], other["edges"], [(1, 2)])
    assert rc == abi.OK
    assert np.array_equal(twin.trace(), trace) and twin.last_counts() == counts and pgc.last_counts(twin) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ the host plan
def test_plan_orders_the_sources_by_first_appearance():
    case = BY_NAME["n5_fixed_in_the_middle"]                                 # vertex 2 is held
    q = [(3, 1), (2, 3), (4, 4), (1, 2), (0, 4)]
    rc, p = pgc.plan(case["fixed"], case["edges"], q)
    assert rc == abi.OK and p["sources"] == [3, 1, 4, 0]
    assert p["query_sources"].tolist() == [[0, 1], [-1, 0], [2, 2], [1, -1], [3, 2]]


STATUS = {"bad_argument": abi.ERR_BAD_ARGUMENT, "unsupported": abi.ERR_UNSUPPORTED}


@pytest.mark.parametrize("refusal", pc.refusals(), ids=[r[0] for r in pc.refusals()])
def test_every_refusal_of_optimize_applies(twin, refusal):
    name, poses, fixed, edges, status = refusal
    rc, _ = pgc.covariance(twin, poses, fixed, edges, [(0, 1)])
    assert rc == STATUS[status] and twin.last_error() != "", name
    if name != "nan_pose":                                                   # the plan sees no poses
        assert pgc.plan(fixed, edges, [(0, 1)])[0] == STATUS[status]


def test_refusals_of_the_queries_and_parameters(twin):
    case = BY_NAME["rows_65"]
    g = (case["poses"], case["fixed"], case["edges"])
    by_row = cc.vertex_of_rows(case["fixed"])
    for q in ([(0, 66)], [(-1, 2)], [(1, 2)] * 1025):
        assert pgc.covariance(twin, *g, q)[0] == abi.ERR_BAD_ARGUMENT
        assert pgc.plan(case["fixed"], case["edges"], q)[0] == abi.ERR_BAD_ARGUMENT
    assert pgc.covariance(twin, *g, np.zeros((0, 2), np.int32))[0] == abi.ERR_BAD_ARGUMENT
    many = [(int(by_row[r]), int(by_row[r + 1])) for r in range(64)]          # 65 distinct free vertices
    assert pgc.covariance(twin, *g, many)[0] == abi.ERR_UNSUPPORTED
    assert pgc.plan(case["fixed"], case["edges"], many)[0] == abi.ERR_UNSUPPORTED
    assert pgc.plan(case["fixed"], case["edges"], many[:63])[0] == abi.OK    # 64 of them
    for kw in ({"max_pcg_iterations": 0}, {"preconditioner": 2}, {"pcg_tolerance": -1.0}, {"pcg_tolerance": float("nan")}):
        assert pgc.covariance(twin, *g, [(1, 2)], **kw)[0] == abi.ERR_BAD_ARGUMENT
    small = pg.PoseGraph(max_vertices=8, max_edges=8)
    assert pgc.covariance(small, *g, [(1, 2)])[0] == abi.ERR_UNSUPPORTED
    small.close()


def test_a_free_component_without_a_fixed_vertex_is_singular(twin):
    """vertices 4 and 5 hang together and on nothing else: optimize accepts the graph (the damping carries it), Sigma does not exist"""
    c = pc.make("split", 6, seed=42, chain=False, closures=[(0, 1), (1, 2), (2, 3), (0, 3), (4, 5)])
    assert twin.optimize(c["poses"], c["fixed"], c["edges"])[0] == abi.OK
    assert pgc.plan(c["fixed"], c["edges"], [(1, 2)])[0] == pgc.ERR_SINGULAR
    rc, _ = pgc.covariance(twin, c["poses"], c["fixed"], c["edges"], [(1, 2)])
    assert rc == pgc.ERR_SINGULAR and "fixed vertex" in twin.last_error()


# ------------------------------------------------------------------------------------------------ the search window
def test_search_window_against_eigvalsh():
    rng = np.random.default_rng(5)
    for _ in range(20):
        A = rng.normal(size=(3, 3))
        S = A @ A.T * 10.0 ** rng.uniform(-6, 2)
        rc, lin, ang = pgc.search_window(S, 3.0)
        assert rc == abi.OK
        top = np.linalg.eigvalsh(S[:2, :2])[-1]
        assert abs(lin - 3.0 * np.sqrt(top)) <= 1e-14 * lin and abs(ang - 3.0 * np.sqrt(S[2, 2])) <= 1e-15 * ang
    assert pgc.search_window(np.diag([4.0, 1.0, 0.25]), 2.0) == (abi.OK, 4.0, 1.0)
    assert pgc.search_window(np.zeros((3, 3)), 2.0) == (abi.OK, 0.0, 0.0)
    bad = np.diag([1.0, 1.0, 1.0])
    for S in (bad * np.nan, np.diag([-1.0, 1.0, 1.0]), np.diag([1.0, -1.0, 1.0]), np.diag([1.0, 1.0, -1.0]), np.diag([np.inf, 1.0, 1.0])):
        assert pgc.search_window(S, 1.0)[0] == abi.ERR_BAD_ARGUMENT
    for sigmas in (-1.0, float("nan"), float("inf")):
        assert pgc.search_window(bad, sigmas)[0] == abi.ERR_BAD_ARGUMENT


def test_window_of_a_closure_candidate_grows_along_the_chain(twin):
    """the farther the scan's vertex from the sub-map's anchor along an open chain, the wider the window"""
    c = chain(30, 0, seed=43)
    rc, r = pgc.covariance(twin, c["poses"], c["fixed"], c["edges"], [(2, 4), (2, 12), (2, 29)])
    assert rc == abi.OK
    w = [pgc.search_window(R, 3.0) for R in r["relative"]]
    assert all(x[0] == abi.OK for x in w)
    assert w[0][1] < w[1][1] < w[2][1] and w[0][2] < w[1][2] < w[2][2]


if __name__ == "__main__":                                                   # the figures of the docstring
    g = pg.PoseGraph()
    for case in DENSE:
        d, r = deviation(g, case, cc.queries_for(case)[0])
        print(f"{case['name']:28s} rows {r['free_vertices']:5d} sources {r['sources']:3d} iterations max {r['pcg_iterations_max']:4d} deviation {d:.3e}")
