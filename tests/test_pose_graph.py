"""The 2-D pose graph's one-core host twin (include/visfs_pose_graph.h with a NULL handle) against the NumPy checker
(tests/pose_graph_oracle.py) on the cases of tests/pose_graph_cases.py, the checker against known answers, the theory behind the
preconditioner, the host plan and the helper that turns a scan refinement into an edge.  tests/test_gpu_pose_graph.py holds the
device to the twin byte for byte on the same cases.

Bounds.  With pcg_tolerance = 1e-13 the twin's steps are the dense solves of the checker up to rounding, so both run the same
accept/reject sequence.  Measured on the CPU over all dense cases: poses differ by at most 5.6e-14 (rows_1024), costs by at most
2.5e-14 relative; the bounds asserted are 100 times that."""
import numpy as np
import pytest

import pose_graph_cases as pc
import pose_graph_oracle as po
from visfs_amd import abi
from visfs_amd import pose_graph as pg
from visfs_amd import scan_refine as sr

CASES = pc.cases()
DENSE = [c for c in CASES if c["dense"]]
POSE_BOUND = 5.6e-12         # 100 x the largest deviation measured (5.6e-14)
COST_BOUND = 2.5e-12         # 100 x the largest relative deviation measured (2.5e-14)
EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def twin(hiplib):
    g = pg.PoseGraph()
    yield g
    g.close()


@pytest.fixture(scope="module")
def solved(twin):
    """every case through the twin once: name -> (record, trace)"""
    out = {}
    for c in CASES:
        rc, r = twin.optimize(c["poses"], c["fixed"], c["edges"], pcg_tolerance=1e-13, **c["params"])
        assert rc == abi.OK, (c["name"], twin.last_error())
        out[c["name"]] = (r, twin.trace())
    return out


def noise_free(N, seed, closures):
    c = pc.make("noise_free", N, seed=seed, noise=0.0, closures=closures, start_noise=(0.1, 0.05))
    return c


# ------------------------------------------------------------------------------------------------ the checker alone, first
def test_checker_returns_the_truth_from_noise_free_measurements():
    c = noise_free(12, 31, [(0, 11), (2, 8)])
    o = po.optimize(c["poses"], c["fixed"], c["edges"], max_iterations=50, function_tolerance=0.0)
    assert np.abs(o["poses"] - c["truth"]).max() <= 1e-9


def test_checker_single_edge_returns_z_on_the_fixed_pose():
    a, z = np.array([0.4, -1.2, 0.7]), np.array([0.8, 0.3, -0.4])
    start = np.array([a, po.compose(a, z) + np.array([0.2, -0.1, 0.3])])
    o = po.optimize(start, [1, 0], [(0, 1, z, np.diag([3.0, 2.0, 5.0]), 0.0)], max_iterations=50, function_tolerance=0.0)
    assert np.abs(o["poses"][1] - po.compose(a, z)).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ the twin: known answers
def test_twin_returns_the_truth_from_noise_free_measurements(twin):
    c = noise_free(12, 31, [(0, 11), (2, 8)])
    rc, r = twin.optimize(c["poses"], c["fixed"], c["edges"], max_iterations=50, function_tolerance=0.0)
    assert rc == abi.OK
    assert np.abs(r["poses"] - c["truth"]).max() <= 1e-9


def test_twin_single_edge_returns_z_on_the_fixed_pose(twin):
    a, z = np.array([0.4, -1.2, 0.7]), np.array([0.8, 0.3, -0.4])
    start = np.array([a, po.compose(a, z) + np.array([0.2, -0.1, 0.3])])
    for edge, fixed in (((0, 1, z, np.diag([3.0, 2.0, 5.0]), 0.0), [1, 0]),):
        rc, r = twin.optimize(start, fixed, [edge], max_iterations=50, function_tolerance=0.0)
        assert rc == abi.OK
        assert np.abs(r["poses"][1] - po.compose(a, z)).max() <= 1e-9
        assert np.array_equal(r["poses"][0], a)


# ------------------------------------------------------------------------------------------------ the hooks
def dense_from_blocks(case, blocks):
    row, n = po.rows_of(case["fixed"])
    H = np.zeros((3 * n, 3 * n))
    for e, b in zip(case["edges"], blocks):
        a, c = row[e[0]], row[e[1]]
        if a >= 0:
            H[3 * a:3 * a + 3, 3 * a:3 * a + 3] += b[0]
        if c >= 0:
            H[3 * c:3 * c + 3, 3 * c:3 * c + 3] += b[2]
        if a >= 0 and c >= 0:
            H[3 * a:3 * a + 3, 3 * c:3 * c + 3] += b[1]
            H[3 * c:3 * c + 3, 3 * a:3 * a + 3] += b[1].T
    return H


@pytest.mark.parametrize("case", DENSE, ids=[c["name"] for c in DENSE])
def test_linearize_hook_against_the_dense_system(twin, case):
    """Every entry of H and g is a sum of at most (edges at the vertex) terms, each a product of three 3 x 3 factors: the bound is
    64 ulp of the largest entry per term summed, far above the few ulp each term can be off and far below any wrong term."""
    rc, L = twin.linearize(case["poses"], case["fixed"], case["edges"])
    assert rc == abi.OK, twin.last_error()
    o = po.linearize(case["poses"], case["fixed"], case["edges"])
    n = o["rows"]
    assert L["rows"] == n
    degree = int(np.bincount(np.array([[e[0], e[1]] for e in case["edges"]]).reshape(-1)).max())
    tol = 64 * EPS * degree
    H = dense_from_blocks(case, L["edge_blocks"])
    top = np.abs(o["H"]).max()
    assert np.abs(H - o["H"]).max() <= tol * top
    assert np.abs(L["g"].reshape(-1) - o["g"]).max() <= tol * max(top * np.abs(o["chi2"]).max() ** 0.5, np.abs(o["g"]).max())
    assert np.abs(L["chi2"] - o["chi2"]).max() <= 64 * EPS * max(np.abs(o["chi2"]).max(), 1e-300)
    assert abs(L["cost"] - o["cost"]) <= 64 * EPS * len(case["edges"]) ** 0.5 * o["cost"] + 1e-300
    for r in range(n):                                                     # D and C are the band of the same H
        assert np.abs(L["D"][r] - o["H"][3 * r:3 * r + 3, 3 * r:3 * r + 3]).max() <= tol * top
        want = o["H"][3 * r:3 * r + 3, 3 * r + 3:3 * r + 6] if r + 1 < n else np.zeros((3, 3))
        assert np.abs(L["C"][r] - want).max() <= tol * top


PRECONDITION = [c for c in DENSE if len(c["fixed"]) <= 70] + [c for c in DENSE if c["name"] == "rows_1025"]


@pytest.mark.parametrize("preconditioner", [1, 0])
@pytest.mark.parametrize("case", PRECONDITION, ids=[c["name"] for c in PRECONDITION])
def test_precondition_hook_against_the_dense_solve(twin, case, preconditioner):
    """z = M^-1 r by cyclic reduction against numpy.linalg.solve on the dense band: both are backward stable on the symmetric
    positive definite M, so they differ by a modest multiple of cond(M) eps |z|; 100 cond(M) eps is asserted (the prototype's
    1.4e-14 .. 1.1e-13 at cond about 1e2 .. 1e3)."""
    o = po.linearize(case["poses"], case["fixed"], case["edges"])
    lam = 1e-5 * np.max(np.diag(o["H"]))
    rng = np.random.default_rng(5)
    r = rng.normal(size=(o["rows"], 3))
    rc, z = twin.precondition(case["poses"], case["fixed"], case["edges"], lam, r, preconditioner)
    assert rc == abi.OK, twin.last_error()
    want = po.precondition(o["H"], lam, r, preconditioner)
    ev = np.linalg.eigvalsh(po.band(o["H"], preconditioner) + lam * np.eye(3 * o["rows"]))
    cond = ev[-1] / ev[0]
    dev = np.abs(z - want).max() / np.abs(want).max()
    print(case["name"], "preconditioner", preconditioner, "cond", cond, "deviation", dev)
    assert dev <= 100 * cond * EPS


# ------------------------------------------------------------------------------------------------ the optimisation
@pytest.fixture(scope="module")
def checked():
    return {}


def checker(checked, case):
    if case["name"] not in checked:
        checked[case["name"]] = po.optimize(case["poses"], case["fixed"], case["edges"], max_iterations=case["params"].get("max_iterations", 20))
    return checked[case["name"]]


@pytest.mark.parametrize("case", DENSE, ids=[c["name"] for c in DENSE])
def test_twin_follows_the_checker(solved, checked, case):
    r, trace = solved[case["name"]]
    o = checker(checked, case)
    assert trace[:, 2].tolist() == o["trace"][:, 2].tolist()                # the same accept / reject sequence
    assert (r["iterations"], r["trials"], r["termination"]) == (o["iterations"], o["trials"], o["termination"])
    dp = np.abs(r["poses"] - o["poses"]).max()
    # relative; a final cost that is zero up to rounding (a graph with as many measurements as unknowns) is held to eps of the initial one
    dc = max(abs(r["final_cost"] - o["final_cost"]) / max(o["final_cost"], EPS * o["initial_cost"]),
             abs(r["initial_cost"] - o["initial_cost"]) / o["initial_cost"])
    print(case["name"], "pose deviation", dp, "relative cost deviation", dc)
    assert dp <= POSE_BOUND
    assert dc <= COST_BOUND
    assert np.abs(r["chi2"] - o["chi2"]).max() <= COST_BOUND * max(o["chi2"].max(), o["final_cost"])
    ok = trace[:, 0] < po.REJECTED
    assert np.abs(trace[ok, 0] - o["trace"][ok, 0]).max() <= COST_BOUND * o["initial_cost"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_costs_never_rise(solved, case):
    r, trace = solved[case["name"]]
    assert r["final_cost"] <= r["initial_cost"]
    accepted = trace[trace[:, 2] == 1.0, 0]
    costs = np.concatenate([[r["initial_cost"]], accepted])
    assert np.all(np.diff(costs) < 0.0)
    assert r["final_cost"] == costs[-1]
    assert r["trials"] == len(trace) and r["pcg_iterations"] == int(trace[:, 3].sum())


def test_the_cases_do_what_they_are_there_for(solved):
    truth = {c["name"]: c for c in CASES}
    r, _ = solved["huber_false_closure"]
    false_edge = len(truth["huber_false_closure"]["edges"]) - 1
    assert r["chi2"][false_edge] > 100.0 * np.delete(r["chi2"], false_edge).max()          # the false closure is left unsatisfied
    # the false edge asks two poses 2.2 m apart to lie 0.1 m apart; the kernel's constant pull is allowed a seventh of that
    assert np.abs(r["poses"][:, :2] - truth["huber_false_closure"]["truth"][:, :2]).max() < 0.3
    r, _ = solved["yaw_across_pi"]
    d = r["poses"] - truth["yaw_across_pi"]["truth"]
    d[:, 2] -= po.TWO_PI * np.rint(d[:, 2] / po.TWO_PI)
    assert np.abs(d).max() < 0.1
    r, _ = solved["rotation_beyond_the_bound"]
    assert r["termination"] == po.ROTATION_BOUND and np.abs(r["poses"][:, 2] - truth["rotation_beyond_the_bound"]["poses"][:, 2]).max() <= 1.0


def test_calling_again_from_the_returned_poses_passes_the_rotation_bound(twin):
    c = {x["name"]: x for x in CASES}["rotation_beyond_the_bound"]
    poses, calls = c["poses"], 0
    while True:
        rc, r = twin.optimize(poses, c["fixed"], c["edges"])
        assert rc == abi.OK
        poses, calls = r["poses"], calls + 1
        if r["termination"] != po.ROTATION_BOUND or calls == 8:
            break
    assert 1 < calls < 8
    assert np.abs(poses - c["truth"]).max() < 0.05


# ------------------------------------------------------------------------------------------------ theory
def test_tridiagonal_preconditioner_meets_its_iteration_bound(twin):
    """H - M has rank <= 6 per off-chain edge, so PCG preconditioned by M ends within 6 k + 1 iterations in exact arithmetic:
    N = 512, k = 2, lambda at its first value, tolerance 1e-12.  Measured: 13 with the tridiagonal preconditioner on the twin (the
    checker's dense PCG: 13), 170 with block-Jacobi."""
    c = pc.make("theory", 512, k=2, seed=40)
    counts = {}
    for preconditioner in (1, 0):
        rc, r = twin.optimize(c["poses"], c["fixed"], c["edges"], max_iterations=1, pcg_tolerance=1e-12, max_pcg_iterations=5000,
                              preconditioner=preconditioner)
        assert rc == abi.OK
        counts[preconditioner] = int(twin.trace()[0, 3])
    o = po.linearize(c["poses"], c["fixed"], c["edges"])
    dense, _ = po.pcg_iterations(o["H"], o["g"], 1e-5 * np.max(np.diag(o["H"])), 1e-12, 1)
    print("PCG iterations: tridiagonal", counts[1], "block-Jacobi", counts[0], "checker", dense)
    assert counts[1] <= 6 * 2 + 1
    assert dense <= 6 * 2 + 1
    assert counts[1] < counts[0]


# ------------------------------------------------------------------------------------------------ the helper
def test_edge_from_refine_against_a_finite_difference_propagation():
    anchor = np.array([1.5, -0.7, 2.2])
    rng = np.random.default_rng(9)
    A = rng.normal(size=(3, 3))
    W = A @ A.T + np.eye(3)
    r = sr.Result()
    r.refined, r.x, r.y, r.yaw = 1, 2.1, 0.4, -2.9
    r.information[:] = W.reshape(9).tolist()
    rc, z, Wz = pg.edge_from_refine(anchor, r)
    assert rc == abi.OK
    p = np.array([r.x, r.y, r.yaw])
    assert np.abs(z - po.between(anchor, p)).max() <= 1e-15 * 8
    assert np.abs(po.compose(anchor, z)[:2] - p[:2]).max() <= 1e-14
    # z as a function of the refined pose: J = dz / dp by central differences; the information of z is J^-T W J^-1
    h, J = 1e-6, np.zeros((3, 3))
    for k in range(3):
        d = np.zeros(3); d[k] = h
        J[:, k] = (po.between(anchor, p + d) - po.between(anchor, p - d)) / (2 * h)
    Ji = np.linalg.inv(J)
    want = Ji.T @ W @ Ji
    assert np.abs(Wz - want).max() <= 1e-8 * np.abs(want).max()
    assert np.array_equal(Wz, Wz.T)
    r.refined = 0
    assert pg.edge_from_refine(anchor, r)[0] == abi.ERR_BAD_ARGUMENT


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_lists_on_hand_made_graphs(hiplib):
    W = np.eye(3)
    z = np.zeros(3)
    # vertices 0 .. 5, 2 held: rows 0 1 - 2 3 4.  Edges in this order:
    edges = [(0, 1, z, W), (1, 2, z, W), (3, 2, z, W), (4, 3, z, W), (1, 3, z, W), (5, 0, z, W), (3, 4, z, W), (4, 5, z, W)]
    rc, p = pg.plan([0, 0, 1, 0, 0, 0], edges)
    assert rc == abi.OK
    assert p["rows"] == 5 and p["row_of"] == [0, 1, -1, 2, 3, 4]
    assert p["inc"] == [[(0, 0), (5, 1)], [(0, 1), (1, 0), (4, 0)], [(2, 0), (3, 1), (4, 1), (6, 0)], [(3, 0), (6, 1), (7, 0)], [(5, 0), (7, 1)]]
    # row 1 (vertex 1) and row 2 (vertex 3) are neighbours though vertex 2 lies between them: edge 4 is a chain edge
    assert p["chain"] == [[(0, 0)], [(4, 0)], [(3, 1), (6, 0)], [(7, 0)], []]
    rc, p = pg.plan([1, 0], [(1, 0, z, W), (0, 1, z, W)])
    assert rc == abi.OK and p["rows"] == 1 and p["inc"] == [[(0, 0), (1, 1)]] and p["chain"] == [[]]


# ------------------------------------------------------------------------------------------------ refusals
STATUS = {"bad_argument": abi.ERR_BAD_ARGUMENT, "unsupported": abi.ERR_UNSUPPORTED}


@pytest.mark.parametrize("refusal", pc.refusals(), ids=[r[0] for r in pc.refusals()])
def test_refusals(twin, refusal):
    name, poses, fixed, edges, status = refusal
    rc, _ = twin.optimize(poses, fixed, edges)
    assert rc == STATUS[status], name
    assert twin.last_error() != ""


def test_limits_and_parameters_are_refused(hiplib, twin):
    small = pg.PoseGraph(max_vertices=4, max_edges=4)
    c = pc.make("five", 5, seed=50)
    assert small.optimize(c["poses"], c["fixed"], c["edges"])[0] == abi.ERR_UNSUPPORTED          # N = 5 > 4
    c = pc.make("four", 4, seed=51, closures=[(0, 2), (0, 3)])
    assert small.optimize(c["poses"], c["fixed"], c["edges"])[0] == abi.ERR_UNSUPPORTED          # E = 5 > 4
    c = pc.make("four", 4, seed=51)
    assert small.optimize(c["poses"], c["fixed"], c["edges"])[0] == abi.OK                       # and the object still works
    small.close()
    for kw in ({"max_vertices": 4097}, {"max_edges": 65537}):
        with pytest.raises(Exception):
            pg.PoseGraph(**kw)
    for kw in ({"max_iterations": 0}, {"max_iterations": 51}, {"pcg_tolerance": -1.0}, {"function_tolerance": float("nan")},
               {"max_pcg_iterations": 0}, {"pcg_budget": 0}, {"preconditioner": 2}):
        assert twin.optimize(c["poses"], c["fixed"], c["edges"], **kw)[0] == abi.ERR_BAD_ARGUMENT, kw


def test_pcg_budget_ends_the_call(twin):
    c = {x["name"]: x for x in CASES}["rows_63"]
    rc, r = twin.optimize(c["poses"], c["fixed"], c["edges"], pcg_budget=30, pcg_tolerance=1e-13)
    assert rc == abi.OK
    assert r["termination"] == po.PCG_BUDGET and r["pcg_iterations"] == 30
    assert r["final_cost"] <= r["initial_cost"] and r["trials"] == len(twin.trace())
