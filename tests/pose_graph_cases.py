"""The graphs the pose-graph tests share (tests/test_pose_graph.py on the CPU, tests/test_gpu_pose_graph.py on the device):
a synthetic trajectory, its odometry chain and k closures with full 3 x 3 informations, in the shapes that take another path in
the plan, the cyclic reduction or the lane sums.  A case is a dict: name, poses (the start), truth, fixed, edges (tuples
(i, j, z, information, huber_delta)), params (keyword arguments of optimize) and `dense` (small enough for the dense checker)."""
import numpy as np

import pose_graph_oracle as po


def _information(rng, scale=1.0):
    A = rng.normal(size=(3, 3))
    W = A @ A.T + np.diag([4.0, 4.0, 8.0])
    return scale * 0.5 * (W + W.T)


def trajectory(N, yaw0=0.0, laps=2.0):
    """N poses on `laps` rounds of a circle of circumference 0.5 N / laps, yaw continuous (not wrapped)"""
    out = np.zeros((N, 3))
    step = 0.5
    dyaw = 2.0 * np.pi * laps / max(N, 8)
    p = np.array([0.0, 0.0, yaw0])
    for i in range(N):
        out[i] = p
        p = po.compose(p, np.array([step, 0.0, dyaw]))
    return out


def make(name, N, k=0, seed=0, fixed=(0,), noise=0.01, start_noise=(0.05, 0.02), yaw0=0.0, wrap=False, reverse=False, closures=None,
         chain=True, huber=0.0, params=None, dense=True, extra=None, laps=2.0, chain_scale=1.0):
    rng = np.random.default_rng(seed)
    truth = trajectory(N, yaw0, laps)
    fx = np.zeros(N, dtype=np.uint8)
    fx[list(fixed)] = 1
    edges = []

    def add(i, j, hub=0.0, z=None, scale=1.0):
        zz = po.between(truth[i], truth[j]) + noise * rng.normal(size=3) * np.array([1.0, 1.0, 0.5]) if z is None else np.asarray(z, dtype=np.float64)
        edges.append((int(i), int(j), zz, _information(rng, scale), hub))

    if chain:
        for i in range(N - 1):
            add(i + 1, i, scale=chain_scale) if reverse else add(i, i + 1, scale=chain_scale)
    if closures is None:
        closures = []
        while len(closures) < k:
            i, j = sorted(int(v) for v in rng.integers(0, N, size=2))
            if j - i >= 2:
                closures.append((i, j))
    for i, j in closures:
        add(i, j, huber)
    for e in (extra or []):
        add(*e)
    start = truth + rng.normal(size=(N, 3)) * np.array([start_noise[0], start_noise[0], start_noise[1]])
    start[fx != 0] = truth[fx != 0]
    if wrap:                                                                # the yaws as a front end hands them out: in (-pi, pi]
        start[:, 2] -= po.TWO_PI * np.rint(start[:, 2] / po.TWO_PI)
    return {"name": name, "poses": start, "truth": truth, "fixed": fx, "edges": edges, "params": dict(params or {}), "dense": dense, "k": len(closures)}


def cases():
    out = [
        make("n2_one_edge", 2, fixed=(1,), seed=1),
        make("n3", 3, seed=2, closures=[(0, 2)]),
        make("n5_fixed_in_the_middle", 5, fixed=(2,), seed=3, closures=[(0, 4)]),
        make("n5_two_fixed", 5, fixed=(0, 4), seed=4, closures=[(1, 3)]),
        make("edge_between_two_fixed", 6, fixed=(0, 1), seed=5, closures=[(0, 5)]),
        make("duplicate_edges", 6, seed=6, closures=[(0, 3), (0, 3), (1, 2), (2, 1)]),
        make("edges_given_j_below_i", 12, seed=7, reverse=True, closures=[(0, 11), (3, 9)]),
        make("rows_63", 64, k=3, seed=8),
        make("rows_64", 65, k=3, seed=9),
        make("rows_65", 66, k=3, seed=10),
        make("rows_1023", 1024, k=4, seed=11, params={"max_iterations": 3}),
        make("rows_1024", 1025, k=4, seed=12, params={"max_iterations": 3}),
        make("rows_1025", 1026, k=4, seed=13, params={"max_iterations": 3}),
        make("n4096", 4096, k=8, seed=14, params={"max_iterations": 3}, dense=False),
        # no chain edge at all: every edge links rows two apart (vertex 0 is held and has no row)
        # (with as many edges as free vertices the cost falls to 0 and a rho sat on the edge of acceptance: the edges three apart
        # make the case over-determined)
        make("no_chain_edges", 11, seed=15, chain=False, closures=[(i, i + 2) for i in range(9)] + [(0, 1)] + [(i, i + 3) for i in range(1, 8)]),
        # a false closure between places two metres apart, under the robust kernel (the true closures carry it too); the odometry is
        # a hundred times as certain as a closure, so bending the chain costs more than the kernel charges for the false edge
        make("huber_false_closure", 40, seed=16, closures=[(2, 30), (5, 35)], huber=1.0, extra=[(10, 25, 1.0, (0.1, 0.0, 0.0))], chain_scale=100.0),
        # yaws that cross +-pi along the way, handed in wrapped
        make("yaw_across_pi", 48, seed=17, yaw0=2.9, wrap=True, closures=[(0, 24), (10, 40)], laps=1.5),
        # a start that is out by more than the rotation bound allows in one call
        make("rotation_beyond_the_bound", 4, seed=18, closures=[(0, 3)], start_noise=(0.05, 0.0)),
    ]
    out[-1]["poses"][1:, 2] += 1.4
    return out


def refusals():
    """(name, poses, fixed, edges, expected status name) — each differs from a sound graph in one thing"""
    base = make("base", 5, seed=20, closures=[(0, 4)])
    W = base["edges"][0][3]

    def with_edge(e):
        return base["edges"][:-1] + [e]

    nan_pose = base["poses"].copy(); nan_pose[3, 1] = np.nan
    none_fixed = np.zeros(5, dtype=np.uint8)
    lonely = make("lonely", 5, seed=21, chain=False, closures=[(0, 1), (1, 2), (2, 3)])          # vertex 4 is free and has no edge
    indefinite = np.diag([1.0, -1.0, 1.0])
    asym = W.copy(); asym[0, 1] += 0.5
    return [
        ("nan_pose", nan_pose, base["fixed"], base["edges"], "bad_argument"),
        ("nan_measurement", base["poses"], base["fixed"], with_edge((0, 4, np.array([np.inf, 0.0, 0.0]), W, 0.0)), "bad_argument"),
        ("nan_information", base["poses"], base["fixed"], with_edge((0, 4, np.zeros(3), W * np.nan, 0.0)), "bad_argument"),
        ("index_out_of_range", base["poses"], base["fixed"], with_edge((0, 5, np.zeros(3), W, 0.0)), "bad_argument"),
        ("negative_index", base["poses"], base["fixed"], with_edge((-1, 4, np.zeros(3), W, 0.0)), "bad_argument"),
        ("i_equals_j", base["poses"], base["fixed"], with_edge((3, 3, np.zeros(3), W, 0.0)), "bad_argument"),
        ("indefinite_information", base["poses"], base["fixed"], with_edge((0, 4, np.zeros(3), indefinite, 0.0)), "bad_argument"),
        ("asymmetric_information", base["poses"], base["fixed"], with_edge((0, 4, np.zeros(3), asym, 0.0)), "bad_argument"),
        ("negative_huber", base["poses"], base["fixed"], with_edge((0, 4, np.zeros(3), W, -1.0)), "bad_argument"),
        ("no_fixed_vertex", base["poses"], none_fixed, base["edges"], "bad_argument"),
        ("free_vertex_without_an_edge", lonely["poses"], lonely["fixed"], lonely["edges"], "bad_argument"),
    ]
