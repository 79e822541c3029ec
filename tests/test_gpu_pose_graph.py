"""The 2-D pose graph on the GPU (include/visfs_pose_graph.h on a visfs_ba handle: k_pose_graph, one workgroup of 1024 work items
for the whole optimisation) against the one-core host twin, byte for byte: the poses, chi2, the record, the whole trace and the
linearize and precondition hooks, on every case of tests/pose_graph_cases.py.  tests/test_pose_graph.py holds the twin to the
NumPy checker on the same cases."""
import numpy as np
import pytest

import pose_graph_cases as pc
from visfs_amd import abi, backend
from visfs_amd import pose_graph as pg

pytestmark = pytest.mark.gpu

CASES = pc.cases()
BY_NAME = {c["name"]: c for c in CASES}


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


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_twin(pair, case):
    dev, host = pair
    out = []
    for g in (dev, host):
        rc, r = g.optimize(case["poses"], case["fixed"], case["edges"], pcg_tolerance=1e-13, **case["params"])
        assert rc == abi.OK, g.last_error()
        out.append((r, g.trace()))
    (rd, td), (rh, th) = out
    assert rd["bytes"] == rh["bytes"], ({k: rd[k] for k in ("iterations", "trials", "termination", "pcg_iterations", "initial_cost", "final_cost")},
                                        {k: rh[k] for k in ("iterations", "trials", "termination", "pcg_iterations", "initial_cost", "final_cost")})
    same_bytes(rd["poses"], rh["poses"], "poses")
    same_bytes(rd["chi2"], rh["chi2"], "chi2")
    same_bytes(td, th, "trace")
    assert rd["trials"] == len(td) and rd["trials"] > 0
    assert dev.last_counts() == (1, 2, 1) and host.last_counts() == (0, 0, 0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_hooks_on_the_device_equal_the_twin(pair, case):
    dev, host = pair
    (sd, Ld), (sh, Lh) = dev.linearize(case["poses"], case["fixed"], case["edges"]), host.linearize(case["poses"], case["fixed"], case["edges"])
    assert sd == sh == abi.OK, (dev.last_error(), host.last_error())
    assert Ld["rows"] == Lh["rows"] and Ld["cost"].hex() == Lh["cost"].hex()
    for k in ("edge_blocks", "g", "D", "C", "chi2"):
        same_bytes(Ld[k], Lh[k], k)
    lam = 1e-5 * float(np.max(Lh["D"][:, [0, 1, 2], [0, 1, 2]]))
    r = np.random.default_rng(3).normal(size=(Lh["rows"], 3))
    for preconditioner in (1, 0):
        (sd, zd), (sh, zh) = (g.precondition(case["poses"], case["fixed"], case["edges"], lam, r, preconditioner) for g in (dev, host))
        assert sd == sh == abi.OK
        same_bytes(zd, zh, f"M^-1 r, preconditioner {preconditioner}")
        assert np.all(np.isfinite(zd)) and np.abs(zd).max() > 0.0


def test_default_parameters_and_block_jacobi_equal_the_twin(pair):
    dev, host = pair
    case = BY_NAME["rows_65"]
    for kw in ({}, {"preconditioner": 0, "max_iterations": 2}):
        out = []
        for g in (dev, host):
            rc, r = g.optimize(case["poses"], case["fixed"], case["edges"], **kw)
            assert rc == abi.OK
            out.append((r, g.trace()))
        assert out[0][0]["bytes"] == out[1][0]["bytes"]
        same_bytes(out[0][0]["poses"], out[1][0]["poses"], "poses")
        same_bytes(out[0][1], out[1][1], "trace")


def test_a_call_after_a_refusal(pair):
    dev, host = pair
    case = BY_NAME["n5_two_fixed"]
    rc, first = dev.optimize(case["poses"], case["fixed"], case["edges"])
    assert rc == abi.OK
    trace = dev.trace()
    name, poses, fixed, edges, _ = pc.refusals()[0]
    assert dev.optimize(poses, fixed, edges)[0] == abi.ERR_BAD_ARGUMENT and dev.last_error() != ""
    same_bytes(dev.trace(), trace, "the hook data of the last call stay")
    rc, again = dev.optimize(case["poses"], case["fixed"], case["edges"])
    assert rc == abi.OK and again["bytes"] == first["bytes"]
    same_bytes(again["poses"], first["poses"], "poses")
    assert dev.last_counts() == (1, 2, 1)


def test_pcg_budget_on_the_device(pair):
    dev, host = pair
    case = BY_NAME["rows_63"]
    out = []
    for g in (dev, host):
        rc, r = g.optimize(case["poses"], case["fixed"], case["edges"], pcg_budget=30, pcg_tolerance=1e-13)
        assert rc == abi.OK
        assert r["termination"] == 4 and r["pcg_iterations"] == 30
        out.append(r)
    assert out[0]["bytes"] == out[1]["bytes"]
    same_bytes(out[0]["poses"], out[1]["poses"], "poses")
