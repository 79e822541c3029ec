"""The PnP-RANSAC pose guess on the GPU (include/visfs_pnp.h): the device path against the host twin byte for byte — every
hypothesis's sample, validity flag, model and count, the winner, every refinement pass's model, threshold and inlier list, and the
transform, covariance, matches and inliers — at the wavefront and workgroup edges of both kernels, with NaN rows, with and without
to_xyz, on degenerate inputs, and with two objects and a BA solve on one handle."""
import numpy as np
import pytest

import pnp_cases as pc
from visfs_amd import abi, backend, pnp, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


@pytest.fixture(scope="module")
def pair(solver):
    dev, host = pnp.Pnp(pnp.MAX_POINTS, solver=solver), pnp.Pnp(pnp.MAX_POINTS)
    yield dev, host
    dev.close(); host.close()


CAM = dict(zip(("fx", "fy", "cx", "cy"), pc.K))


def _same_call(dev, host, prm, from_xyz, to_xy, to_xyz=None):
    cam = pnp.camera(Tir=pc.TIR, **CAM)
    ra, a = dev.solve_status(pnp.default_params(**prm), cam, from_xyz, to_xy, to_xyz)
    rb, b = host.solve_status(pnp.default_params(**prm), cam, from_xyz, to_xy, to_xyz)
    assert ra == rb == abi.OK
    sa, sb = dev.download(), host.download()
    for key in sorted(sb):
        assert np.asarray(sa[key]).tobytes() == np.asarray(sb[key]).tobytes(), key
    for key in sorted(b):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert not np.isnan(a["T"]).any() and not np.isnan(a["cov"]).any() and np.isfinite(sa["models"]).all()
    return a, sa


@pytest.mark.parametrize("rows", pc.DEVICE_ROWS)
def test_rows_at_the_edges_equal_the_host_twin(pair, rows):
    s = pc.scene(rows, 0.3 if rows >= 20 else 0.0, 50 + rows)
    prm = pc.params_dict(min_inliers=min(12, rows))
    for to in (s["to_xyz"], None):
        out, st = _same_call(*pair, prm, s["from_xyz"], s["to_xy"], to)
        assert st["m"] == rows and st["winner"] >= 0 and len(out["inliers"]) >= min(12, rows) and len(st["pass_count"]) >= 1
        if rows >= 20:                                      # (four or five noisy rows do not pin the pose to the scene's truth)
            rot, dist = pc.pose_error(out["T"], s["truth"])
            assert rot < 0.01 and dist < 0.05


@pytest.mark.parametrize("iterations", pc.DEVICE_ITERATIONS)
def test_hypothesis_counts_at_the_edges_equal_the_host_twin(pair, iterations):
    s = pc.scene(150, 0.35, 70)
    out, st = _same_call(*pair, pc.params_dict(iterations=iterations), s["from_xyz"], s["to_xy"], s["to_xyz"])
    assert len(st["valid"]) == iterations and st["counts"].max() == st["counts"][st["winner"]]
    assert st["winner"] == int(np.argmax(np.where(st["valid"] == 1, st["counts"], -1)))      # ties to the lowest index


def test_committed_cases_equal_the_host_twin(pair):
    passes = set()
    for name in sorted(pc.CASES):
        s = pc.case(name)
        out, st = _same_call(*pair, s["params"], s["from_xyz"], s["to_xy"], s["to_xyz"] if s["with_to_xyz"] else None)
        passes.add(len(st["pass_count"]))
        assert len(out["inliers"]) >= 4
    assert max(passes) > 1                                   # the loop of step 6 ran more than once on the device


def test_nan_rows_and_other_seeds_equal_the_host_twin(pair):
    s = pc.scene(80, 0.2, 41, nan_rows=9)
    out, st = _same_call(*pair, pc.params_dict(), s["from_xyz"], s["to_xy"], s["to_xyz"])
    assert st["m"] == 71 and len(out["matches"]) == 71 and np.isfinite(s["from_xyz"][out["inliers"]]).all()
    for seed in (1, 2 ** 63 + 5):
        _same_call(*pair, pc.params_dict(seed=seed, refine_iterations=32, refine_sigma=1.5), s["from_xyz"], s["to_xy"], None)


@pytest.mark.parametrize("name", sorted(pc.degenerate_inputs()))
def test_degenerate_inputs_give_the_zero_transform(pair, name):
    prm, from_xyz, to_xy = pc.degenerate_inputs()[name]
    out, st = _same_call(*pair, prm, from_xyz, to_xy)
    assert (out["T"] == 0).all() and len(out["inliers"]) == 0 and (out["cov"] == np.eye(6)).all()
    assert np.isfinite(st["refit_tq"]).all() and np.isfinite(st["pass_tq"]).all() and np.isfinite(st["pass_threshold"]).all()


def test_argument_checks_on_the_device(solver, pair):
    dev, _ = pair
    s = pc.scene(20, 0.0, 3)
    cam = pnp.camera(Tir=pc.TIR, **CAM)
    assert dev.solve_status(pnp.default_params(iterations=0), cam, s["from_xyz"], s["to_xy"])[0] == abi.ERR_BAD_ARGUMENT
    assert dev.solve_status(pnp.default_params(iterations=4097), cam, s["from_xyz"], s["to_xy"])[0] == abi.ERR_UNSUPPORTED
    assert dev.solve_status(pnp.default_params(reproj_error=float("nan")), cam, s["from_xyz"], s["to_xy"])[0] == abi.ERR_BAD_ARGUMENT
    small = pnp.Pnp(16, solver=solver)
    assert small.solve_status(pnp.default_params(), cam, s["from_xyz"], s["to_xy"])[0] == abi.ERR_BAD_ARGUMENT
    small.close()
    with pytest.raises(backend.BackendError):
        pnp.Pnp(4097, solver=solver)


def test_two_objects_and_a_ba_solve_on_one_handle(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    a, b, host = pnp.Pnp(400, solver=solver), pnp.Pnp(64, solver=solver), pnp.Pnp(400)
    sa, sb = pc.case("m300_out40"), pc.case("m64_out30")
    cam = pnp.camera(Tir=pc.TIR, **CAM)
    pa, pb = pnp.default_params(**sa["params"]), pnp.default_params(**sb["params"])
    a0 = a.solve(pa, cam, sa["from_xyz"], sa["to_xy"], sa["to_xyz"])
    b0 = b.solve(pb, cam, sb["from_xyz"], sb["to_xy"], None)
    st_a = a.download()                                     # the state of a after b has run
    rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
    a1 = a.solve(pa, cam, sa["from_xyz"], sa["to_xy"], sa["to_xyz"])
    b1 = b.solve(pb, cam, sb["from_xyz"], sb["to_xy"], None)
    assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
    assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()
    want_a = host.solve(pa, cam, sa["from_xyz"], sa["to_xy"], sa["to_xyz"])
    st_h = host.download()
    want_b = host.solve(pb, cam, sb["from_xyz"], sb["to_xy"], None)
    for got, got2, want in ((a0, a1, want_a), (b0, b1, want_b)):
        assert all(got[k].tobytes() == want[k].tobytes() == got2[k].tobytes() for k in want)
    assert all(np.asarray(st_a[k]).tobytes() == np.asarray(st_h[k]).tobytes() for k in st_h)
    assert len(a0["inliers"]) > 50 and len(b0["inliers"]) > 30
    for o in (a, b, host):
        o.close()
