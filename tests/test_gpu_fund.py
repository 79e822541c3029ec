"""The fundamental-matrix cull on the GPU (include/visfs_fund.h): the device path against the host twin byte for byte — every
hypothesis's sample, model count, models and inlier counts, the winner, the two transforms, and status_out, mask_out, F_out, n_inliers
and applied — at the wavefront and workgroup edges of both kernels, with NaN rows, cleared status entries, status_out aliasing
status_in, on the degenerate inputs, and with two objects, a PnP solve and a BA solve on one handle."""
import numpy as np
import pytest

import fund_cases as fc
import pnp_cases as pc
from visfs_amd import abi, backend, fund, pnp, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


@pytest.fixture(scope="module")
def pair(solver):
    dev, host = fund.Fund(fund.MAX_POINTS, solver=solver), fund.Fund(fund.MAX_POINTS)
    yield dev, host
    dev.close(); host.close()


def _same_call(dev, host, prm, from_xy, to_xy, status, in_place=False):
    ra, a = dev.cull_status(fund.default_params(**prm), from_xy, to_xy, status, in_place)
    rb, b = host.cull_status(fund.default_params(**prm), from_xy, to_xy, status, in_place)
    assert ra == rb == abi.OK
    sa, sb = dev.download(), host.download()
    for key in sorted(sb):
        assert np.asarray(sa[key]).tobytes() == np.asarray(sb[key]).tobytes(), key
    for key in sorted(b):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    assert np.isfinite(a["F"]).all() and np.isfinite(sa["models"]).all()
    return a, sa


@pytest.mark.parametrize("rows", fc.DEVICE_ROWS)
def test_rows_at_the_edges_equal_the_host_twin(pair, rows):
    s = fc.scene(rows, 0.3 if rows >= 20 else 0.0, 50 + rows)
    out, st = _same_call(*pair, fc.params_dict(iterations=64), s["from_xy"], s["to_xy"], s["status"])
    assert st["m"] == rows and out["applied"] == 1 and st["winner"][0] >= 0
    assert out["n_inliers"] == int(out["mask"].sum()) >= 7
    assert out["status"].tolist() == (out["mask"] & s["status"]).tolist()


@pytest.mark.parametrize("iterations", fc.DEVICE_ITERATIONS)
def test_hypothesis_counts_at_the_edges_equal_the_host_twin(pair, iterations):
    s = fc.scene(150, 0.3, 70)
    out, st = _same_call(*pair, fc.params_dict(iterations=iterations), s["from_xy"], s["to_xy"], s["status"])
    assert len(st["n_models"]) == iterations and st["n_models"].min() >= 1
    h, k = st["winner"]
    flat = st["counts"].reshape(-1)
    assert 3 * h + k == int(np.argmax(flat)) and flat.max() == out["n_inliers"]      # ties to the lowest h, then the lowest model


def test_committed_cases_equal_the_host_twin(pair):
    shapes = set()
    for name in sorted(fc.CASES):
        s = fc.case(name)
        out, st = _same_call(*pair, s["params"], s["from_xy"], s["to_xy"], s["status"])
        shapes.update(st["n_models"].tolist())
        assert out["n_inliers"] >= 7
    assert {1, 3} <= shapes                                  # one and three real roots ran on the device


def test_nan_rows_status_zeros_aliasing_and_other_seeds_equal_the_host_twin(pair):
    s = fc.scene(80, 0.2, 41, nan_rows=9)
    assert (s["status"] == 0).any()
    out, st = _same_call(*pair, fc.params_dict(iterations=64), s["from_xy"], s["to_xy"], s["status"])
    bad = ~(np.isfinite(s["from_xy"]).all(axis=1) & np.isfinite(s["to_xy"]).all(axis=1))
    assert st["m"] == 71 and not out["mask"][bad].any() and out["n_inliers"] >= 40
    alias, _ = _same_call(*pair, fc.params_dict(iterations=64), s["from_xy"], s["to_xy"], s["status"], in_place=True)
    assert alias["status"].tolist() == out["status"].tolist() and alias["mask"].tolist() == out["mask"].tolist()
    zeros, _ = _same_call(*pair, fc.params_dict(iterations=64), s["from_xy"], s["to_xy"], np.zeros_like(s["status"]))
    assert not zeros["status"].any() and zeros["mask"].tolist() == out["mask"].tolist()
    for seed in (1, 2 ** 63 + 5):
        _same_call(*pair, fc.params_dict(iterations=64, seed=seed, pixel_error=0.5), s["from_xy"], s["to_xy"], s["status"])


@pytest.mark.parametrize("name", sorted(fc.degenerate_inputs()))
def test_degenerate_inputs_equal_the_host_twin(pair, name):
    prm, from_xy, to_xy, status = fc.degenerate_inputs()[name]
    out, st = _same_call(*pair, prm, from_xy, to_xy, status)
    fc.check_degenerate(name, prm, from_xy, to_xy, status, out, st)


def test_argument_checks_on_the_device(solver, pair):
    dev, _ = pair
    s = fc.scene(20, 0.0, 3)
    args = (s["from_xy"], s["to_xy"], s["status"])
    assert dev.cull_status(fund.default_params(iterations=0), *args)[0] == abi.ERR_BAD_ARGUMENT
    assert dev.cull_status(fund.default_params(iterations=4097), *args)[0] == abi.ERR_UNSUPPORTED
    assert dev.cull_status(fund.default_params(pixel_error=float("nan")), *args)[0] == abi.ERR_BAD_ARGUMENT
    small = fund.Fund(16, solver=solver)
    assert small.cull_status(fund.default_params(), *args)[0] == abi.ERR_BAD_ARGUMENT
    small.close()
    with pytest.raises(backend.BackendError):
        fund.Fund(4097, solver=solver)


def test_two_objects_a_pnp_solve_and_a_ba_solve_on_one_handle(solver):
    wnd = synth.make_window("C1")
    cam = pnp.camera(Tir=pc.TIR, **dict(zip(("fx", "fy", "cx", "cy"), pc.K)))
    sp = pc.case("m64_out30")
    pp = pnp.default_params(**sp["params"])
    pose = pnp.Pnp(64, solver=solver)
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))                   # before any cull exists on the handle
    p0 = pose.solve(pp, cam, sp["from_xyz"], sp["to_xy"], sp["to_xyz"])
    assert rc0 == abi.OK
    a, b, host = fund.Fund(400, solver=solver), fund.Fund(64, solver=solver), fund.Fund(400)
    sa, sb = fc.case("m300_out30_b"), fc.case("m64_out25")
    pa, pb = fund.default_params(**sa["params"]), fund.default_params(**sb["params"])
    a0 = a.cull(pa, sa["from_xy"], sa["to_xy"], sa["status"])
    b0 = b.cull(pb, sb["from_xy"], sb["to_xy"], sb["status"])
    st_a = a.download()                                      # the state of a after b has run
    rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
    p1 = pose.solve(pp, cam, sp["from_xyz"], sp["to_xy"], sp["to_xyz"])
    a1 = a.cull(pa, sa["from_xy"], sa["to_xy"], sa["status"])
    b1 = b.cull(pb, sb["from_xy"], sb["to_xy"], sb["status"])
    assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
    assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()
    assert all(p0[k].tobytes() == p1[k].tobytes() for k in p0) and len(p0["inliers"]) > 30
    want_a = host.cull(pa, sa["from_xy"], sa["to_xy"], sa["status"])
    st_h = host.download()
    want_b = host.cull(pb, sb["from_xy"], sb["to_xy"], sb["status"])
    for got, got2, want in ((a0, a1, want_a), (b0, b1, want_b)):
        assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() == np.asarray(got2[k]).tobytes() for k in want)
    assert all(np.asarray(st_a[k]).tobytes() == np.asarray(st_h[k]).tobytes() for k in st_h)
    assert a0["n_inliers"] > 150 and b0["n_inliers"] > 30
    for o in (a, b, host, pose):
        o.close()
