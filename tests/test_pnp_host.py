"""The host twin of the PnP-RANSAC pose guess (include/visfs_pnp.h) against the NumPy checker (tests/pnp_oracle.py), on the CPU.
Samples and validity flags exactly; the hypotheses pixel by pixel; counts, winner and every inlier list exactly given the library's
hypotheses; thresholds, pose and covariance within MODEL_BOUND.  Every case first meets the conditions of tests/pnp_cases.py on the
checker's output alone."""
import numpy as np
import pytest

import pnp_cases as pc
import pnp_oracle as po
from visfs_amd import abi, pnp


@pytest.fixture(scope="module")
def twin():
    t = pnp.Pnp(pnp.MAX_POINTS)
    yield t
    t.close()


def _solve(twin, s, **kw):
    prm = dict(s["params"]); prm.update(kw)
    to = s["to_xyz"] if s.get("with_to_xyz") else None
    out = twin.solve(pnp.default_params(**prm), pnp.camera(*pc.K, Tir=pc.TIR), s["from_xyz"], s["to_xy"], to)
    return out, twin.download()


def test_at_least_one_case_decides_by_the_tie_rule():
    assert any(pc.reference(name)[1]["ties"] > 1 for name in pc.CASES)          # condition (d)
    assert any(False in pc.reference(name)[1]["valid"] for name in pc.CASES)    # the invalid path is exercised
    assert any(len(pc.reference(name)[1]["after"]["passes"]) > 1 for name in pc.CASES)


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_host_twin_equals_the_checker(twin, name):
    s, ref = pc.reference(name)
    out, st = _solve(twin, s)
    keep = ref["matches"]
    X, uv = s["from_xyz"][keep].astype(np.float64), s["to_xy"][keep].astype(np.float64)
    assert out["matches"].tolist() == keep.tolist()
    assert st["samples"].tolist() == ref["samples"]
    assert st["valid"].astype(bool).tolist() == ref["valid"]
    dh, dfar, dfar_px = pc.hypothesis_pixel_difference(st["models"], ref["models"], ref["valid"], X)
    # given the library's hypotheses: counts, winner, then every list
    counts, winner, margin = po.count_models(st["models"], st["valid"], pc.K, X, uv, np.float32(s["params"]["reproj_error"]))
    assert margin > 1e-4
    assert counts == st["counts"].tolist() and winner == st["winner"] == ref["winner"]
    W = st["models"][winner]
    to_kept = s["to_xyz"][keep] if s["with_to_xyz"] else None
    aft = po.after_winner(W[:, :3], W[:, 3], pc.K, pc.TIR, s["from_xyz"][keep], s["to_xy"][keep], to_kept, s["params"])
    assert aft["margin"] > 1e-4
    assert len(st["pass_count"]) == len(aft["passes"])
    dm = max(float(np.abs(_rt(st["refit_tq"])[0] - aft["refit"][0]).max()), float(np.abs(_rt(st["refit_tq"])[1] - aft["refit"][1]).max()))
    for k, (R, t, thr, _, lst) in enumerate(aft["passes"]):
        assert st["pass_inliers"][k][:st["pass_count"][k]].tolist() == lst, k
        dm = max(dm, abs(float(st["pass_threshold"][k]) - float(thr)))
        q = st["pass_tq"][k]
        dm = max(dm, float(np.abs(_rt(q)[0] - R).max()), float(np.abs(_rt(q)[1] - t).max()))
    assert out["inliers"].tolist() == keep[aft["inliers"]].tolist() == ref["inliers"].tolist()
    dm = max(dm, float(np.abs(out["T"] - aft["T"]).max()), float(np.abs(out["cov"] - aft["cov"]).max()))
    print(f"pnp parity {name}: hypotheses {dh:.3e} px on rows within an image width (bound {pc.HYPOTHESIS_PX_BOUND:.1e}), {dfar:.3e} relative "
          f"on rows thrown farther out (bound {pc.HYPOTHESIS_FAR_BOUND:.1e}; {dfar_px:.3e} px unscaled); refit, passes, pose, thresholds, covariance "
          f"{dm:.3e} (bound {pc.MODEL_BOUND:.1e}); {len(aft['passes'])} passes, {len(out['inliers'])} inliers, "
          f"{ref['ties']} hypotheses share the winning count, {ref['valid'].count(False)} invalid samples")
    assert dh <= pc.HYPOTHESIS_PX_BOUND
    assert dfar <= pc.HYPOTHESIS_FAR_BOUND
    assert dm <= pc.MODEL_BOUND
    rot, dist = pc.pose_error(out["T"], s["truth"])
    assert rot < 0.01 and dist < 0.05


def _rt(tq):
    x, y, z, w = tq[3:]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(tq[:3])


def test_nan_rows_are_dropped_and_row_numbers_are_the_callers(twin):
    s = pc.scene(80, 0.2, 41, nan_rows=9)
    s["params"] = pc.params_dict()
    s["with_to_xyz"] = True
    out, st = _solve(twin, s)
    ref = po.solve(s["params"], pc.K, pc.TIR, s["from_xyz"], s["to_xy"], s["to_xyz"])
    assert st["m"] == 71 and out["matches"].tolist() == ref["matches"].tolist()
    assert st["samples"].tolist() == ref["samples"]
    assert out["inliers"].tolist() == ref["inliers"].tolist() and len(out["inliers"]) >= 12
    assert np.isfinite(s["from_xyz"][out["inliers"]]).all()
    rot, dist = pc.pose_error(out["T"], s["truth"])
    assert rot < 0.01 and dist < 0.05


def test_a_call_is_a_pure_function_of_its_arguments(twin):
    s, _ = pc.reference("m64_out30")
    a, sa = _solve(twin, s)
    _solve(twin, pc.reference("m300_out40")[0])
    b, sb = _solve(twin, s)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert all(np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes() for k in sa)
    c, sc = _solve(twin, s, seed=7)
    assert sc["samples"].tolist() != sa["samples"].tolist()
    assert sc["samples"].tolist() == [po.sample(7, h, sc["m"]) for h in range(50)]


@pytest.mark.parametrize("name", sorted(pc.degenerate_inputs()))
def test_degenerate_inputs_give_the_zero_transform(twin, name):
    prm, from_xyz, to_xy = pc.degenerate_inputs()[name]
    rc, out = twin.solve_status(pnp.default_params(**prm), pnp.camera(*pc.K, Tir=pc.TIR), from_xyz, to_xy, None)
    assert rc == abi.OK
    st = twin.download()
    assert (out["T"] == 0).all() and len(out["inliers"]) == 0 and (out["cov"] == np.eye(6)).all()
    assert len(out["matches"]) == len(from_xyz)
    for key in ("models", "refit_tq", "pass_tq", "pass_threshold"):
        assert np.isfinite(st[key]).all(), key
    ref = po.solve(prm, pc.K, pc.TIR, from_xyz, to_xy, None)
    assert (ref["T"] == 0).all() and len(ref["inliers"]) == 0
    if name in ("collinear", "identical"):
        assert not st["valid"].any() and st["winner"] == -1
    if name == "three_rows":
        assert len(st["valid"]) == 0
    if name == "no_refinement":
        assert st["winner"] >= 0 and st["counts"][st["winner"]] >= 12 and len(st["pass_count"]) == 0
    if name == "weak_winner":
        assert st["winner"] >= 0 and 0 < st["counts"][st["winner"]] < 12 and st["counts"].tolist() == ref["counts"]


def test_argument_checks(twin):
    s = pc.scene(20, 0.0, 3)
    cam = pnp.camera(*pc.K, Tir=pc.TIR)

    def status(p=None, c=None, n=20, **kw):
        return twin.solve_status(p or pnp.default_params(**kw), c or cam, s["from_xyz"][:n], s["to_xy"][:n])[0]
    assert status() == abi.OK
    assert status(iterations=0) == abi.ERR_BAD_ARGUMENT
    assert status(iterations=4097) == abi.ERR_UNSUPPORTED
    assert status(refine_iterations=-1) == abi.ERR_BAD_ARGUMENT
    assert status(refine_iterations=33) == abi.ERR_UNSUPPORTED
    assert status(reproj_error=float("nan")) == abi.ERR_BAD_ARGUMENT
    assert status(refine_sigma=float("inf")) == abi.ERR_BAD_ARGUMENT
    assert status(c=pnp.camera(fx=float("nan"))) == abi.ERR_BAD_ARGUMENT
    small = pnp.Pnp(16)
    assert small.solve_status(pnp.default_params(), cam, s["from_xyz"], s["to_xy"])[0] == abi.ERR_BAD_ARGUMENT
    assert "capacity" in small.last_error()
    small.close()
    lib = pnp.load()
    import ctypes as C
    h = C.c_void_p()
    assert lib.visfs_pnp_create_host(4097, C.byref(h)) == abi.ERR_UNSUPPORTED
    assert lib.visfs_pnp_create_host(0, C.byref(h)) == abi.ERR_BAD_ARGUMENT
    fresh = pnp.Pnp(8)
    with pytest.raises(Exception):
        fresh.download()
    fresh.close()


def test_min_inliers_below_four_is_raised_to_four(twin):
    s, _ = pc.reference("m4")
    a, _ = _solve(twin, s, min_inliers=0)
    b, _ = _solve(twin, s, min_inliers=4)
    assert a["T"].tobytes() == b["T"].tobytes() and len(a["inliers"]) == 4
    three = {"from_xyz": s["from_xyz"][:3], "to_xy": s["to_xy"][:3], "params": s["params"]}
    out, _ = _solve(twin, three, min_inliers=0)
    assert (out["T"] == 0).all() and len(out["matches"]) == 3
