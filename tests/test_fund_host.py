"""The host twin of the fundamental-matrix cull (include/visfs_fund.h) against the NumPy checker (tests/fund_oracle.py), on the CPU.
Samples, validity, model counts, every inlier count, the winner, the mask and the ANDed status exactly; the conditioned models F^
within MODEL_BOUND.  Every case first meets the conditions of tests/fund_cases.py on the checker's output alone.

MODEL_BOUND is 100 x the largest twin-to-checker difference measured over the cases (3.6e-13, profiles/fund_parity.log): 3.6e-11 on
the entries of a unit-norm matrix.  On conditioned coordinates of size ~1 that moves an epipolar distance by ~1e-10 of the image
scale, some 1e-8 px: three decades below the 1e-5 px of condition (a), and the F^[2][2] of two models differ by 1e-6 (b), so a
difference within the bound can flip neither a count nor the order of two models."""
import ctypes as C

import numpy as np
import pytest

import fund_cases as fc
import fund_oracle as fo
from visfs_amd import abi, fund


@pytest.fixture(scope="module")
def twin():
    t = fund.Fund(fund.MAX_POINTS)
    yield t
    t.close()


def _cull(twin, s, **kw):
    prm = dict(s["params"]); prm.update(kw)
    out = twin.cull(fund.default_params(**prm), s["from_xy"], s["to_xy"], s["status"])
    return out, twin.download()


def test_abi_and_defaults():
    assert fund.load().visfs_fund_abi_version() == fund.ABI_VERSION == 1
    p = fund.default_params()
    assert (p.pixel_error, p.iterations, p.seed) == (1.0, 1000, 0)


def test_some_case_decides_by_the_tie_rule():
    assert any(fc.reference(name)[1]["ties"] > 1 for name in fc.CASES if fc.CASES[name][0] >= 8)        # condition (d)
    assert any(w[1] > 0 for w in (fc.reference(name)[1]["winner"] for name in fc.CASES))               # a winner that is not model 0
    counts = {len(ms) for name in fc.CASES for ms in fc.reference(name)[1]["models"]}
    assert {1, 3} <= counts                                                                            # one and three real roots


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_host_twin_equals_the_checker(twin, name):
    s, ref = fc.reference(name)
    out, st = _cull(twin, s)
    assert st["m"] == ref["m"] and out["applied"] == ref["applied"] == 1
    assert st["samples"].tolist() == ref["samples"]
    assert st["n_models"].tolist() == [len(ms) for ms in ref["models"]]
    d = 0.0
    for h, ms in enumerate(ref["models"]):
        for k, Fh in enumerate(ms):
            d = max(d, float(np.abs(st["models"][h][k] - Fh).max()))
        assert (st["models"][h][len(ms):] == 0).all()
    dT = max(float(np.abs(st["T1"] - ref["T1"]).max()), float(np.abs(st["T2"] - ref["T2"]).max()))
    assert st["counts"].tolist() == ref["counts"]
    assert st["winner"] == ref["winner"]
    assert out["mask"].tolist() == ref["mask"].tolist() and out["status"].tolist() == ref["status"].tolist()
    assert out["n_inliers"] == ref["n_inliers"] == int(out["mask"].sum())
    scale = float(np.abs(ref["F"]).max())
    dF = float(np.abs(out["F"] - ref["F"]).max()) / scale
    print(f"fund parity {name}: m {st['m']}, {len(ref['samples'])} hypotheses, models {np.bincount(st['n_models'], minlength=4).tolist()} by "
          f"count; F^ {d:.3e} (bound {fc.MODEL_BOUND:.1e}); T {dT:.3e}; F relative {dF:.3e}; winner {st['winner']} with {out['n_inliers']} "
          f"inliers, {ref['ties']} models share the winning count; nearest error {ref['margin']:.2e} px from the threshold")
    assert d <= fc.MODEL_BOUND and dF <= fc.MODEL_BOUND
    assert dT <= 1e-12 * max(1.0, float(np.abs(ref["T1"]).max()), float(np.abs(ref["T2"]).max()))     # two serial sums of the same terms


def test_every_row_enters_whatever_its_status(twin):
    s, ref = fc.reference("m64_out25")
    assert (s["status"] == 0).any()
    a, sa = _cull(twin, s)
    zeros = dict(s, status=np.zeros_like(s["status"]))
    b, sb = _cull(twin, zeros)
    assert sa["samples"].tolist() == sb["samples"].tolist() and a["mask"].tolist() == b["mask"].tolist() and a["F"].tobytes() == b["F"].tobytes()
    assert not b["status"].any() and a["status"].tolist() == (a["mask"] & s["status"]).tolist()
    twos = dict(s, status=(s["status"] * 2).astype(np.uint8))                      # nonzero is set
    assert _cull(twin, twos)[0]["status"].tolist() == a["status"].tolist()
    c = twin.cull(fund.default_params(**s["params"]), s["from_xy"], s["to_xy"], s["status"], in_place=True)       # status_out is status_in
    assert c["status"].tolist() == a["status"].tolist() and c["mask"].tolist() == a["mask"].tolist()


def test_nan_rows_are_never_sampled_and_their_mask_is_zero(twin):
    s = fc.scene(80, 0.2, 41, nan_rows=9)
    s["params"] = fc.params_dict(iterations=64)
    out, st = _cull(twin, s)
    ref = fo.cull(s["params"], s["from_xy"], s["to_xy"], s["status"])
    bad = ~(np.isfinite(s["from_xy"]).all(axis=1) & np.isfinite(s["to_xy"]).all(axis=1))
    assert bad.sum() == 9 and st["m"] == 71 and st["samples"].max() < 71
    assert st["samples"].tolist() == ref["samples"] and st["counts"].tolist() == ref["counts"] and st["winner"] == ref["winner"]
    assert out["mask"].tolist() == ref["mask"].tolist() and not out["mask"][bad].any() and not out["status"][bad].any()
    assert out["n_inliers"] >= 40 and np.isfinite(out["F"]).all()


def test_a_call_is_a_pure_function_of_its_arguments(twin):
    s, _ = fc.reference("m64_out25")
    a, sa = _cull(twin, s)
    _cull(twin, fc.reference("m300_out30_b")[0])
    b, sb = _cull(twin, s)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    assert all(np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes() for k in sa)
    c, sc = _cull(twin, s, seed=7)
    assert sc["samples"].tolist() != sa["samples"].tolist()
    assert sc["samples"].tolist() == [fo.sample(7, h, sc["m"]) for h in range(s["params"]["iterations"])]
    assert all(len(set(row)) == 7 for row in sc["samples"].tolist())


@pytest.mark.parametrize("name", sorted(fc.degenerate_inputs()))
def test_degenerate_inputs_are_ok_and_finite(twin, name):
    prm, from_xy, to_xy, status = fc.degenerate_inputs()[name]
    rc, out = twin.cull_status(fund.default_params(**prm), from_xy, to_xy, status)
    assert rc == abi.OK
    st = twin.download()
    fc.check_degenerate(name, prm, from_xy, to_xy, status, out, st)
    ref = fo.cull(prm, from_xy, to_xy, status)
    assert out["applied"] == ref["applied"] and st["m"] == ref["m"]
    if name in ("m0", "m6", "m7", "m8", "nan_rows", "nan_rows_leave_six", "pixel_error_zero", "pixel_error_negative"):
        assert out["mask"].tolist() == ref["mask"].tolist() and out["status"].tolist() == ref["status"].tolist()
        assert st["winner"] == ref["winner"] and st["counts"].tolist() == ref["counts"]


def test_argument_checks(twin):
    s = fc.scene(20, 0.0, 3)

    def status(n=20, **kw):
        return twin.cull_status(fund.default_params(**kw), s["from_xy"][:n], s["to_xy"][:n], s["status"][:n])[0]
    assert status() == abi.OK
    assert status(iterations=0) == abi.ERR_BAD_ARGUMENT
    assert status(iterations=4097) == abi.ERR_UNSUPPORTED
    assert status(iterations=4096, n=8) == abi.OK
    assert status(pixel_error=float("nan")) == abi.ERR_BAD_ARGUMENT
    assert status(pixel_error=float("inf")) == abi.ERR_BAD_ARGUMENT
    small = fund.Fund(16)
    assert small.cull_status(fund.default_params(), s["from_xy"], s["to_xy"], s["status"])[0] == abi.ERR_BAD_ARGUMENT
    assert "capacity" in small.last_error()
    small.close()
    lib = fund.load()
    h = C.c_void_p()
    assert lib.visfs_fund_create_host(4097, C.byref(h)) == abi.ERR_UNSUPPORTED
    assert lib.visfs_fund_create_host(0, C.byref(h)) == abi.ERR_BAD_ARGUMENT
    ni, ap = C.c_int32(), C.c_int32()
    assert lib.visfs_fund_cull(twin.h, None, 0, None, None, None, None, None, None, C.byref(ni), C.byref(ap)) == abi.ERR_BAD_ARGUMENT
    prm = fund.default_params()
    assert lib.visfs_fund_cull(twin.h, C.byref(prm), 5, None, None, None, None, None, None, C.byref(ni), C.byref(ap)) == abi.ERR_BAD_ARGUMENT
    assert lib.visfs_fund_cull(twin.h, C.byref(prm), -1, None, None, None, None, None, None, C.byref(ni), C.byref(ap)) == abi.ERR_BAD_ARGUMENT
    fresh = fund.Fund(8)
    with pytest.raises(Exception):
        fresh.download()
    fresh.close()
