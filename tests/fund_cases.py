"""Scenes of the fundamental-matrix tests and the conditions they must meet on the checker's output alone (tests/fund_oracle.py),
before the library is compared with it.

A scene: the bench camera (fx = fy = 435.2 at 752 x 480), random points at 1.5 .. 9 m seen from two poses a frame apart (up to 0.06 rad
about each axis, up to 0.3 m), 0.3 px of pixel noise in the second view, and a share of rows displaced by 15 .. 80 px.
"""
import math

import numpy as np

import fund_oracle as fo

WIDTH, HEIGHT = 752, 480
K = (435.2, 435.2, 367.4, 252.2)

# The bound of tests/test_fund_host.py: 100 x the largest host-twin-to-checker difference of a conditioned model F^ (unit norm) over
# CASES (profiles/fund_parity.log).
MEASURED_MODEL = 3.6e-13
MODEL_BOUND = 100 * MEASURED_MODEL

# Conditions (a) .. (e), see check_conditions.
ERROR_MARGIN_PX = 1e-5         # (a)
KEY_SEPARATION = 1e-6          # (b)
SIGN_GAP = 1e-6                # (b) the two largest magnitudes of F^: its sign is decided by the larger
REAL_IMAG_MAX, COMPLEX_IMAG_MIN = 1e-9, 1e-5      # (c) relative imaginary parts: real below, complex above
LIMIT_FACTOR = 1e3             # (c) rank and leading-coefficient ratios this factor above their limits (or as far below)
MAX_DISPLACED_KEPT = 0.05      # (e) share of the displaced rows the mask may keep, scenes with >= 20 rows and <= 30 % displaced
MIN_TRUE_KEPT = 0.80           # (e) share of the true rows it must keep

# name: (rows, displaced fraction, hypotheses, scene seed)
CASES = {
    "m300_out30": (300, 0.30, 256, 1),
    "m300_out30_b": (300, 0.30, 50, 3),
    "m300_clean": (300, 0.0, 64, 3),
    "m64_out25": (64, 0.25, 128, 5),
    "m20_out20": (20, 0.20, 64, 4),
    "m8": (8, 0.0, 16, 6),
    "m7": (7, 0.0, 1, 7),
}

# Shapes of the device test (tests/test_gpu_fund.py): wavefront and workgroup edges of both kernels.
DEVICE_ROWS = (7, 8, 9, 63, 64, 65, 255, 256, 257, 300, 1100)
DEVICE_ITERATIONS = (1, 3, 4, 5, 64, 65, 256)


def _rot(w):
    t = float(np.linalg.norm(w))
    if t == 0.0:
        return np.eye(3)
    k = w / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * Kx + (1 - math.cos(t)) * (Kx @ Kx)


def scene(rows, displaced, seed, nan_rows=0):
    """dict: from_xy [n][2], to_xy [n][2] float32, status [n] uint8 (one in ten cleared), displaced mask [n]."""
    rng = np.random.default_rng(5000 + seed)
    R, t = _rot(rng.uniform(-0.06, 0.06, 3)), rng.uniform(-0.3, 0.3, 3)
    uv = np.stack([rng.uniform(8, WIDTH - 8, rows), rng.uniform(8, HEIGHT - 8, rows)], axis=1)
    z = rng.uniform(1.5, 9.0, rows)
    P = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], axis=1)
    Q = P @ R.T + t
    to = np.stack([K[0] * Q[:, 0] / Q[:, 2] + K[2], K[1] * Q[:, 1] / Q[:, 2] + K[3]], axis=1) + rng.normal(0.0, 0.3, (rows, 2))
    out = np.zeros(rows, dtype=bool)
    out[rng.permutation(rows)[:int(round(displaced * rows))]] = True
    ang, rad = rng.uniform(0, 2 * math.pi, rows), rng.uniform(15.0, 80.0, rows)
    to[out] += np.stack([np.cos(ang), np.sin(ang)], axis=1)[out] * rad[out, None]
    status = np.ones(rows, dtype=np.uint8)
    status[rng.permutation(rows)[:rows // 10]] = 0
    from_xy, to_xy = uv.astype(np.float32), to.astype(np.float32)
    if nan_rows:
        idx = rng.permutation(rows)[:nan_rows]
        from_xy[idx[::2], 0] = np.nan
        to_xy[idx[1::2], 1] = np.inf
    return {"from_xy": from_xy, "to_xy": to_xy, "status": status, "displaced": out}


def params_dict(**kw):
    p = {"pixel_error": 1.0, "iterations": 1000, "seed": 0}
    p.update(kw)
    return p


def case(name):
    rows, displaced, iterations, seed = CASES[name]
    s = scene(rows, displaced, seed)
    s["params"] = params_dict(iterations=iterations)
    s["displaced_share"] = displaced
    return s


_REFERENCE = {}


def reference(name):
    """The checker's result of a case, computed once and shared (read-only) by the tests; the conditions are asserted here."""
    if name not in _REFERENCE:
        s = case(name)
        ref = fo.cull(s["params"], s["from_xy"], s["to_xy"], s["status"])
        check_conditions(ref, s)
        _REFERENCE[name] = (s, ref)
    return _REFERENCE[name]


def check_conditions(ref, s):
    """Conditions (a), (b), (c) and (e) on one checker result; (d) is ref['ties'] > 1 in some case."""
    assert ref["margin"] > ERROR_MARGIN_PX, f"(a) an error lies {ref['margin']:.2e} px from the threshold"
    for h, d in enumerate(ref["diags"]):
        r = d["rank_ratio"]
        assert r > LIMIT_FACTOR * fo.RANK_LIMIT or r < fo.RANK_LIMIT / LIMIT_FACTOR, f"(c) hypothesis {h}: rank ratio {r:.2e} at its limit"
        if r < fo.RANK_LIMIT:
            continue
        r = d["lead_ratio"]
        assert r > LIMIT_FACTOR * fo.LEAD_LIMIT or r < fo.LEAD_LIMIT / LIMIT_FACTOR, f"(c) hypothesis {h}: leading coefficient {r:.2e} at its limit"
        if r < fo.LEAD_LIMIT:
            continue
        assert d["max_real_imag"] < REAL_IMAG_MAX and d["min_complex_imag"] > COMPLEX_IMAG_MIN, \
            f"(c) hypothesis {h}: a root is neither clearly real nor clearly complex ({d['max_real_imag']:.2e}, {d['min_complex_imag']:.2e})"
        assert d["key_sep"] > KEY_SEPARATION, f"(b) hypothesis {h}: two models {d['key_sep']:.2e} apart in F^[2][2]"
        assert d["sign_gap"] > SIGN_GAP, f"(b) hypothesis {h}: the two largest entries of a model {d['sign_gap']:.2e} apart"
    if ref["m"] >= 20 and s["displaced_share"] <= 0.30:
        keep = ref["keep"]
        bad, good = s["displaced"][keep], ~s["displaced"][keep]
        mask = ref["mask"][keep].astype(bool)
        assert mask[bad].sum() <= MAX_DISPLACED_KEPT * max(1, bad.sum()), f"(e) the mask keeps {mask[bad].sum()} of {bad.sum()} displaced rows"
        assert mask[good].sum() >= MIN_TRUE_KEPT * good.sum(), f"(e) the mask keeps {mask[good].sum()} of {good.sum()} true rows"


# ---- degenerate inputs (both test files): each returns VISFS_BA_OK, finite outputs and no NaN ------------------------------------
def degenerate_inputs():
    """name -> (params dict, from_xy, to_xy, status)."""
    out = {}
    s = scene(40, 0.0, 31)
    ones = np.ones(40, dtype=np.uint8)
    out["identical"] = (params_dict(iterations=32), np.tile(s["from_xy"][:1], (40, 1)), np.tile(s["to_xy"][:1], (40, 1)), ones)
    out["to_equals_from"] = (params_dict(iterations=32), s["from_xy"], s["from_xy"].copy(), ones)
    t = np.arange(40, dtype=np.float32)
    line1 = np.stack([20.0 + 16.0 * t, 30.0 + 8.0 * t], axis=1).astype(np.float32)
    line2 = np.stack([25.0 + 16.0 * t, 41.0 + 8.0 * t], axis=1).astype(np.float32)
    out["one_line"] = (params_dict(iterations=32), line1, line2, ones)
    for m in (0, 6, 7, 8):
        q = scene(max(m, 1), 0.0, 40 + m)
        out[f"m{m}"] = (params_dict(iterations=8), q["from_xy"][:m], q["to_xy"][:m], q["status"][:m])
    q = scene(30, 0.0, 50, nan_rows=24)
    out["nan_rows_leave_six"] = (params_dict(iterations=8), q["from_xy"], q["to_xy"], q["status"])
    q = scene(30, 0.0, 51, nan_rows=8)
    out["nan_rows"] = (params_dict(iterations=32), q["from_xy"], q["to_xy"], q["status"])
    q = scene(60, 0.2, 52)
    out["pixel_error_zero"] = (params_dict(iterations=32, pixel_error=0.0), q["from_xy"], q["to_xy"], q["status"])
    out["pixel_error_negative"] = (params_dict(iterations=32, pixel_error=-2.0), q["from_xy"], q["to_xy"], q["status"])
    out["no_winner"] = (params_dict(iterations=32, pixel_error=1e-20), q["from_xy"], q["to_xy"], q["status"])
    return out


def check_degenerate(name, prm, from_xy, to_xy, status, out, st):
    """What a degenerate input must give, on the library's output (out of cull_status, st of download) alone."""
    n = len(from_xy)
    set_in = (np.asarray(status) != 0).astype(np.uint8)
    for key in ("F",):
        assert np.isfinite(out[key]).all(), key
    for key in ("models", "T1", "T2"):
        assert np.isfinite(st[key]).all(), key
    assert len(out["mask"]) == len(out["status"]) == n and set(out["mask"].tolist()) <= {0, 1} and set(out["status"].tolist()) <= {0, 1}
    assert out["n_inliers"] == int(out["mask"].sum())
    if out["applied"]:
        assert out["status"].tolist() == (out["mask"] & set_in).tolist()
    else:
        assert out["status"].tolist() == set_in.tolist() and not out["mask"].any() and (out["F"] == 0).all()
        assert len(st["n_models"]) == 0 and st["winner"] == (-1, -1) and (st["T1"] == 0).all()
    if name in ("identical", "to_equals_from", "one_line"):             # A has rank below 7 for every sample
        assert out["applied"] == 1 and not st["n_models"].any() and not st["counts"].any() and st["winner"] == (-1, -1)
        assert not out["mask"].any() and (out["F"] == 0).all() and (st["models"] == 0).all()
    if name in ("m0", "m6", "nan_rows_leave_six"):
        assert out["applied"] == 0 and st["m"] == {"m0": 0, "m6": 6, "nan_rows_leave_six": 6}[name]
    if name == "m7":
        assert out["applied"] == 1 and out["mask"].all() and out["n_inliers"] == 7 and len(st["n_models"]) == 1
        assert st["samples"].tolist() == [list(range(7))] and (out["F"] != 0).any() == bool(st["n_models"][0])
    if name == "m8":
        assert out["applied"] == 1 and len(st["n_models"]) == prm["iterations"] and sorted(st["samples"][0].tolist()) != list(range(8))
    if name == "nan_rows":
        assert out["applied"] == 1 and st["m"] == 22
    if name == "no_winner":
        assert out["applied"] == 1 and st["n_models"].any() and st["counts"].max() < 7 and st["winner"] == (-1, -1)
        assert not out["mask"].any() and not out["status"].any() and (out["F"] == 0).all()
