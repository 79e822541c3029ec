"""Scenes of the PnP tests and the conditions they must meet on the checker's output alone (tests/pnp_oracle.py), before the library
is compared with it.

A scene: the bench camera (fx = fy = 435.2 at 752 x 480), words at 1.5 .. 9 m seen from the current pose, 0.3 px of pixel noise,
outliers displaced by 15 .. 80 px.  from_xyz is in the robot frame of the frame before, so the truth of T_out is the motion itself.
"""
import math

import numpy as np

import pnp_oracle as po

WIDTH, HEIGHT = 752, 480
K = (435.2, 435.2, 367.4, 252.2)
TIR = [0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0]

# The bounds of tests/test_pnp_host.py: 100 x the largest host-twin-to-checker difference over CASES (profiles/pnp_parity.log).
# A measured pose difference above 1e-8 or a hypothesis difference above 1e-6 px would mean one side is wrong.
MEASURED_HYPOTHESIS_PX = 2.0e-8           # absolute, rows a hypothesis projects within one image width of the origin
MEASURED_HYPOTHESIS_FAR = 1.68e-7          # relative to |pixel| / WIDTH, rows thrown farther out (hypothesis_pixel_difference)
MEASURED_MODEL = 1.46e-11
HYPOTHESIS_PX_BOUND = 100 * MEASURED_HYPOTHESIS_PX
HYPOTHESIS_FAR_BOUND = 100 * MEASURED_HYPOTHESIS_FAR
MODEL_BOUND = 100 * MEASURED_MODEL            # pose entries (rad, m), thresholds (px) and covariance entries

# name: (rows, outlier fraction, hypotheses, min_inliers, scene seed, with to_xyz)
CASES = {
    "m300_out40": (300, 0.40, 50, 12, 100, True),
    "m300_out40_b": (300, 0.40, 50, 12, 23, False),
    "m300_clean": (300, 0.0, 50, 12, 16, False),
    "m64_out30": (64, 0.30, 50, 12, 12, True),
    "m20_out25": (20, 0.25, 50, 8, 18, False),
    "m5": (5, 0.0, 50, 4, 10, True),
    "m4": (4, 0.0, 50, 4, 6, False),
}

# Shapes of the device test (tests/test_gpu_pnp.py): wavefront and workgroup edges of both kernels.
DEVICE_ROWS = (4, 5, 63, 64, 65, 300, 1100)
DEVICE_ITERATIONS = (1, 3, 50, 65, 256)


def motion(rng):
    """A frame-to-frame motion of the robot: up to ~0.1 rad and 0.3 m."""
    w = rng.uniform(-0.06, 0.06, 3)
    T = np.eye(4)
    T[:3, :3] = po.expm_so3(w)
    T[:3, 3] = rng.uniform(-0.3, 0.3, 3)
    return T


def scene(rows, outliers, seed, nan_rows=0):
    """dict: from_xyz [n][3], to_xy [n][2], to_xyz [n][3] float32, truth [4][4], outlier mask."""
    rng = np.random.default_rng(1000 + seed)
    T = motion(rng)
    Ti = np.eye(4); Ti[:3] = np.array(TIR).reshape(3, 4)
    uv = np.stack([rng.uniform(8, WIDTH - 8, rows), rng.uniform(8, HEIGHT - 8, rows)], axis=1)
    z = rng.uniform(1.5, 9.0, rows)
    pc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z, np.ones(rows)], axis=1)
    now = pc @ Ti.T                              # the words in the robot frame now
    before = now @ T.T                           # ... and in the robot frame of the frame before
    to_xy = uv + rng.normal(0.0, 0.3, (rows, 2))
    out = np.zeros(rows, dtype=bool)
    out[rng.permutation(rows)[:int(round(outliers * rows))]] = True
    ang = rng.uniform(0, 2 * math.pi, rows)
    rad = rng.uniform(15.0, 80.0, rows)
    to_xy[out] += np.stack([np.cos(ang), np.sin(ang)], axis=1)[out] * rad[out, None]
    from_xyz = before[:, :3].astype(np.float32)
    to_xyz = (now[:, :3] + rng.normal(0.0, 0.01, (rows, 3))).astype(np.float32)
    to_xyz[rng.permutation(rows)[:rows // 10]] = np.nan
    if nan_rows:
        from_xyz[rng.permutation(rows)[:nan_rows]] = np.nan
    return {"from_xyz": from_xyz, "to_xy": to_xy.astype(np.float32), "to_xyz": to_xyz, "truth": T, "outlier": out}


def params_dict(**kw):
    p = {"min_inliers": 12, "iterations": 50, "reproj_error": 2.0, "refine_iterations": 5, "refine_sigma": 3.0, "seed": 0}
    p.update(kw)
    return p


def case(name):
    rows, outliers, iterations, min_inliers, seed, with_to = CASES[name]
    s = scene(rows, outliers, seed)
    s["params"] = params_dict(iterations=iterations, min_inliers=min_inliers)
    s["with_to_xyz"] = with_to
    return s


_REFERENCE = {}


def reference(name):
    """The checker's result of a case, computed once and shared (read-only) by the tests; the conditions are asserted here."""
    if name not in _REFERENCE:
        s = case(name)
        ref = po.solve(s["params"], K, TIR, s["from_xyz"], s["to_xy"], s["to_xyz"] if s["with_to_xyz"] else None)
        ref["ties"] = check_conditions(ref, s["truth"])
        _REFERENCE[name] = (s, ref)
    return _REFERENCE[name]


def hypothesis_pixel_difference(models, ref_models, valid, X):
    """(absolute, relative, far_absolute): the largest difference between the pixels two sets of hypotheses give the rows X.  absolute: in pixels,
    over the rows the reference hypothesis projects within one image width of the origin (|u|, |v| <= WIDTH).  relative: over the
    other rows (a depth near zero throws them far outside the image), the difference divided by |pixel| / WIDTH: pixel coordinates grow
    as 1 / depth there, and so does the effect of the last bits of a model.  far_absolute: the same rows in plain pixels, for the log."""
    absolute = relative = far_absolute = 0.0
    for A, B, ok in zip(models, ref_models, valid):
        if ok:
            a, b = po.project(A[:, :3], A[:, 3], K, X), po.project(B[:, :3], B[:, 3], K, X)
            near = (np.abs(b) <= WIDTH).all(axis=1)
            d = np.abs(a - b)
            if near.any():
                absolute = max(absolute, float(d[near].max()))
            if (~near).any():
                relative = max(relative, float((d[~near] / np.maximum(1.0, np.abs(b[~near]) / WIDTH)).max()))
                far_absolute = max(far_absolute, float(d[~near].max()))
    return absolute, relative, far_absolute


def pose_error(T, truth):
    """(rotation angle in rad, translation distance in m) between two 4x4 transforms."""
    D = np.linalg.inv(truth) @ T
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    return math.acos(c), float(np.linalg.norm(D[:3, 3]))


def check_conditions(ref, truth):  # noqa: C901
    """Conditions (a), (b), (c) and (e) on one checker result; returns the number of hypotheses that share the winning count (d)."""
    assert ref["margin"] > 1e-4, f"(a) an error lies {ref['margin']:.2e} px from its threshold"
    for h, d in enumerate(ref["diags"]):
        assert not (0.25e-8 < d["sin2"] < 4e-8), f"(b) hypothesis {h}: collinearity at its boundary"
        if d["sin2"] < 1e-8:
            continue
        assert d["max_real_imag"] < 1e-9 and d["min_complex_imag"] > 1e-4, f"(b) hypothesis {h}: a root is neither clearly real nor clearly complex"
        assert d["root_sep"] > 2e-2, f"(b) hypothesis {h}: real roots {d['root_sep']:.2e} apart"
        assert d["depth_margin"] > 1e-2, f"(b) hypothesis {h}: a depth ratio {d['depth_margin']:.2e} from zero"
        assert d["fourth_gap"] > 0.01, f"(c) hypothesis {h}: best and second best {d['fourth_gap']:.2e} px apart on the fourth row"
    rot, dist = pose_error(ref["T"], truth)
    assert rot < 0.01 and dist < 0.05, f"(e) the checker's result is {rot:.4f} rad, {dist:.4f} m from the truth"
    return ref["ties"]


# ---- degenerate inputs (both test files): each returns VISFS_BA_OK, the stated result and no NaN -----------------------------------
def degenerate_inputs():
    """name -> (params dict, from_xyz, to_xy, expectation): 'zero' (zero transform, no inliers)."""
    rng = np.random.default_rng(77)
    out = {}
    t = np.linspace(1.0, 6.0, 40)
    line = np.stack([2.0 + t, 0.3 * t - 1.0, 0.1 * t], axis=1).astype(np.float32)
    Ti = np.array(TIR).reshape(3, 4)
    pc = (line.astype(np.float64) - Ti[:, 3]) @ Ti[:, :3]                 # into the camera frame (Tir is a rotation here)
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], axis=1).astype(np.float32)
    out["collinear"] = (params_dict(), line, uv)
    out["identical"] = (params_dict(), np.tile(line[:1], (40, 1)), np.tile(uv[:1], (40, 1)))
    s = scene(3, 0.0, 31)
    out["three_rows"] = (params_dict(min_inliers=4), s["from_xyz"], s["to_xy"])
    s = scene(64, 0.0, 32)
    out["no_refinement"] = (params_dict(refine_iterations=0), s["from_xyz"], s["to_xy"])
    s = scene(100, 0.70, 33)
    out["weak_winner"] = (params_dict(iterations=3, min_inliers=12), s["from_xyz"], s["to_xy"])
    del rng
    return out
