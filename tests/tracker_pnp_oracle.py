"""The checker of tracker_oracle.py (or, with the cull on, of tracker_cull_oracle.py) with estimateMotion3DTo2D put behind each frame
as the staged chain runs it today: the staged pnp.Pnp.solve on that frame's covisible rows, with to_xyz matched by id from the
frame's words (None when the frame has no words, a NaN triple for a row whose id is not among them), which is what
visfs_amd/host/MotionEstimator.h builds from its maps.  The intermediates come from pnp.Pnp.download().  It shares no code with the
pose guess of the resident call: rows, search and refinement are those of visfs_pnp_solve, which has its own NumPy checker
(pnp_oracle.py)."""
import numpy as np

import tracker_cull_oracle as tco
import tracker_oracle as to
from visfs_amd import pnp

POSE_ARRAYS = ("T", "cov", "matches", "inliers")
HOOK_ARRAYS = ("samples", "valid", "models", "counts", "refit_tq", "pass_tq", "pass_threshold", "pass_count", "pass_inliers")


def not_ran():
    """What tracker_pnp.last reports when the pose guess did not run."""
    return dict(ran=0, T=np.zeros((4, 4)), cov=np.eye(6), matches=np.zeros(0, dtype=np.int32), inliers=np.zeros(0, dtype=np.int32))


def inactive():
    """What tracker_pnp.download reports when the pose guess did not run."""
    return dict(m=0, winner=-1, samples=np.zeros((0, 4), dtype=np.int32), valid=np.zeros(0, dtype=np.int32), models=np.zeros((0, 3, 4)),
                counts=np.zeros(0, dtype=np.int32), refit_tq=np.zeros(7), pass_tq=np.zeros((0, 7)),
                pass_threshold=np.zeros(0, dtype=np.float32), pass_count=np.zeros(0, dtype=np.int32),
                pass_inliers=np.zeros((0, 0), dtype=np.int32))


def pnp_camera(cam):
    """The pnp.Camera of a flow.Camera: its float intrinsics as doubles, its Tir."""
    return pnp.camera(fx=float(cam.fx), fy=float(cam.fy), cx=float(cam.cx), cy=float(cam.cy), Tir=list(cam.Tir))


def to_xyz_by_id(out):
    if len(out["word_id"]) == 0:
        return None
    where = {int(i): k for k, i in enumerate(out["word_id"])}
    rows = np.full((len(out["covisible_id"]), 3), np.nan, dtype=np.float32)
    for r, i in enumerate(out["covisible_id"]):
        k = where.get(int(i))
        if k is not None:
            rows[r] = out["word_xyz"][k]
    return rows


class PnpChecker:
    """base: a tracker_oracle.Checker or a tracker_cull_oracle.CullChecker.  process() gives the base's (result, intermediates) with
    result["pose"] (as tracker_pnp.last) and intermediates["pnp"] (as tracker_pnp.download) added."""

    def __init__(self, base, cam, params, solver=None):
        self.base, self.params, self.cam = base, params, pnp_camera(cam)
        self.pnp = pnp.Pnp(base.max_features, solver=solver)

    def close(self):
        self.pnp.close()
        self.base.close()

    def process(self, left, right, delta_guess=None, outliers=()):
        out, inter = self.base.process(left, right, delta_guess, outliers)
        if inter is None:
            out["pose"] = not_ran()
            return out, inter
        txyz = to_xyz_by_id(out)
        pose = self.pnp.solve(self.params, self.cam, out["covisible_from_xyz"], out["covisible_to_xy"], txyz)
        pose["ran"] = 1
        out["pose"] = pose
        inter["pnp"] = self.pnp.download()
        inter["pnp"]["rows_without_word"] = 0 if txyz is None else int(np.isnan(txyz).any(axis=1).sum())
        inter["pnp"]["to_xyz_is_null"] = txyz is None
        return out, inter


def assert_same_pose(got, want, what=""):
    assert got["ran"] == want["ran"], (what, "ran", got["ran"], want["ran"])
    for key in POSE_ARRAYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, key, a, b)


def assert_same_hook(got, want, what=""):
    for key in ("m", "winner"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in HOOK_ARRAYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, key)


def base_checker(scn, cam, solver=None):
    if scn.get("cull") is not None:
        return tco.CullChecker(scn["width"], scn["height"], cam, scn["cull"], solver=solver, **scn["trk"], **scn["flow"])
    return to.Checker(scn["width"], scn["height"], cam, solver=solver, **scn["trk"], **scn["flow"])
