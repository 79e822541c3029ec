"""The checker of tracker_oracle.py with Tracker/CullByFundationMatrix put where the reference has it (Tracker.cpp:275-277, :83-96):
behind the staged flow.track comes the staged fund.Fund.cull on the same rows, and the status after the AND is what the checker's
own reduce sees.  It shares no code with the resident call: the rows, the conditioning and the search are those of the staged
visfs_fund_cull, which has its own NumPy checker (fund_oracle.py)."""
import numpy as np

import tracker_oracle as to
from visfs_amd import fund

CULL_KEYS = ("applied", "m", "n_hypotheses", "n_inliers", "winner")
CULL_ARRAYS = ("mask", "status", "F", "T1", "T2")


def inactive():
    """What tracker.Tracker.download_cull reports when the cull does not run."""
    z = np.zeros((3, 3))
    return dict(applied=0, m=0, n_hypotheses=0, n_inliers=0, winner=(-1, -1), mask=np.zeros(0, dtype=np.uint8),
                status=np.zeros(0, dtype=np.uint8), F=z, T1=z.copy(), T2=z.copy())


class CullChecker(to.Checker):
    """cull: dict(cull, pixel_error, iterations, seed).  As in the reference the cull runs only with flow_back off.  The fund object
    is a host-twin one, or a device one when a solver is given."""

    def __init__(self, width, height, cam, cull, solver=None, **kw):
        super().__init__(width, height, cam, solver=solver, **kw)
        self.cull_params = fund.default_params(pixel_error=cull["pixel_error"], iterations=cull["iterations"], seed=cull["seed"])
        self.active = bool(cull["cull"]) and not self.prm.flow_back
        self.fund = fund.Fund(self.max_features, solver=solver)
        self._staged_track = self.flow.track
        self.flow.track = self._track_and_cull             # the one call of process() that tracks frame to frame
        self._last = None

    def close(self):
        self.fund.close()
        super().close()

    def _track_and_cull(self, from_xy, guess_xy=None):
        to_xy, status, err = self._staged_track(from_xy, guess_xy)
        if not self.active:
            return to_xy, status, err
        out = self.fund.cull(self.cull_params, from_xy, to_xy, status)
        d = self.fund.download()
        self._last = dict(lk_status=status, applied=out["applied"], m=d["m"], n_hypotheses=len(d["samples"]), n_inliers=out["n_inliers"],
                          winner=d["winner"], mask=out["mask"], status=out["status"], F=out["F"], T1=d["T1"], T2=d["T2"],
                          n_valid_samples=int((d["n_models"] > 0).sum()))
        return to_xy, out["status"], err

    def process(self, left, right, delta_guess=None, outliers=()):
        self._last = None
        out, inter = super().process(left, right, delta_guess, outliers)
        if inter is not None:
            if self._last is None:
                inter["cull"] = inactive()
            else:
                inter["lk_status"] = self._last.pop("lk_status")      # visfs_tracker_download reports the status before the AND
                inter["cull"] = self._last
        return out, inter


def assert_same_cull(got, want, what=""):
    for key in CULL_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in CULL_ARRAYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, key)
