"""ctypes binding of the pose guess inside the resident front end (include/visfs_tracker_pnp.h, in libvisfs_ba_hip.so) — plumbing only.

`enable(trk, params)` makes a `tracker.Tracker` run estimateMotion3DTo2D inside its process calls, single or grouped, on the covisible
rows of each call (`params`: a `pnp.Params`; None switches it off again); `last(trk)` is the pose guess of its last call as
`pnp.Pnp.solve` returns it; `download(trk)` is the test hook, as `pnp.Pnp.download` reports it.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import pnp as _pnp
from . import tracker as _tracker

ABI_VERSION = 1
EXPORTS = ["visfs_tracker_pnp_abi_version", "visfs_tracker_enable_pnp", "visfs_tracker_pnp_last", "visfs_tracker_download_pnp"]

_pf = C.POINTER(C.c_float)
_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)


class Result(C.Structure):
    _fields_ = [("ran", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("pad", C.c_int32), ("matches", _pi32),
                ("inliers", _pi32), ("T", C.c_double * 16), ("cov", C.c_double * 36)]


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    _tracker.load()
    _pnp.load()
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_tracker_pnp_abi_version.restype = C.c_int
    lib.visfs_tracker_enable_pnp.argtypes = [C.c_void_p, C.POINTER(_pnp.Params)]
    lib.visfs_tracker_enable_pnp.restype = C.c_int
    lib.visfs_tracker_pnp_last.argtypes = [C.c_void_p, C.POINTER(Result)]
    lib.visfs_tracker_pnp_last.restype = C.c_int
    lib.visfs_tracker_download_pnp.argtypes = [C.c_void_p, _pi32, _pi32, _pi32, _pi32, _pi32, _pd, _pi32, _pi32, _pd, _pd, _pf, _pi32, _pi32]
    lib.visfs_tracker_download_pnp.restype = C.c_int
    if lib.visfs_tracker_pnp_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/tracker_pnp.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def enable_status(trk, params):
    return load().visfs_tracker_enable_pnp(trk.h, C.byref(params) if params is not None else None)


def enable(trk, params):
    """params: a pnp.Params, or None to switch the pose guess off.  Enable before the tracker joins a group."""
    rc = enable_status(trk, params)
    if rc != abi.OK:
        raise backend.BackendError(f"visfs_tracker_enable_pnp: status {rc}: {trk.last_error()}")


def last_status(trk):
    """(status, dict(ran, T [4][4], cov [6][6], matches, inliers: covisible row numbers, int32) or None)."""
    res = Result()
    rc = load().visfs_tracker_pnp_last(trk.h, C.byref(res))
    if rc != abi.OK:
        return rc, None
    take = lambda ptr, n: np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n > 0 else np.zeros(0, dtype=np.int32)
    return rc, {"ran": int(res.ran), "T": np.array(res.T[:]).reshape(4, 4), "cov": np.array(res.cov[:]).reshape(6, 6),
                "matches": take(res.matches, res.n_matches), "inliers": take(res.inliers, res.n_inliers)}


def last(trk):
    rc, out = last_status(trk)
    if rc != abi.OK:
        raise backend.BackendError(f"visfs_tracker_pnp_last: status {rc}")
    return out


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def download(trk):
    """State of the pose guess of the last call, with the keys and shapes of pnp.Pnp.download; all sizes 0 and winner -1 when it did
    not run."""
    lib = load()
    m, H, R = C.c_int32(), C.c_int32(), C.c_int32()
    none = [None] * 10
    rc = lib.visfs_tracker_download_pnp(trk.h, C.byref(m), C.byref(H), C.byref(R), *none)
    if rc != abi.OK:
        raise backend.BackendError(f"tracker download_pnp: status {rc}: {trk.last_error()}")
    m, H, R = m.value, H.value, R.value
    out = {"m": m, "samples": np.zeros((H, 4), dtype=np.int32), "valid": np.zeros(H, dtype=np.int32), "models": np.zeros((H, 3, 4)),
           "counts": np.zeros(H, dtype=np.int32), "refit_tq": np.zeros(7), "pass_tq": np.zeros((R, 7)),
           "pass_threshold": np.zeros(R, dtype=np.float32), "pass_count": np.zeros(R, dtype=np.int32),
           "pass_inliers": np.zeros((R, m), dtype=np.int32)}
    w = C.c_int32()
    rc = lib.visfs_tracker_download_pnp(trk.h, None, None, None, _ptr(out["samples"], C.c_int32), _ptr(out["valid"], C.c_int32),
                                        _ptr(out["models"], C.c_double), _ptr(out["counts"], C.c_int32), C.byref(w),
                                        _ptr(out["refit_tq"], C.c_double), _ptr(out["pass_tq"], C.c_double),
                                        _ptr(out["pass_threshold"], C.c_float), _ptr(out["pass_count"], C.c_int32),
                                        _ptr(out["pass_inliers"], C.c_int32))
    if rc != abi.OK:
        raise backend.BackendError(f"tracker download_pnp: status {rc}: {trk.last_error()}")
    out["winner"] = w.value
    return out
