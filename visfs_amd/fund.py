"""ctypes binding of the fundamental-matrix cull (include/visfs_fund.h, in libvisfs_ba_hip.so) — plumbing only.

`Fund(capacity, solver=s)` runs Tracker::rejectOutlierWithFundationMatrix as HIP kernels on the stream of `backend.Solver` `s`;
`Fund(capacity)` without a solver is the host restatement (one core) the parity tests compare against.
"""
import ctypes as C

import numpy as np

from . import abi, backend

ABI_VERSION = 1
EXPORTS = [
    "visfs_fund_abi_version", "visfs_fund_default_params", "visfs_fund_create", "visfs_fund_create_host", "visfs_fund_destroy",
    "visfs_fund_last_error", "visfs_fund_cull", "visfs_fund_last_sizes", "visfs_fund_download",
]
MAX_POINTS = 4096
MAX_ITERATIONS = 4096


class Params(C.Structure):
    _fields_ = [("pixel_error", C.c_float), ("iterations", C.c_int32), ("seed", C.c_uint64)]


_pf = C.POINTER(C.c_float)
_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_fund_abi_version.restype = C.c_int
    lib.visfs_fund_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_fund_default_params.restype = None
    lib.visfs_fund_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_fund_create.restype = C.c_int
    lib.visfs_fund_create_host.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_fund_create_host.restype = C.c_int
    lib.visfs_fund_destroy.argtypes = [C.c_void_p]
    lib.visfs_fund_destroy.restype = None
    lib.visfs_fund_last_error.argtypes = [C.c_void_p]
    lib.visfs_fund_last_error.restype = C.c_char_p
    lib.visfs_fund_cull.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, _pf, _pf, _pu8, _pu8, _pu8, _pd, _pi32, _pi32]
    lib.visfs_fund_cull.restype = C.c_int
    lib.visfs_fund_last_sizes.argtypes = [C.c_void_p, _pi32, _pi32]
    lib.visfs_fund_last_sizes.restype = C.c_int
    lib.visfs_fund_download.argtypes = [C.c_void_p, _pi32, _pi32, _pd, _pi32, _pi32, _pi32, _pd, _pd]
    lib.visfs_fund_download.restype = C.c_int
    if lib.visfs_fund_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/fund.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_fund_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Fund:
    """The cull over the C ABI.  solver: a backend.Solver (device) or None (host restatement)."""

    def __init__(self, capacity=MAX_POINTS, solver=None):
        self._lib = load()
        self.capacity, self.solver = int(capacity), solver
        h = C.c_void_p()
        if solver is None:
            rc = self._lib.visfs_fund_create_host(self.capacity, C.byref(h))
        else:
            rc = self._lib.visfs_fund_create(solver.h, self.capacity, C.byref(h))
        self.status = rc
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_fund_create failed with status {rc}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_fund_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_fund_last_error(self.h).decode()

    def cull_status(self, params, from_xy, to_xy, status, in_place=False):
        """(status code, result dict): status [n] and mask [n] (uint8), F [3][3], n_inliers, applied.  in_place: the ANDed status is
        written over the array handed in as the status (status_out aliases status_in)."""
        a = np.ascontiguousarray(np.asarray(from_xy, dtype=np.float32).reshape(-1, 2))
        b = np.ascontiguousarray(np.asarray(to_xy, dtype=np.float32).reshape(-1, 2))
        n = len(a)
        st_in = np.ascontiguousarray(np.asarray(status, dtype=np.uint8).reshape(-1))
        if len(b) != n or len(st_in) != n:
            raise ValueError("from_xy, to_xy and status must have the same number of rows")
        if in_place:
            st_in = st_in.copy()
        st_out = st_in if in_place else np.zeros(n, dtype=np.uint8)
        mask = np.zeros(n, dtype=np.uint8)
        F = np.zeros((3, 3))
        ni, ap = C.c_int32(), C.c_int32()
        rc = self._lib.visfs_fund_cull(self.h, C.byref(params), n, _ptr(a, C.c_float), _ptr(b, C.c_float), _ptr(st_in, C.c_uint8),
                                       _ptr(st_out, C.c_uint8), _ptr(mask, C.c_uint8), _ptr(F, C.c_double), C.byref(ni), C.byref(ap))
        return rc, {"status": st_out, "mask": mask, "F": F, "n_inliers": ni.value, "applied": ap.value}

    def cull(self, params, from_xy, to_xy, status, in_place=False):
        rc, out = self.cull_status(params, from_xy, to_xy, status, in_place)
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_fund_cull: status {rc}: {self.last_error()}")
        return out

    def download(self):
        """State of the last cull: m; per hypothesis samples [H][7], n_models [H], models [H][3][3][3] (conditioned, in their order),
        counts [H][3]; winner (h, k); T1, T2 [3][3]."""
        m, H = C.c_int32(), C.c_int32()
        rc = self._lib.visfs_fund_last_sizes(self.h, C.byref(m), C.byref(H))
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_fund_last_sizes: status {rc}")
        m, H = m.value, H.value
        out = {"m": m, "samples": np.zeros((H, 7), dtype=np.int32), "n_models": np.zeros(H, dtype=np.int32),
               "models": np.zeros((H, 3, 3, 3)), "counts": np.zeros((H, 3), dtype=np.int32), "T1": np.zeros((3, 3)), "T2": np.zeros((3, 3))}
        wh, wk = C.c_int32(), C.c_int32()
        rc = self._lib.visfs_fund_download(self.h, _ptr(out["samples"], C.c_int32), _ptr(out["n_models"], C.c_int32),
                                           _ptr(out["models"], C.c_double), _ptr(out["counts"], C.c_int32), C.byref(wh), C.byref(wk),
                                           _ptr(out["T1"], C.c_double), _ptr(out["T2"], C.c_double))
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_fund_download: status {rc}: {self.last_error()}")
        out["winner"] = (wh.value, wk.value)
        return out
