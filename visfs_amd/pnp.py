"""ctypes binding of the PnP-RANSAC pose guess (include/visfs_pnp.h, in libvisfs_ba_hip.so) — plumbing only.

`Pnp(capacity, solver=s)` runs estimateMotion3DTo2D as HIP kernels on the stream of `backend.Solver` `s`; `Pnp(capacity)` without
a solver is the host restatement (one core) the parity tests compare against.
"""
import ctypes as C

import numpy as np

from . import abi, backend

ABI_VERSION = 1
EXPORTS = [
    "visfs_pnp_abi_version", "visfs_pnp_default_params", "visfs_pnp_create", "visfs_pnp_create_host", "visfs_pnp_destroy",
    "visfs_pnp_last_error", "visfs_pnp_solve", "visfs_pnp_last_sizes", "visfs_pnp_download",
]
MAX_POINTS = 4096
MAX_ITERATIONS = 4096
MAX_REFINE = 32


class Params(C.Structure):
    _fields_ = [("min_inliers", C.c_int32), ("iterations", C.c_int32), ("reproj_error", C.c_float), ("refine_iterations", C.c_int32),
                ("refine_sigma", C.c_float), ("seed", C.c_uint64)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("Tir", C.c_double * 12)]


_pf = C.POINTER(C.c_float)
_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_pnp_abi_version.restype = C.c_int
    lib.visfs_pnp_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_pnp_default_params.restype = None
    lib.visfs_pnp_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_pnp_create.restype = C.c_int
    lib.visfs_pnp_create_host.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_pnp_create_host.restype = C.c_int
    lib.visfs_pnp_destroy.argtypes = [C.c_void_p]
    lib.visfs_pnp_destroy.restype = None
    lib.visfs_pnp_last_error.argtypes = [C.c_void_p]
    lib.visfs_pnp_last_error.restype = C.c_char_p
    lib.visfs_pnp_solve.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Camera), C.c_int32, _pf, _pf, _pf, _pd, _pd, _pi32, _pi32,
                                    _pi32, _pi32]
    lib.visfs_pnp_solve.restype = C.c_int
    lib.visfs_pnp_last_sizes.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_pnp_last_sizes.restype = C.c_int
    lib.visfs_pnp_download.argtypes = [C.c_void_p, _pi32, _pi32, _pd, _pi32, _pi32, _pd, _pd, _pf, _pi32, _pi32]
    lib.visfs_pnp_download.restype = C.c_int
    if lib.visfs_pnp_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/pnp.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_pnp_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def camera(fx=435.2, fy=435.2, cx=367.4, cy=252.2, Tir=None):
    """The bench camera; Tir 3x4 row-major (default: the optical frame looking along the robot's x axis)."""
    c = Camera(fx, fy, cx, cy)
    c.Tir[:] = [float(v) for v in (Tir if Tir is not None else [0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0])]
    return c


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Pnp:
    """The solver over the C ABI.  solver: a backend.Solver (device) or None (host restatement)."""

    def __init__(self, capacity=MAX_POINTS, solver=None):
        self._lib = load()
        self.capacity, self.solver = int(capacity), solver
        h = C.c_void_p()
        if solver is None:
            rc = self._lib.visfs_pnp_create_host(self.capacity, C.byref(h))
        else:
            rc = self._lib.visfs_pnp_create(solver.h, self.capacity, C.byref(h))
        self.status = rc
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_pnp_create failed with status {rc}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_pnp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_pnp_last_error(self.h).decode()

    def solve_status(self, params, cam, from_xyz, to_xy, to_xyz=None):
        """(status, result dict): T [4][4], cov [6][6], matches, inliers (row numbers, int32)."""
        a = np.ascontiguousarray(np.asarray(from_xyz, dtype=np.float32).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(to_xy, dtype=np.float32).reshape(-1, 2))
        c = np.ascontiguousarray(np.asarray(to_xyz, dtype=np.float32).reshape(-1, 3)) if to_xyz is not None else None
        n = len(a)
        if len(b) != n or (c is not None and len(c) != n):
            raise ValueError("from_xyz, to_xy and to_xyz must have the same number of rows")
        T = np.zeros((4, 4)); cov = np.zeros((6, 6))
        matches = np.zeros(max(n, 1), dtype=np.int32); inliers = np.zeros(max(n, 1), dtype=np.int32)
        nm, ni = C.c_int32(), C.c_int32()
        rc = self._lib.visfs_pnp_solve(self.h, C.byref(params), C.byref(cam), n, _ptr(a, C.c_float), _ptr(b, C.c_float),
                                       _ptr(c, C.c_float) if c is not None else None, _ptr(T, C.c_double), _ptr(cov, C.c_double),
                                       _ptr(matches, C.c_int32), C.byref(nm), _ptr(inliers, C.c_int32), C.byref(ni))
        return rc, {"T": T, "cov": cov, "matches": matches[:nm.value].copy(), "inliers": inliers[:ni.value].copy()}

    def solve(self, params, cam, from_xyz, to_xy, to_xyz=None):
        rc, out = self.solve_status(params, cam, from_xyz, to_xy, to_xyz)
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_pnp_solve: status {rc}: {self.last_error()}")
        return out

    def download(self):
        """State of the last solve: per-hypothesis samples [H][4], valid [H], models [H][3][4], counts [H]; winner; refit_tq [7];
        per refinement pass pass_tq [R][7], pass_threshold [R], pass_count [R], pass_inliers [R][m] (-1 behind the count)."""
        m, H, R = C.c_int32(), C.c_int32(), C.c_int32()
        rc = self._lib.visfs_pnp_last_sizes(self.h, C.byref(m), C.byref(H), C.byref(R))
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_pnp_last_sizes: status {rc}")
        m, H, R = m.value, H.value, R.value
        out = {"m": m, "samples": np.zeros((H, 4), dtype=np.int32), "valid": np.zeros(H, dtype=np.int32), "models": np.zeros((H, 3, 4)),
               "counts": np.zeros(H, dtype=np.int32), "refit_tq": np.zeros(7), "pass_tq": np.zeros((R, 7)),
               "pass_threshold": np.zeros(R, dtype=np.float32), "pass_count": np.zeros(R, dtype=np.int32),
               "pass_inliers": np.zeros((R, m), dtype=np.int32)}
        w = C.c_int32()
        rc = self._lib.visfs_pnp_download(self.h, _ptr(out["samples"], C.c_int32), _ptr(out["valid"], C.c_int32), _ptr(out["models"], C.c_double),
                                          _ptr(out["counts"], C.c_int32), C.byref(w), _ptr(out["refit_tq"], C.c_double),
                                          _ptr(out["pass_tq"], C.c_double), _ptr(out["pass_threshold"], C.c_float),
                                          _ptr(out["pass_count"], C.c_int32), _ptr(out["pass_inliers"], C.c_int32))
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_pnp_download: status {rc}: {self.last_error()}")
        out["winner"] = w.value
        return out
