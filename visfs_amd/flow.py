"""ctypes binding of the Lucas-Kanade tracker (include/visfs_flow.h, in libvisfs_ba_hip.so) — plumbing only.

`Flow(params, width, height, solver=s)` keeps the image pyramids on the device of `backend.Solver` `s` and tracks with HIP kernels;
`Flow(params, width, height)` without a solver is the host restatement (one core) the parity tests compare against.
"""
import ctypes as C

import numpy as np

from . import abi, backend

ABI_VERSION = 1
EXPORTS = [
    "visfs_flow_abi_version", "visfs_flow_default_params", "visfs_flow_create", "visfs_flow_create_host", "visfs_flow_destroy",
    "visfs_flow_last_error", "visfs_flow_push_frame", "visfs_flow_track", "visfs_flow_stereo", "visfs_flow_level_size",
    "visfs_flow_download_level", "visfs_flow_hook_triangulate",
]

SLOT_PREVIOUS, SLOT_CURRENT = 0, 1
IMAGE_LEFT, IMAGE_RIGHT = 0, 1


class Params(C.Structure):
    _fields_ = [("win_size", C.c_int32), ("max_level", C.c_int32), ("iterations", C.c_int32), ("eps", C.c_float),
                ("flow_back", C.c_int32), ("min_eig_threshold", C.c_float), ("back_gate_track", C.c_float),
                ("back_gate_stereo", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("cx_right", C.c_float),
                ("baseline", C.c_float), ("Tir", C.c_double * 12)]


_pf = C.POINTER(C.c_float)
_pu8 = C.POINTER(C.c_uint8)
_pi16 = C.POINTER(C.c_int16)
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
    lib.visfs_flow_abi_version.restype = C.c_int
    lib.visfs_flow_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_flow_default_params.restype = None
    lib.visfs_flow_create.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_flow_create.restype = C.c_int
    lib.visfs_flow_create_host.argtypes = [C.POINTER(Params), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_flow_create_host.restype = C.c_int
    lib.visfs_flow_destroy.argtypes = [C.c_void_p]
    lib.visfs_flow_destroy.restype = None
    lib.visfs_flow_last_error.argtypes = [C.c_void_p]
    lib.visfs_flow_last_error.restype = C.c_char_p
    lib.visfs_flow_push_frame.argtypes = [C.c_void_p, _pu8, _pu8, C.c_int32]
    lib.visfs_flow_push_frame.restype = C.c_int
    lib.visfs_flow_track.argtypes = [C.c_void_p, C.c_int32, _pf, _pf, _pf, _pu8, _pf]
    lib.visfs_flow_track.restype = C.c_int
    lib.visfs_flow_stereo.argtypes = [C.c_void_p, C.c_int32, _pf, C.POINTER(Camera), _pf, _pu8, _pf]
    lib.visfs_flow_stereo.restype = C.c_int
    lib.visfs_flow_level_size.argtypes = [C.c_void_p, C.c_int32, _pi32, _pi32]
    lib.visfs_flow_level_size.restype = C.c_int
    lib.visfs_flow_download_level.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _pu8, _pi16]
    lib.visfs_flow_download_level.restype = C.c_int
    lib.visfs_flow_hook_triangulate.argtypes = [C.POINTER(Params), C.POINTER(Camera), C.c_int32, _pf, _pf, _pf]
    lib.visfs_flow_hook_triangulate.restype = C.c_int
    if lib.visfs_flow_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/flow.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_flow_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def camera(fx=435.2, fy=435.2, cx=367.4, cy=252.2, cx_right=367.4, baseline=0.11, Tir=None):
    """The bench camera; Tir 3x4 row-major (default: the optical frame looking along the robot's x axis)."""
    c = Camera(fx, fy, cx, cy, cx_right, baseline)
    c.Tir[:] = [float(v) for v in (Tir if Tir is not None else [0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0])]
    return c


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _xy(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 2))


class Flow:
    """The tracker over the C ABI.  solver: a backend.Solver (device pyramids) or None (host restatement)."""

    def __init__(self, params, width, height, solver=None):
        self._lib = load()
        self.params = params if params is not None else default_params()
        self.width, self.height, self.solver = int(width), int(height), solver
        h = C.c_void_p()
        if solver is None:
            rc = self._lib.visfs_flow_create_host(C.byref(self.params), self.width, self.height, C.byref(h))
        else:
            rc = self._lib.visfs_flow_create(solver.h, C.byref(self.params), self.width, self.height, C.byref(h))
        self.status = rc
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_flow_create failed with status {rc}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_flow_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_flow_last_error(self.h).decode()

    def _check(self, rc, what):
        if rc != abi.OK:
            raise backend.BackendError(f"{what}: status {rc}: {self.last_error()}")

    def push_frame(self, left, right):
        """left, right: uint8 [height][width] (any row stride)."""
        imgs = []
        for im in (left, right):
            im = np.asarray(im)
            if im.dtype != np.uint8 or im.shape != (self.height, self.width):
                raise ValueError("images must be uint8 [height][width]")
            imgs.append(im if im.strides[1] == 1 and im.strides[0] >= self.width else np.ascontiguousarray(im))
        if imgs[0].strides[0] != imgs[1].strides[0]:
            imgs = [np.ascontiguousarray(im) for im in imgs]
        self._check(self._lib.visfs_flow_push_frame(self.h, _ptr(imgs[0], C.c_uint8), _ptr(imgs[1], C.c_uint8), imgs[0].strides[0]),
                    "push_frame")

    def track(self, from_xy, guess_xy=None):
        """(to_xy [n][2] float32, status [n] uint8, err [n] float32)."""
        p = _xy(from_xy)
        g = _xy(guess_xy) if guess_xy is not None else None
        n = len(p)
        to = np.zeros((n, 2), dtype=np.float32); st = np.zeros(n, dtype=np.uint8); err = np.zeros(n, dtype=np.float32)
        self._check(self._lib.visfs_flow_track(self.h, n, _ptr(p, C.c_float), _ptr(g, C.c_float) if g is not None else None,
                                               _ptr(to, C.c_float), _ptr(st, C.c_uint8), _ptr(err, C.c_float)), "track")
        return to, st, err

    def stereo(self, left_xy, cam):
        """(right_xy [n][2] float32, status [n] uint8, xyz [n][3] float32 in the robot frame, NaN where not triangulated)."""
        p = _xy(left_xy)
        n = len(p)
        to = np.zeros((n, 2), dtype=np.float32); st = np.zeros(n, dtype=np.uint8); xyz = np.zeros((n, 3), dtype=np.float32)
        self._check(self._lib.visfs_flow_stereo(self.h, n, _ptr(p, C.c_float), C.byref(cam), _ptr(to, C.c_float), _ptr(st, C.c_uint8),
                                                _ptr(xyz, C.c_float)), "stereo")
        return to, st, xyz

    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        self._check(self._lib.visfs_flow_level_size(self.h, level, C.byref(w), C.byref(h)), "level_size")
        return w.value, h.value

    def download_level(self, slot, image, level):
        """(pixels [h][w] uint8, derivative [h][w][2] int16) of one resident pyramid level."""
        w, h = self.level_size(level)
        px = np.zeros((h, w), dtype=np.uint8); der = np.zeros((h, w, 2), dtype=np.int16)
        self._check(self._lib.visfs_flow_download_level(self.h, slot, image, level, _ptr(px, C.c_uint8), _ptr(der, C.c_int16)),
                    "download_level")
        return px, der


def hook_triangulate(params, cam, left_xy, right_xy):
    l, r = _xy(left_xy), _xy(right_xy)
    xyz = np.zeros((len(l), 3), dtype=np.float32)
    rc = load().visfs_flow_hook_triangulate(C.byref(params), C.byref(cam), len(l), _ptr(l, C.c_float), _ptr(r, C.c_float), _ptr(xyz, C.c_float))
    assert rc == abi.OK, rc
    return xyz
