"""ctypes binding of the corner extraction (include/visfs_corners.h, in libvisfs_ba_hip.so) — plumbing only.

`corners(flow_obj, ...)` runs goodFeaturesToTrack on a resident level-0 image of a `flow.Flow`: HIP kernels when the object lives on
a solver's device, the one-core host restatement otherwise.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import flow as _flow

ABI_VERSION = 1
EXPORTS = [
    "visfs_corners_abi_version", "visfs_corners_default_params", "visfs_flow_corners", "visfs_flow_corners_download",
    "visfs_flow_corners_last_discs", "visfs_corners_hook_halfwidth",
]
MAX_CORNERS = 4096
MAX_RADIUS = 32768

SLOT_PREVIOUS, SLOT_CURRENT = _flow.SLOT_PREVIOUS, _flow.SLOT_CURRENT
IMAGE_LEFT, IMAGE_RIGHT = _flow.IMAGE_LEFT, _flow.IMAGE_RIGHT


class Params(C.Structure):
    _fields_ = [("max_corners", C.c_int32), ("quality_level", C.c_double), ("min_distance", C.c_double)]


class Disc(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("radius", C.c_int32)]


DISC_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("radius", np.int32)])

_pf = C.POINTER(C.c_float)
_pu8 = C.POINTER(C.c_uint8)
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
    lib.visfs_corners_abi_version.restype = C.c_int
    lib.visfs_corners_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_corners_default_params.restype = None
    lib.visfs_flow_corners.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int32, C.c_void_p, C.c_int32, _pf, _pi32]
    lib.visfs_flow_corners.restype = C.c_int
    lib.visfs_flow_corners_download.argtypes = [C.c_void_p, _pf, _pu8, _pu8, _pi32, _pf]
    lib.visfs_flow_corners_download.restype = C.c_int
    lib.visfs_flow_corners_last_discs.argtypes = [C.c_void_p, _pi32]
    lib.visfs_flow_corners_last_discs.restype = C.c_int
    lib.visfs_corners_hook_halfwidth.argtypes = [C.c_int32, _pi32]
    lib.visfs_corners_hook_halfwidth.restype = C.c_int
    if lib.visfs_corners_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/corners.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_corners_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def make_discs(discs):
    """discs: None, a DISC_DTYPE array, or rows (x, y, radius) -> a contiguous DISC_DTYPE array."""
    if discs is None:
        return np.zeros(0, dtype=DISC_DTYPE)
    if isinstance(discs, np.ndarray) and discs.dtype == DISC_DTYPE:
        return np.ascontiguousarray(discs)
    out = np.zeros(len(discs), dtype=DISC_DTYPE)
    for i, (x, y, r) in enumerate(discs):
        out[i] = (x, y, r)
    return out


def corners_status(flow_obj, slot=SLOT_CURRENT, image=IMAGE_LEFT, discs=None, capacity=None, **params):
    """(status, xy float32 [n][2]) without raising: what the argument tests look at."""
    lib = load()
    p = default_params(**params)
    d = make_discs(discs)
    cap = int(capacity) if capacity is not None else max(int(p.max_corners), 1)
    xy = np.zeros((max(cap, 1), 2), dtype=np.float32)
    n = C.c_int32(0)
    rc = lib.visfs_flow_corners(flow_obj.h, slot, image, C.byref(p), len(d), d.ctypes.data if len(d) else None, cap,
                                xy.ctypes.data_as(_pf), C.byref(n))
    return rc, xy[:n.value].copy()


def corners(flow_obj, slot=SLOT_CURRENT, image=IMAGE_LEFT, discs=None, **params):
    """goodFeaturesToTrack on a resident image of `flow_obj` -> float32 [n][2], strongest first.  params: max_corners,
    quality_level, min_distance; discs: the mask (see make_discs)."""
    rc, xy = corners_status(flow_obj, slot, image, discs, **params)
    if rc != abi.OK:
        raise backend.BackendError(f"corners: status {rc}: {flow_obj.last_error()}")
    return xy


def download(flow_obj, n_discs=None):
    """State of the last corners call: dict(eig [h][w] float32, mask [h][w] uint8, disc_drawn [n] uint8, n_candidates, max_val).  The
    library says how many discs that call had; n_discs, if given, must agree."""
    lib = load()
    last = C.c_int32(0)
    rc = lib.visfs_flow_corners_last_discs(flow_obj.h, C.byref(last))
    if rc != abi.OK:
        raise backend.BackendError(f"corners download: status {rc}: no corner call to report on")
    if n_discs is not None and int(n_discs) != last.value:
        raise ValueError(f"the last corners call had {last.value} discs, not {n_discs}")
    h, w = flow_obj.height, flow_obj.width
    eig = np.zeros((h, w), dtype=np.float32); mask = np.zeros((h, w), dtype=np.uint8)
    drawn = np.zeros(last.value, dtype=np.uint8)
    nc, mv = C.c_int32(0), C.c_float(0.0)
    rc = lib.visfs_flow_corners_download(flow_obj.h, eig.ctypes.data_as(_pf), mask.ctypes.data_as(_pu8),
                                         drawn.ctypes.data_as(_pu8) if last.value else None, C.byref(nc), C.byref(mv))
    if rc != abi.OK:
        raise backend.BackendError(f"corners download: status {rc}: {flow_obj.last_error()}")
    return dict(eig=eig, mask=mask, disc_drawn=drawn, n_candidates=nc.value, max_val=np.float32(mv.value))


def halfwidth(radius):
    hw = np.zeros(max(int(radius), 0) + 1, dtype=np.int32)
    rc = load().visfs_corners_hook_halfwidth(int(radius), hw.ctypes.data_as(_pi32))
    if rc != abi.OK:
        raise backend.BackendError(f"halfwidth: status {rc}")
    return hw
