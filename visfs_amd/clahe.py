"""ctypes binding of the equalised frame push (include/visfs_clahe.h, in libvisfs_ba_hip.so) — plumbing only.

`push_frame(flow_obj, params, left, right)` is `flow.Flow.push_frame` with cv::CLAHE::apply on both images first: HIP kernels when the
object lives on a solver's device, the one-core host restatement otherwise.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import flow as _flow

ABI_VERSION = 1
EXPORTS = [
    "visfs_clahe_abi_version", "visfs_clahe_default_params", "visfs_flow_push_frame_clahe", "visfs_clahe_hook_geometry",
    "visfs_flow_clahe_last_tiles", "visfs_flow_clahe_download",
]
MAX_TILES = 32

IMAGE_LEFT, IMAGE_RIGHT = _flow.IMAGE_LEFT, _flow.IMAGE_RIGHT


class Params(C.Structure):
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32)]


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
    lib.visfs_clahe_abi_version.restype = C.c_int
    lib.visfs_clahe_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_clahe_default_params.restype = None
    lib.visfs_flow_push_frame_clahe.argtypes = [C.c_void_p, C.POINTER(Params), _pu8, _pu8, C.c_int32]
    lib.visfs_flow_push_frame_clahe.restype = C.c_int
    lib.visfs_clahe_hook_geometry.argtypes = [C.POINTER(Params), C.c_int32, C.c_int32, _pi32, _pi32, _pi32, _pi32, _pi32]
    lib.visfs_clahe_hook_geometry.restype = C.c_int
    lib.visfs_flow_clahe_last_tiles.argtypes = [C.c_void_p, _pi32, _pi32]
    lib.visfs_flow_clahe_last_tiles.restype = C.c_int
    lib.visfs_flow_clahe_download.argtypes = [C.c_void_p, C.c_int32, _pu8, _pi32]
    lib.visfs_flow_clahe_download.restype = C.c_int
    if lib.visfs_clahe_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/clahe.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_clahe_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def push_frame_status(flow_obj, params, left, right):
    """The status of visfs_flow_push_frame_clahe without raising: what the argument tests look at.  params: a Params or None."""
    lib = load()
    imgs = []
    for im in (left, right):
        im = np.asarray(im)
        if im.dtype != np.uint8 or im.shape != (flow_obj.height, flow_obj.width):
            raise ValueError("images must be uint8 [height][width]")
        imgs.append(im if im.strides[1] == 1 and im.strides[0] >= flow_obj.width else np.ascontiguousarray(im))
    if imgs[0].strides[0] != imgs[1].strides[0]:
        imgs = [np.ascontiguousarray(im) for im in imgs]
    return lib.visfs_flow_push_frame_clahe(flow_obj.h, C.byref(params) if params is not None else None, imgs[0].ctypes.data_as(_pu8),
                                           imgs[1].ctypes.data_as(_pu8), imgs[0].strides[0])


def push_frame(flow_obj, params, left, right):
    """left, right: uint8 [height][width] (any row stride); params: a Params (default_params())."""
    rc = push_frame_status(flow_obj, params, left, right)
    if rc != abi.OK:
        raise backend.BackendError(f"push_frame_clahe: status {rc}: {flow_obj.last_error()}")


def download(flow_obj, image=IMAGE_LEFT):
    """State of the last push_frame of `flow_obj` for one image: dict(lut [tiles_y][tiles_x][256] uint8, hist [tiles_y][tiles_x][256]
    int32, the histograms after clipping and redistribution)."""
    lib = load()
    tx, ty = C.c_int32(0), C.c_int32(0)
    rc = lib.visfs_flow_clahe_last_tiles(flow_obj.h, C.byref(tx), C.byref(ty))
    if rc != abi.OK:
        raise backend.BackendError(f"clahe download: status {rc}: no equalised push to report on")
    lut = np.zeros((ty.value, tx.value, 256), dtype=np.uint8); hist = np.zeros((ty.value, tx.value, 256), dtype=np.int32)
    rc = lib.visfs_flow_clahe_download(flow_obj.h, int(image), lut.ctypes.data_as(_pu8), hist.ctypes.data_as(_pi32))
    if rc != abi.OK:
        raise backend.BackendError(f"clahe download: status {rc}: {flow_obj.last_error()}")
    return dict(lut=lut, hist=hist)


def hook_geometry_status(params, w, h):
    v = [C.c_int32(0) for _ in range(5)]
    rc = load().visfs_clahe_hook_geometry(C.byref(params) if params is not None else None, int(w), int(h), *[C.byref(x) for x in v])
    return rc, dict(zip(("ext_w", "ext_h", "tile_w", "tile_h", "clip"), (x.value for x in v)))


def hook_geometry(params, w, h):
    """dict(ext_w, ext_h, tile_w, tile_h, clip) for a w x h image."""
    rc, out = hook_geometry_status(params, w, h)
    if rc != abi.OK:
        raise backend.BackendError(f"clahe geometry: status {rc}")
    return out
