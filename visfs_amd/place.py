"""ctypes binding of visual place recognition (include/visfs_place.h, in libvisfs_ba_hip.so) — plumbing only.

`DescriptorSet(flow_obj, capacity)` describes key-points on a resident level-0 image of a `flow.Flow`; `KeyFrameStore(solver)` keeps
key-frames and answers `query(set)`.  HIP kernels when the flow object / the store lives on a solver's device, the one-core twin
otherwise (`Flow` without a solver, `KeyFrameStore(None)`).
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import flow as _flow

ABI_VERSION = 1
EXPORTS = [
    "visfs_place_abi_version", "visfs_place_default_params", "visfs_place_set_create", "visfs_place_set_destroy",
    "visfs_place_set_last_error", "visfs_place_describe", "visfs_place_set_last_counts", "visfs_place_set_download",
    "visfs_place_db_create", "visfs_place_db_destroy", "visfs_place_db_last_error", "visfs_place_db_add", "visfs_place_db_reset",
    "visfs_place_db_size", "visfs_place_query", "visfs_place_last_counts", "visfs_place_db_download", "visfs_place_hook_pattern",
    "visfs_place_set_upload",
]
MAX_POINTS = 512
MAX_KEYFRAMES = 1024
MAX_CANDIDATES = 8
BINS = 32
MARGIN = 15
QUERY_LAUNCHES = 2
NO_SECOND = 257

SLOT_PREVIOUS, SLOT_CURRENT = _flow.SLOT_PREVIOUS, _flow.SLOT_CURRENT
IMAGE_LEFT, IMAGE_RIGHT = _flow.IMAGE_LEFT, _flow.IMAGE_RIGHT


class Params(C.Structure):
    _fields_ = [("first_slot", C.c_int32), ("last_slot", C.c_int32), ("max_distance", C.c_int32), ("ratio_num", C.c_int32),
                ("ratio_den", C.c_int32), ("min_matches", C.c_int32), ("cross_check", C.c_int32)]


class Row(C.Structure):
    _fields_ = [("query_index", C.c_int32), ("db_index", C.c_int32), ("distance", C.c_int32), ("id", C.c_int32),
                ("from_xyz", C.c_float * 3), ("to_xy", C.c_float * 2)]


class Candidate(C.Structure):
    _fields_ = [("slot", C.c_int32), ("count", C.c_int32), ("key", C.c_int64)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_slots", C.c_int32), ("n_candidates", C.c_int32), ("first_slot", C.c_int32),
                ("candidate", Candidate * MAX_CANDIDATES), ("count", C.c_int32 * MAX_KEYFRAMES),
                ("row", (Row * MAX_POINTS) * MAX_CANDIDATES)]


ROW_DTYPE = np.dtype([("query_index", np.int32), ("db_index", np.int32), ("distance", np.int32), ("id", np.int32),
                      ("from_xyz", np.float32, 3), ("to_xy", np.float32, 2)])
assert ROW_DTYPE.itemsize == C.sizeof(Row) == 36

_pf = C.POINTER(C.c_float)
_pu8 = C.POINTER(C.c_uint8)
_pi8 = C.POINTER(C.c_int8)
_pi32 = C.POINTER(C.c_int32)
_pi64 = C.POINTER(C.c_int64)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_place_abi_version.restype = C.c_int
    lib.visfs_place_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_place_default_params.restype = None
    lib.visfs_place_set_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_place_set_create.restype = C.c_int
    lib.visfs_place_set_destroy.argtypes = [C.c_void_p]
    lib.visfs_place_set_destroy.restype = None
    lib.visfs_place_set_last_error.argtypes = [C.c_void_p]
    lib.visfs_place_set_last_error.restype = C.c_char_p
    lib.visfs_place_describe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _pf]
    lib.visfs_place_describe.restype = C.c_int
    lib.visfs_place_set_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32, _pi32]
    lib.visfs_place_set_last_counts.restype = C.c_int
    lib.visfs_place_set_download.argtypes = [C.c_void_p, _pi32, _pf, _pu8, _pu8, _pu8]
    lib.visfs_place_set_download.restype = C.c_int
    lib.visfs_place_set_upload.argtypes = [C.c_void_p, C.c_int32, _pf, _pu8, _pu8]
    lib.visfs_place_set_upload.restype = C.c_int
    lib.visfs_place_db_create.argtypes =[C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_place_db_create.restype = C.c_int
    lib.visfs_place_db_destroy.argtypes = [C.c_void_p]
    lib.visfs_place_db_destroy.restype = None
    lib.visfs_place_db_last_error.argtypes = [C.c_void_p]
    lib.visfs_place_db_last_error.restype = C.c_char_p
    lib.visfs_place_db_add.argtypes = [C.c_void_p, C.c_void_p, _pi32, _pf, C.c_int64, _pi32]
    lib.visfs_place_db_add.restype = C.c_int
    lib.visfs_place_db_reset.argtypes = [C.c_void_p]
    lib.visfs_place_db_reset.restype = C.c_int
    lib.visfs_place_db_size.argtypes = [C.c_void_p, _pi32]
    lib.visfs_place_db_size.restype = C.c_int
    lib.visfs_place_query.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(Result)]
    lib.visfs_place_query.restype = C.c_int
    lib.visfs_place_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32, _pi32]
    lib.visfs_place_last_counts.restype = C.c_int
    lib.visfs_place_db_download.argtypes = [C.c_void_p, C.c_int32, _pi32, _pi64, _pu8, _pu8, _pi32, _pf]
    lib.visfs_place_db_download.restype = C.c_int
    lib.visfs_place_hook_pattern.argtypes = [_pi8]
    lib.visfs_place_hook_pattern.restype = C.c_int
    if lib.visfs_place_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/place.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_place_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def pattern():
    """The rotated test points, int8 [32][512][2]."""
    pts = np.zeros((BINS, 512, 2), dtype=np.int8)
    rc = load().visfs_place_hook_pattern(pts.ctypes.data_as(_pi8))
    if rc != abi.OK:
        raise backend.BackendError(f"pattern: status {rc}")
    return pts


def _counts(fn, h):
    v = [C.c_int32(-1) for _ in range(4)]
    rc = fn(h, *[C.byref(x) for x in v])
    if rc != abi.OK:
        raise backend.BackendError(f"last_counts: status {rc}")
    return tuple(x.value for x in v)


class DescriptorSet:
    """The descriptors of one frame's key-points, resident where `flow_obj` lives.  Close it before the flow object."""

    def __init__(self, flow_obj, capacity=MAX_POINTS):
        self._lib = load()
        self.flow = flow_obj
        h = C.c_void_p()
        self.status = self._lib.visfs_place_set_create(flow_obj.h, int(capacity), C.byref(h))
        if self.status != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_place_set_create failed with status {self.status}: {flow_obj.last_error()}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_place_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_place_set_last_error(self.h).decode()

    def describe_status(self, xy, slot=SLOT_CURRENT, image=IMAGE_LEFT):
        p = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2))
        return self._lib.visfs_place_describe(self.h, slot, image, len(p), p.ctypes.data_as(_pf) if len(p) else None)

    def describe(self, xy, slot=SLOT_CURRENT, image=IMAGE_LEFT):
        rc = self.describe_status(xy, slot, image)
        if rc != abi.OK:
            raise backend.BackendError(f"describe: status {rc}: {self.last_error()}")

    def upload(self, xy, desc, valid):
        """Test hook: descriptors made to order in place of a describe."""
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2))
        desc = np.ascontiguousarray(np.asarray(desc, dtype=np.uint8).reshape(-1, 32))
        valid = np.ascontiguousarray(np.asarray(valid, dtype=np.uint8).reshape(-1))
        if not len(xy) == len(desc) == len(valid):
            raise ValueError("xy, desc and valid must have one row per key-point")
        n = len(xy)
        rc = self._lib.visfs_place_set_upload(self.h, n, xy.ctypes.data_as(_pf) if n else None, desc.ctypes.data_as(_pu8) if n else None,
                                              valid.ctypes.data_as(_pu8) if n else None)
        if rc != abi.OK:
            raise backend.BackendError(f"set upload: status {rc}: {self.last_error()}")

    def last_counts(self):
        """(uploads, launches, downloads, waits) of the last describe."""
        return _counts(self._lib.visfs_place_set_last_counts, self.h)

    def download(self):
        """dict(xy [n][2] float32, desc [n][32] uint8, valid [n] uint8, bin [n] uint8) of the last describe."""
        n = C.c_int32(0)
        rc = self._lib.visfs_place_set_download(self.h, C.byref(n), None, None, None, None)
        if rc != abi.OK:
            raise backend.BackendError(f"set download: status {rc}: {self.last_error()}")
        m = n.value
        xy = np.zeros((m, 2), dtype=np.float32); desc = np.zeros((m, 32), dtype=np.uint8)
        valid = np.zeros(m, dtype=np.uint8); bins = np.zeros(m, dtype=np.uint8)
        if m:
            rc = self._lib.visfs_place_set_download(self.h, C.byref(n), xy.ctypes.data_as(_pf), desc.ctypes.data_as(_pu8),
                                                    valid.ctypes.data_as(_pu8), bins.ctypes.data_as(_pu8))
            if rc != abi.OK:
                raise backend.BackendError(f"set download: status {rc}: {self.last_error()}")
        return dict(xy=xy, desc=desc, valid=valid, bin=bins)


class KeyFrameStore:
    """The key-frame store.  solver: a backend.Solver (device) or None (host twin)."""

    def __init__(self, solver=None, max_keyframes=MAX_KEYFRAMES):
        self._lib = load()
        self.solver = solver
        h = C.c_void_p()
        self.status = self._lib.visfs_place_db_create(solver.h if solver is not None else None, int(max_keyframes), C.byref(h))
        if self.status != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_place_db_create failed with status {self.status}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_place_db_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_place_db_last_error(self.h).decode()

    def add_status(self, dset, ids, xyz, key=0):
        """(status, slot)"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
        slot = C.c_int32(-1)
        rc = self._lib.visfs_place_db_add(self.h, dset.h, ids.ctypes.data_as(_pi32) if len(ids) else None,
                                          xyz.ctypes.data_as(_pf) if len(xyz) else None, int(key), C.byref(slot))
        return rc, slot.value

    def add(self, dset, ids, xyz, key=0):
        rc, slot = self.add_status(dset, ids, xyz, key)
        if rc != abi.OK:
            raise backend.BackendError(f"db_add: status {rc}: {self.last_error()}")
        return slot

    def reset(self):
        self._lib.visfs_place_db_reset(self.h)

    def size(self):
        n = C.c_int32(0)
        self._lib.visfs_place_db_size(self.h, C.byref(n))
        return n.value

    def query_raw(self, dset, **params):
        """(status, Result)"""
        p = default_params(**params)
        r = Result()
        return self._lib.visfs_place_query(self.h, dset.h, C.byref(p), C.byref(r)), r

    def query(self, dset, **params):
        """dict(n_slots, first_slot, count int32 [n_slots], candidates: list of dict(slot, key, count, rows ROW_DTYPE [count]),
        raw: the whole result block as bytes)."""
        rc, r = self.query_raw(dset, **params)
        if rc != abi.OK:
            raise backend.BackendError(f"query: status {rc}: {self.last_error()}")
        return unpack(r)

    def last_counts(self):
        """(uploads, launches, downloads, waits) of the last query."""
        return _counts(self._lib.visfs_place_last_counts, self.h)

    def download(self, slot):
        """dict(key, desc [n][32], valid [n], ids [n], xyz [n][3]) of one slot."""
        n, key = C.c_int32(0), C.c_int64(0)
        desc = np.zeros((MAX_POINTS, 32), dtype=np.uint8); valid = np.zeros(MAX_POINTS, dtype=np.uint8)
        ids = np.zeros(MAX_POINTS, dtype=np.int32); xyz = np.zeros((MAX_POINTS, 3), dtype=np.float32)
        rc = self._lib.visfs_place_db_download(self.h, int(slot), C.byref(n), C.byref(key), desc.ctypes.data_as(_pu8),
                                               valid.ctypes.data_as(_pu8), ids.ctypes.data_as(_pi32), xyz.ctypes.data_as(_pf))
        if rc != abi.OK:
            raise backend.BackendError(f"db download: status {rc}: {self.last_error()}")
        m = n.value
        return dict(key=key.value, desc=desc[:m].copy(), valid=valid[:m].copy(), ids=ids[:m].copy(), xyz=xyz[:m].copy())


def unpack(r):
    rows = np.frombuffer(bytes(memoryview(r.row)), dtype=ROW_DTYPE).reshape(MAX_CANDIDATES, MAX_POINTS)
    cands = []
    for c in range(r.n_candidates):
        k = r.candidate[c]
        cands.append(dict(slot=k.slot, key=k.key, count=k.count, rows=rows[c, :k.count].copy()))
    return dict(status=r.status, n_slots=r.n_slots, first_slot=r.first_slot,
                count=np.array(r.count[:r.n_slots], dtype=np.int32), candidates=cands, raw=bytes(memoryview(r)))
