"""ctypes binding of the laser pretreatment with its voxel filters (include/visfs_scan_filter.h, in libvisfs_ba_hip.so) — plumbing only.

`ScanFilter(solver)` runs k_scan_filter on the device of `backend.Solver` `solver`; `ScanFilter()` is the one-core host twin.
`.process(scans, params)` takes a list of (points[n][3], T_laser_to_camera, origin) and returns (status, records);
`.range_data(i)` is the list of (origin, returns, misses) `submap.Submaps.insert` takes, `.match_cloud(i)` the [n][3] block the
scan matchers take; `.download(i)`, `hook_slot(...)` and `.last_counts()` are the test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import scan_match as scm
from . import submap as sm

ABI_VERSION = 1
EXPORTS = [
    "visfs_scan_filter_abi_version", "visfs_scan_filter_default_params", "visfs_scan_filter_create", "visfs_scan_filter_destroy",
    "visfs_scan_filter_last_error", "visfs_scan_filter_process", "visfs_scan_filter_num_scans", "visfs_scan_filter_record_of",
    "visfs_scan_filter_range_data", "visfs_scan_filter_match_cloud", "visfs_scan_filter_download", "visfs_scan_filter_hook_slot",
    "visfs_scan_filter_last_counts",
]
MAX_SCANS = 64
MAX_POINTS = 16384
MAX_SUBDIVISIONS = 16
MAX_TRACE = 16
MAX_VOXEL = (1 << 20) - 1
DROPPED, RETURN, MISS = 0, 1, 2
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class Params(C.Structure):
    _fields_ = [("pretreat", scm.PretreatParams), ("voxel_size", C.c_double), ("adaptive_max_length", C.c_double),
                ("adaptive_min_num_points", C.c_int32), ("adaptive_max_range", C.c_double)]


Scan = abi.ScanFilterScan
Record = abi.ScanFilterRecord

_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    lib.visfs_scan_filter_abi_version.restype = C.c_int
    lib.visfs_scan_filter_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_scan_filter_default_params.restype = None
    lib.visfs_scan_filter_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.visfs_scan_filter_create.restype = C.c_int
    lib.visfs_scan_filter_destroy.argtypes = [C.c_void_p]
    lib.visfs_scan_filter_destroy.restype = None
    lib.visfs_scan_filter_last_error.argtypes = [C.c_void_p]
    lib.visfs_scan_filter_last_error.restype = C.c_char_p
    lib.visfs_scan_filter_process.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, C.POINTER(Scan), C.POINTER(Record)]
    lib.visfs_scan_filter_process.restype = C.c_int
    lib.visfs_scan_filter_num_scans.argtypes = [C.c_void_p, _pi32]
    lib.visfs_scan_filter_num_scans.restype = C.c_int
    lib.visfs_scan_filter_record_of.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Record)]
    lib.visfs_scan_filter_record_of.restype = C.c_int
    lib.visfs_scan_filter_range_data.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(sm.RangeData), _pi32]
    lib.visfs_scan_filter_range_data.restype = C.c_int
    lib.visfs_scan_filter_match_cloud.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_pd), _pi32]
    lib.visfs_scan_filter_match_cloud.restype = C.c_int
    lib.visfs_scan_filter_download.argtypes = [C.c_void_p, C.c_int32, _pu8, _pu8, _pu8, _pd, _pi32, _pi32]
    lib.visfs_scan_filter_download.restype = C.c_int
    lib.visfs_scan_filter_hook_slot.argtypes = [_pi32, C.c_int32, C.c_int32, _pi32, _pi32]
    lib.visfs_scan_filter_hook_slot.restype = C.c_int
    lib.visfs_scan_filter_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_scan_filter_last_counts.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def default_params(**kw):
    """Keys of the parameter block, or of its `pretreat` member (num_subdivisions, min_range, max_range, missing_ray_length)."""
    p = Params()
    load().visfs_scan_filter_default_params(C.byref(p))
    own = {name for name, _ in Params._fields_}
    for k, v in kw.items():
        setattr(p if k in own else p.pretreat, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _copy(ptr, n):
    return np.array(np.ctypeslib.as_array(ptr, shape=(n, 3))) if n else np.zeros((0, 3))


class ScanFilter:
    """A visfs_scan_filter over the C ABI.  solver: a backend.Solver (device) or None (the host twin)."""

    def __init__(self, solver=None):
        self._lib = load()
        self.solver = solver
        h = C.c_void_p()
        rc = self._lib.visfs_scan_filter_create(solver.h if solver is not None else None, C.byref(h))
        self.status = rc
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_scan_filter_create failed with status {rc}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_scan_filter_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_scan_filter_last_error(self.h).decode()

    def process(self, scans, params=None, check_size=True):
        """scans: a list of (points[n][3], T_laser_to_camera (12 values or 3x4), origin[3]) or of bare point arrays (identity,
        zero origin).  (status, list of record dicts)."""
        p = params if params is not None else default_params()
        m = len(scans)
        arr = (Scan * max(m, 1))()
        keep = []
        for i, s in enumerate(scans):
            pts, T, o = s if isinstance(s, tuple) else (s, IDENTITY, (0.0, 0.0, 0.0))
            pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
            keep.append(pts)
            arr[i].T_laser_to_camera[:] = [float(v) for v in np.asarray(T, dtype=np.float64).reshape(12)]
            arr[i].origin[:] = [float(v) for v in o]
            arr[i].n = len(pts)
            arr[i].points_xyz = _ptr(pts, C.c_double)
        recs = (Record * max(m, 1))()
        rc = self._lib.visfs_scan_filter_process(self.h, C.byref(p), m, arr, recs)
        return rc, [recs[i].as_dict() for i in range(m)] if rc == abi.OK else []

    def num_scans(self):
        m = C.c_int32(-1)
        assert self._lib.visfs_scan_filter_num_scans(self.h, C.byref(m)) == abi.OK
        return m.value

    def record(self, scan):
        r = Record()
        rc = self._lib.visfs_scan_filter_record_of(self.h, scan, C.byref(r))
        return rc, r.as_dict()

    def range_data_struct(self, scan):
        """(status, ctypes array of visfs_range_data whose pointers lie in the object's download block, count)."""
        rd = (sm.RangeData * MAX_SUBDIVISIONS)()
        n = C.c_int32(0)
        rc = self._lib.visfs_scan_filter_range_data(self.h, scan, MAX_SUBDIVISIONS, rd, C.byref(n))
        return rc, rd, n.value

    def range_data(self, scan):
        """A list of (origin[3], returns[k][3], misses[m][3]) copies, as submap.Submaps.insert takes it."""
        rc, rd, n = self.range_data_struct(scan)
        assert rc == abi.OK, rc
        return [([float(v) for v in rd[i].origin], _copy(rd[i].returns, rd[i].n_returns), _copy(rd[i].misses, rd[i].n_misses))
                for i in range(n)]

    def match_cloud(self, scan):
        """A copy of the match cloud [n][3]."""
        xyz = _pd()
        n = C.c_int32(0)
        rc = self._lib.visfs_scan_filter_match_cloud(self.h, scan, C.byref(xyz), C.byref(n))
        assert rc == abi.OK, rc
        return _copy(xyz, n.value)

    def download(self, scan, n):
        """The hook: dict(cls[n], sub[n], kept[n] uint8; trace: list of (length, count))."""
        cls, sub, kept = (np.zeros(max(n, 1), dtype=np.uint8) for _ in range(3))
        tl = np.zeros(MAX_TRACE)
        tc = np.zeros(MAX_TRACE, dtype=np.int32)
        nt = C.c_int32(-1)
        rc = self._lib.visfs_scan_filter_download(self.h, scan, _ptr(cls, C.c_uint8), _ptr(sub, C.c_uint8), _ptr(kept, C.c_uint8),
                                                  _ptr(tl, C.c_double), _ptr(tc, C.c_int32), C.byref(nt))
        assert rc == abi.OK, rc
        return {"cls": cls[:n], "sub": sub[:n], "kept": kept[:n], "trace": [(float(tl[k]), int(tc[k])) for k in range(nt.value)]}

    def last_counts(self):
        v = [C.c_int32(-1) for _ in range(3)]
        rc = self._lib.visfs_scan_filter_last_counts(self.h, *[C.byref(x) for x in v])
        assert rc == abi.OK, rc
        return tuple(x.value for x in v)


def hook_slot(voxel, count, list_id=0):
    """(status, slots of a pass over `count` points, slot the voxel hashes to)."""
    v = np.ascontiguousarray(np.asarray(voxel, dtype=np.int32).reshape(3))
    slots, slot = C.c_int32(-1), C.c_int32(-1)
    rc = load().visfs_scan_filter_hook_slot(_ptr(v, C.c_int32), list_id, count, C.byref(slots), C.byref(slot))
    return rc, slots.value, slot.value
