"""ctypes binding of the correlative scan matcher (include/visfs_scan_match.h, in libvisfs_ba_hip.so) — plumbing only.

`match(submaps, guess, points)` searches about the guess on a `submap.Submaps` object of either flavour (device grids: HIP
kernels; host restatement: the one-core twin); `download(submaps)` is the test hook; `pretreat(...)` is
Estimator::laserPretreatment on the host.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import submap as sm

ABI_VERSION = 1
EXPORTS = [
    "visfs_scan_match_abi_version", "visfs_scan_match_default_params", "visfs_scan_match", "visfs_scan_match_download",
    "visfs_scan_pretreat_default_params", "visfs_scan_pretreat",
]
MAX_POINTS = 16384
MAX_LINEAR = 32
MAX_SCANS = 1025
MAX_CANDIDATES = 1 << 21


class Params(C.Structure):
    _fields_ = [("linear_search_window", C.c_double), ("angular_search_window", C.c_double),
                ("translation_delta_cost_weight", C.c_double), ("rotation_delta_cost_weight", C.c_double)]


class Result(C.Structure):
    _fields_ = [("matched", C.c_int32), ("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double), ("score", C.c_double),
                ("sum", C.c_int64), ("scan_index", C.c_int32), ("x_offset", C.c_int32), ("y_offset", C.c_int32),
                ("num_scans", C.c_int32), ("num_linear", C.c_int32), ("angular_step", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PretreatParams(C.Structure):
    _fields_ = [("num_subdivisions", C.c_int32), ("min_range", C.c_double), ("max_range", C.c_double),
                ("missing_ray_length", C.c_double)]


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    lib.visfs_scan_match_abi_version.restype = C.c_int
    lib.visfs_scan_match_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_scan_match_default_params.restype = None
    lib.visfs_scan_match.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Params), _pd, C.c_int32, _pd, C.POINTER(Result)]
    lib.visfs_scan_match.restype = C.c_int
    lib.visfs_scan_match_download.argtypes = [C.c_void_p, C.c_int64, _pi32, _pd, _pi32]
    lib.visfs_scan_match_download.restype = C.c_int
    lib.visfs_scan_pretreat_default_params.argtypes = [C.POINTER(PretreatParams)]
    lib.visfs_scan_pretreat_default_params.restype = None
    lib.visfs_scan_pretreat.argtypes = [C.POINTER(PretreatParams), _pd, _pd, C.c_int32, _pd, _pd, _pd, C.POINTER(sm.RangeData), _pi32]
    lib.visfs_scan_pretreat.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_scan_match_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def default_pretreat_params(**kw):
    p = PretreatParams()
    load().visfs_scan_pretreat_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def match(submaps, guess, points, params=None, index=0):
    """visfs_scan_match on a submap.Submaps: (status, result dict).  points [n][3] in the robot frame, guess (x, y, yaw)."""
    lib = load()
    p = params if params is not None else default_params()
    g = np.ascontiguousarray(np.asarray(guess, dtype=np.float64).reshape(3))
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    r = Result()
    rc = lib.visfs_scan_match(submaps.h, index, C.byref(p), _ptr(g, C.c_double), len(pts), _ptr(pts, C.c_double), C.byref(r))
    submaps._scan_last = (r.num_scans, r.num_linear, len(pts)) if rc == abi.OK else getattr(submaps, "_scan_last", (0, 0, 0))
    return rc, r.as_dict()


def download(submaps):
    """The hook after a match: (sums [S][L][L] int32, scores [S][L][L] float64, cells [S][n][2] int32)."""
    lib = load()
    S, nl, n = getattr(submaps, "_scan_last", (0, 0, 0))
    L = 2 * nl + 1 if S else 0
    sums = np.zeros((S, L, L), dtype=np.int32)
    scores = np.zeros((S, L, L), dtype=np.float64)
    cells = np.zeros((S, n, 2), dtype=np.int32)
    cap = max(S * L * L, S * n)
    rc = lib.visfs_scan_match_download(submaps.h, cap, _ptr(sums, C.c_int32), _ptr(scores, C.c_double), _ptr(cells, C.c_int32))
    assert rc == abi.OK, (rc, submaps.last_error())
    return sums, scores, cells


def pretreat(points, T_laser_to_camera, origin=(0.0, 0.0, 0.0), params=None):
    """visfs_scan_pretreat: a list of (origin[3], returns[k][3], misses[m][3]), as submap.Submaps.insert takes it."""
    lib = load()
    p = params if params is not None else default_pretreat_params()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    T = np.ascontiguousarray(np.asarray(T_laser_to_camera, dtype=np.float64).reshape(12))
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    n = len(pts)
    ret = np.zeros((max(n, 1), 3), dtype=np.float64)
    mis = np.zeros((max(n, 1), 3), dtype=np.float64)
    rd = (sm.RangeData * max(p.num_subdivisions, 1))()
    cnt = C.c_int32()
    rc = lib.visfs_scan_pretreat(C.byref(p), _ptr(T, C.c_double), _ptr(o, C.c_double), n, _ptr(pts, C.c_double), _ptr(ret, C.c_double),
                                 _ptr(mis, C.c_double), rd, C.byref(cnt))
    if rc != abi.OK:
        raise backend.BackendError(f"visfs_scan_pretreat failed with status {rc}")
    out = []
    for i in range(cnt.value):
        r = np.array(np.ctypeslib.as_array(rd[i].returns, shape=(rd[i].n_returns, 3))) if rd[i].n_returns else np.zeros((0, 3))
        m = np.array(np.ctypeslib.as_array(rd[i].misses, shape=(rd[i].n_misses, 3))) if rd[i].n_misses else np.zeros((0, 3))
        out.append(([float(v) for v in rd[i].origin], r, m))
    return out


# the methods next to submap.Submaps
sm.Submaps.match = lambda self, guess, points, params=None, index=0: match(self, guess, points, params, index)
sm.Submaps.match_download = lambda self: download(self)
