"""ctypes binding of the branch-and-bound scan matcher (include/visfs_scan_fast.h, in libvisfs_ba_hip.so) — plumbing only.

`ScanStack.from_submaps(submaps, index, depth)` freezes a sub-map of a `submap.Submaps` object of either flavour (device
grids: a device stack searched by HIP kernels; host restatement: the one-core twin); `ScanStack.from_grid(cells, limits,
depth, solver=None)` builds one from a downloaded grid.  `.match(guess, points, params)` searches it; `.download_level(h)`
and `.match_download()` are the test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import scan_match as scm
from . import submap as sm

ABI_VERSION = 1
EXPORTS = [
    "visfs_scan_fast_abi_version", "visfs_scan_stack_default_params", "visfs_scan_stack_create", "visfs_scan_stack_create_from_grid",
    "visfs_scan_stack_destroy", "visfs_scan_stack_last_error", "visfs_scan_stack_describe", "visfs_scan_stack_match",
    "visfs_scan_stack_download_level", "visfs_scan_stack_match_download",
]
MAX_DEPTH = 16
MAX_BYTES = 1 << 30
MAX_POINTS = 16384
MAX_LINEAR = 512
MAX_SCANS = 1025
MAX_CELLS = 1 << 22
MAX_TOP_NODES = 1 << 22
MAX_FRONTIER = 1 << 26


class Params(C.Structure):
    _fields_ = [("linear_search_window", C.c_double), ("angular_search_window", C.c_double), ("min_score", C.c_double),
                ("frontier_capacity", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("match", scm.Result), ("depth_used", C.c_int32)]

    def as_dict(self):
        d = self.match.as_dict()
        d["depth_used"] = self.depth_used
        return d


class Info(C.Structure):
    _fields_ = [("resolution", C.c_double), ("max_x", C.c_double), ("max_y", C.c_double), ("num_x_cells", C.c_int32),
                ("num_y_cells", C.c_int32), ("depth", C.c_int32), ("device", C.c_int32), ("bytes", C.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu16 = C.POINTER(C.c_uint16)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    lib.visfs_scan_fast_abi_version.restype = C.c_int
    lib.visfs_scan_stack_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_scan_stack_default_params.restype = None
    lib.visfs_scan_stack_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_scan_stack_create.restype = C.c_int
    lib.visfs_scan_stack_create_from_grid.argtypes = [C.c_void_p, C.POINTER(sm.Info), _pu16, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_scan_stack_create_from_grid.restype = C.c_int
    lib.visfs_scan_stack_destroy.argtypes = [C.c_void_p]
    lib.visfs_scan_stack_destroy.restype = None
    lib.visfs_scan_stack_last_error.argtypes = [C.c_void_p]
    lib.visfs_scan_stack_last_error.restype = C.c_char_p
    lib.visfs_scan_stack_describe.argtypes = [C.c_void_p, C.POINTER(Info)]
    lib.visfs_scan_stack_describe.restype = C.c_int
    lib.visfs_scan_stack_match.argtypes = [C.c_void_p, C.POINTER(Params), _pd, C.c_int32, _pd, C.POINTER(Result)]
    lib.visfs_scan_stack_match.restype = C.c_int
    lib.visfs_scan_stack_download_level.argtypes = [C.c_void_p, C.c_int32, C.c_int64, _pu16, _pi32]
    lib.visfs_scan_stack_download_level.restype = C.c_int
    lib.visfs_scan_stack_match_download.argtypes = [C.c_void_p, _pi32, _pi32, _pi32, C.c_int64, _pi32, C.c_int64, _pi32]
    lib.visfs_scan_stack_match_download.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_scan_stack_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class ScanStack:
    """A visfs_scan_stack over the C ABI.  `status` is the constructor's return code; `h` is None when it failed."""

    def __init__(self, handle, status, solver=None):
        self._lib = load()
        self.h = handle
        self.status = status
        self.solver = solver                  # a device stack runs on its solver's stream: keep it alive

    @classmethod
    def from_submaps(cls, submaps, index=0, depth=7):
        lib = load()
        h = C.c_void_p()
        rc = lib.visfs_scan_stack_create(submaps.h, index, depth, C.byref(h))
        return cls(h if rc == abi.OK else None, rc, submaps.solver)

    @classmethod
    def from_grid(cls, cells, limits, depth=7, solver=None):
        """cells [ny][nx] uint16 as Submaps.download hands them out; limits: a dict as Submaps.describe gives it."""
        lib = load()
        info = sm.Info()
        for k in ("resolution", "max_x", "max_y", "num_x_cells", "num_y_cells"):
            setattr(info, k, limits[k])
        c = np.ascontiguousarray(cells, dtype=np.uint16)
        assert c.size == info.num_x_cells * info.num_y_cells
        h = C.c_void_p()
        rc = lib.visfs_scan_stack_create_from_grid(solver.h if solver is not None else None, C.byref(info), _ptr(c, C.c_uint16), depth, C.byref(h))
        return cls(h if rc == abi.OK else None, rc, solver)

    def close(self):
        if self.h:
            self._lib.visfs_scan_stack_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_scan_stack_last_error(self.h).decode()

    def describe(self):
        info = Info()
        rc = self._lib.visfs_scan_stack_describe(self.h, C.byref(info))
        assert rc == abi.OK, rc
        return info.as_dict()

    def match(self, guess, points, params=None):
        """visfs_scan_stack_match: (status, result dict).  points [n][3] in the robot frame, guess (x, y, yaw)."""
        p = params if params is not None else default_params()
        g = np.ascontiguousarray(np.asarray(guess, dtype=np.float64).reshape(3))
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        r = Result()
        rc = self._lib.visfs_scan_stack_match(self.h, C.byref(p), _ptr(g, C.c_double), len(pts), _ptr(pts, C.c_double), C.byref(r))
        return rc, r.as_dict()

    def download_level(self, h):
        """Level h as stored: (array [height][width] uint16, low-side extension e): x in [-e, nx), y in [-e, ny)."""
        dims = np.zeros(4, dtype=np.int32)
        rc = self._lib.visfs_scan_stack_download_level(self.h, h, 0, None, _ptr(dims, C.c_int32))
        assert rc == abi.OK, (rc, self.last_error())
        out = np.zeros((int(dims[1]), int(dims[0])), dtype=np.uint16)
        rc = self._lib.visfs_scan_stack_download_level(self.h, h, out.size, _ptr(out, C.c_uint16), _ptr(dims, C.c_int32))
        assert rc == abi.OK, (rc, self.last_error())
        return out, int(dims[2])

    def match_download(self):
        """The hook after a match: a dict with S, L, n, H, B, scored and kept (lists over the levels 0 .. H), bounds
        [S][top nodes per scan] int32 and survivors [m][2] int32 (index, Q) sorted by index; None before any match."""
        hdr = np.zeros(8, dtype=np.int32)
        scored = np.zeros(16, dtype=np.int32)
        kept = np.zeros(16, dtype=np.int32)
        rc = self._lib.visfs_scan_stack_match_download(self.h, _ptr(hdr, C.c_int32), _ptr(scored, C.c_int32), _ptr(kept, C.c_int32), 0, None, 0, None)
        assert rc == abi.OK, (rc, self.last_error())
        S, L, n, H, per, m, B = (int(v) for v in hdr[:7])
        if S == 0:
            return None
        bounds = np.zeros((S, per), dtype=np.int32)
        surv = np.zeros((m, 2), dtype=np.int32)
        rc = self._lib.visfs_scan_stack_match_download(self.h, _ptr(hdr, C.c_int32), _ptr(scored, C.c_int32), _ptr(kept, C.c_int32),
                                                       bounds.size, _ptr(bounds, C.c_int32), m, _ptr(surv, C.c_int32))
        assert rc == abi.OK, (rc, self.last_error())
        return dict(S=S, L=L, n=n, H=H, B=B, scored=scored[:H + 1].tolist(), kept=kept[:H + 1].tolist(), bounds=bounds, survivors=surv)


# the method next to submap.Submaps
sm.Submaps.freeze = lambda self, index=0, depth=7: ScanStack.from_submaps(self, index, depth)
