"""ctypes binding of the scan refinement (include/visfs_scan_refine.h, in libvisfs_ba_hip.so) — plumbing only.

`refine_submaps(submaps, index, initial, target, points, **params)` refines a pose against a live sub-map of a `submap.Submaps`
of either flavour, `refine_stack(stack, initial, target, points, **params)` against level 0 of a `scan_fast.ScanStack`, and
`group_match_refine(group, guesses, points, match_params, **params)` matches one scan against a `scan_group.ScanStackGroup`
and refines every matched member in the same call.  The three are also methods: `Submaps.refine`, `ScanStack.refine`,
`ScanStackGroup.match_refine`.  The `*_trace` functions are the test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import scan_fast as sf
from . import scan_group as sg
from . import submap as sm

ABI_VERSION = 1
EXPORTS = [
    "visfs_scan_refine_abi_version", "visfs_scan_refine_default_params", "visfs_scan_refine", "visfs_scan_stack_refine",
    "visfs_scan_group_match_refine", "visfs_scan_refine_download", "visfs_scan_stack_refine_download",
    "visfs_scan_group_refine_download",
]
LANES = 256
MAX_POINTS = 16384
MAX_ITERATIONS = 50
MAX_TRIALS = 500
TERMINATION = {0: "iterations", 1: "no_progress", 2: "tolerance"}
TRACE_FIELDS = ("cost", "lambda", "accepted", "x", "y", "delta")


class Params(C.Structure):
    _fields_ = [("occupied_space_weight", C.c_double), ("translation_weight", C.c_double), ("rotation_weight", C.c_double),
                ("function_tolerance", C.c_double), ("max_iterations", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("refined", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32),
                ("termination", C.c_int32), ("reserved", C.c_int32), ("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("information", C.c_double * 9)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "information"}
        d["information"] = np.array(self.information[:], dtype=np.float64).reshape(3, 3)
        d["bytes"] = bytes(self)
        return d


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    sg.load()
    lib = backend.load_library()
    lib.visfs_scan_refine_abi_version.restype = C.c_int
    lib.visfs_scan_refine_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_scan_refine_default_params.restype = None
    lib.visfs_scan_refine.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Params), _pd, _pd, C.c_int32, _pd, C.POINTER(Result)]
    lib.visfs_scan_refine.restype = C.c_int
    lib.visfs_scan_stack_refine.argtypes = [C.c_void_p, C.POINTER(Params), _pd, _pd, C.c_int32, _pd, C.POINTER(Result)]
    lib.visfs_scan_stack_refine.restype = C.c_int
    lib.visfs_scan_group_match_refine.argtypes = [C.c_void_p, C.POINTER(sf.Params), C.POINTER(Params), _pd, C.c_int32, _pd,
                                                  C.POINTER(sf.Result), _pi32, _pi32, C.POINTER(Result)]
    lib.visfs_scan_group_match_refine.restype = C.c_int
    lib.visfs_scan_refine_download.argtypes = [C.c_void_p, C.c_int32, _pd, _pi32]
    lib.visfs_scan_refine_download.restype = C.c_int
    lib.visfs_scan_stack_refine_download.argtypes = [C.c_void_p, C.c_int32, _pd, _pi32]
    lib.visfs_scan_stack_refine_download.restype = C.c_int
    lib.visfs_scan_group_refine_download.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _pd, _pi32]
    lib.visfs_scan_group_refine_download.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_scan_refine_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _args(initial, target, points):
    a = np.ascontiguousarray(np.asarray(initial, dtype=np.float64).reshape(3))
    t = np.ascontiguousarray(np.asarray(target, dtype=np.float64).reshape(2))
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    return a, t, pts


def refine_submaps(submaps, index, initial, target, points, params=None, **kw):
    """visfs_scan_refine: (status, result dict)."""
    p = params if params is not None else default_params(**kw)
    a, t, pts = _args(initial, target, points)
    r = Result()
    rc = load().visfs_scan_refine(submaps.h, index, C.byref(p), _ptr(a, C.c_double), _ptr(t, C.c_double), len(pts), _ptr(pts, C.c_double), C.byref(r))
    return rc, r.as_dict()


def refine_stack(stack, initial, target, points, params=None, **kw):
    """visfs_scan_stack_refine: (status, result dict)."""
    p = params if params is not None else default_params(**kw)
    a, t, pts = _args(initial, target, points)
    r = Result()
    rc = load().visfs_scan_stack_refine(stack.h, C.byref(p), _ptr(a, C.c_double), _ptr(t, C.c_double), len(pts), _ptr(pts, C.c_double), C.byref(r))
    return rc, r.as_dict()


def group_match_refine(group, guesses, points, match_params=None, params=None, **kw):
    """visfs_scan_group_match_refine: (results, status, best_member, refined) with the first three as ScanStackGroup.match gives
    them and refined[i] member i's refinement dict.  `group.rc` holds the return code; when it is not OK the four are None."""
    lib = load()
    mp = match_params if match_params is not None else sf.default_params()
    p = params if params is not None else default_params(**kw)
    m = len(group.stacks)
    g = np.asarray(guesses, dtype=np.float64)
    if g.size == 3:
        g = np.tile(g.reshape(1, 3), (m, 1))
    g = np.ascontiguousarray(g.reshape(m, 3))
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    res = (sf.Result * m)()
    ref = (Result * m)()
    status = np.full(m, -1, dtype=np.int32)
    best = C.c_int32(-2)
    group.rc = lib.visfs_scan_group_match_refine(group.h, C.byref(mp), C.byref(p), _ptr(g, C.c_double), len(pts), _ptr(pts, C.c_double), res,
                                                 _ptr(status, C.c_int32), C.byref(best), ref)
    if group.rc != abi.OK:
        return None, None, None, None
    st = [int(v) for v in status]
    return ([res[i].as_dict() if st[i] == abi.OK else None for i in range(m)], st, int(best.value), [ref[i].as_dict() for i in range(m)])


def _trace(call):
    n = C.c_int32(-1)
    rc = call(0, None, C.byref(n))
    assert rc == abi.OK, rc
    out = np.zeros((max(n.value, 1), len(TRACE_FIELDS)), dtype=np.float64)
    rc = call(n.value, _ptr(out, C.c_double), C.byref(n))
    assert rc == abi.OK, rc
    return out[:n.value]


def submaps_trace(submaps):
    """The trials of the last successful refinement on the sub-maps: [trials][6] in the order of TRACE_FIELDS."""
    lib = load()
    return _trace(lambda cap, p, n: lib.visfs_scan_refine_download(submaps.h, cap, p, n))


def stack_trace(stack):
    lib = load()
    return _trace(lambda cap, p, n: lib.visfs_scan_stack_refine_download(stack.h, cap, p, n))


def group_trace(group, member):
    lib = load()
    return _trace(lambda cap, p, n: lib.visfs_scan_group_refine_download(group.h, member, cap, p, n))


# the methods next to the objects they refine on
sm.Submaps.refine = lambda self, initial, target, points, index=0, params=None, **kw: refine_submaps(self, index, initial, target, points, params, **kw)
sf.ScanStack.refine = lambda self, initial, target, points, params=None, **kw: refine_stack(self, initial, target, points, params, **kw)
sg.ScanStackGroup.match_refine = lambda self, guesses, points, match_params=None, params=None, **kw: group_match_refine(self, guesses, points, match_params, params, **kw)
