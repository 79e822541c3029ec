"""ctypes binding of the pose graph's covariances (include/visfs_pose_graph_cov.h, in libvisfs_ba_hip.so) — plumbing only.

`covariance(graph, poses, fixed, edges, queries, **params)` runs visfs_pose_graph_covariance on a `pose_graph.PoseGraph` (device
or host twin) and returns (status, dict) with joint [Q][6][6], relative [Q][3][3] and the record's fields.  `columns`, `plan` and
`last_counts` are the test hooks, `search_window` the host helper that turns a relative covariance into the two windows of
visfs_scan_group_match_refine.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import pose_graph as pg

ABI_VERSION = 1
EXPORTS = [
    "visfs_pose_graph_cov_abi_version", "visfs_pose_graph_cov_default_params", "visfs_pose_graph_covariance",
    "visfs_pose_graph_cov_download_columns", "visfs_pose_graph_cov_plan", "visfs_pose_graph_cov_last_counts",
    "visfs_pose_graph_cov_search_window",
]
MAX_QUERIES = 1024
MAX_SOURCES = 64
ERR_SINGULAR = 10


class Params(C.Structure):
    _fields_ = [("pcg_tolerance", C.c_double), ("max_pcg_iterations", C.c_int32), ("preconditioner", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("sources", C.c_int32), ("columns", C.c_int32), ("pcg_iterations_max", C.c_int32),
                ("pcg_iterations_total", C.c_int32), ("unconverged_columns", C.c_int32), ("free_vertices", C.c_int32),
                ("reserved", C.c_int32), ("cost", C.c_double)]


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    pg.load()
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_pose_graph_cov_abi_version.restype = C.c_int
    lib.visfs_pose_graph_cov_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_pose_graph_cov_default_params.restype = None
    lib.visfs_pose_graph_covariance.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, _pd, _pu8, C.c_int32, C.POINTER(pg.Edge), C.c_int32, _pi32,
                                                _pd, _pd, C.POINTER(Result)]
    lib.visfs_pose_graph_covariance.restype = C.c_int
    lib.visfs_pose_graph_cov_download_columns.argtypes = [C.c_void_p, C.c_int32, _pd, _pi32]
    lib.visfs_pose_graph_cov_download_columns.restype = C.c_int
    lib.visfs_pose_graph_cov_plan.argtypes = [C.c_int32, _pu8, C.c_int32, C.POINTER(pg.Edge), C.c_int32, _pi32, _pi32, _pi32, _pi32]
    lib.visfs_pose_graph_cov_plan.restype = C.c_int
    lib.visfs_pose_graph_cov_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_pose_graph_cov_last_counts.restype = C.c_int
    lib.visfs_pose_graph_cov_search_window.argtypes = [_pd, C.c_double, _pd, _pd]
    lib.visfs_pose_graph_cov_search_window.restype = C.c_int
    if lib.visfs_pose_graph_cov_abi_version() != ABI_VERSION:
        raise backend.BackendError("visfs_pose_graph_cov ABI version mismatch")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_pose_graph_cov_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _queries(queries):
    return np.ascontiguousarray(np.asarray(queries, dtype=np.int32).reshape(-1, 2))


def covariance(graph, poses, fixed, edges, queries, params=None, **kw):
    """(status, dict): joint [Q][6][6], relative [Q][3][3], the record's fields and its `bytes`."""
    lib = load()
    prm = params if params is not None else default_params(**kw)
    p, f, e, ne = graph._graph(poses, fixed, edges)
    q = _queries(queries)
    Q = len(q)
    joint, relative, r = np.zeros((max(Q, 1), 6, 6)), np.zeros((max(Q, 1), 3, 3)), Result()
    rc = lib.visfs_pose_graph_covariance(graph.h, C.byref(prm), len(p), _ptr(p, C.c_double), _ptr(f, C.c_uint8), ne, e, Q, _ptr(q, C.c_int32),
                                         _ptr(joint, C.c_double), _ptr(relative, C.c_double), C.byref(r))
    d = {name: getattr(r, name) for name, _ in Result._fields_}
    d.update(joint=joint[:Q], relative=relative[:Q], bytes=bytes(r))
    return rc, d


def columns(graph, source, rows):
    """(status, columns [3][rows][3], iterations [3]) of source `source` of the graph's last successful covariance call."""
    out, it = np.zeros((3, max(rows, 1), 3)), np.zeros(3, np.int32)
    rc = load().visfs_pose_graph_cov_download_columns(graph.h, source, _ptr(out, C.c_double), _ptr(it, C.c_int32))
    return rc, out[:, :rows], it


def plan(fixed, edges, queries):
    """visfs_pose_graph_cov_plan: (status, dict) with sources (vertices) and query_sources [Q][2] (-1: a fixed vertex)."""
    f = np.ascontiguousarray(np.asarray(fixed).astype(np.uint8).reshape(-1))
    q = _queries(queries)
    Q = len(q)
    n, src, qs = C.c_int32(-1), np.zeros(MAX_SOURCES, np.int32), np.full((max(Q, 1), 2), -2, np.int32)
    rc = load().visfs_pose_graph_cov_plan(len(f), _ptr(f, C.c_uint8), len(edges), pg.make_edges(edges), Q, _ptr(q, C.c_int32), C.byref(n),
                                          _ptr(src, C.c_int32), _ptr(qs, C.c_int32))
    if rc != abi.OK:
        return rc, None
    return rc, {"sources": src[:n.value].tolist(), "query_sources": qs[:Q]}


def last_counts(graph):
    a, b, c = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    rc = load().visfs_pose_graph_cov_last_counts(graph.h, C.byref(a), C.byref(b), C.byref(c))
    assert rc == abi.OK, rc
    return a.value, b.value, c.value


def search_window(relative, sigmas):
    """visfs_pose_graph_cov_search_window: (status, linear, angular)."""
    r = np.ascontiguousarray(np.asarray(relative, dtype=np.float64).reshape(9))
    lin, ang = C.c_double(), C.c_double()
    rc = load().visfs_pose_graph_cov_search_window(_ptr(r, C.c_double), float(sigmas), C.byref(lin), C.byref(ang))
    return rc, lin.value, ang.value
