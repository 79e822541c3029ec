"""ctypes binding of the 2-D pose graph (include/visfs_pose_graph.h, in libvisfs_ba_hip.so) — plumbing only.

`PoseGraph(solver=None, max_vertices=4096, max_edges=65536)` is one `visfs_pose_graph`: on the device of a `backend.Solver`, or
the one-core host twin without one.  `optimize(poses, fixed, edges, **params)` returns (status, result dict); `edges` is a list of
(i, j, z[3], information[3][3], huber_delta) or an array of `Edge`.  `linearize`, `precondition`, `trace` and `last_counts` are
the test hooks; `edge_from_refine` is the host helper that turns a scan refinement into an edge.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import scan_refine as sr

ABI_VERSION = 1
EXPORTS = [
    "visfs_pose_graph_abi_version", "visfs_pose_graph_default_params", "visfs_pose_graph_create", "visfs_pose_graph_destroy",
    "visfs_pose_graph_last_error", "visfs_pose_graph_optimize", "visfs_pose_graph_download_trace", "visfs_pose_graph_linearize",
    "visfs_pose_graph_precondition", "visfs_pose_graph_plan", "visfs_pose_graph_last_counts", "visfs_pose_graph_edge_from_refine",
]
LANES = 1024
MAX_VERTICES = 4096
MAX_EDGES = 65536
MAX_ITERATIONS = 50
MAX_TRIALS = 500
MAX_ROTATION = 1.0
TERMINATION = {0: "iterations", 1: "no_progress", 2: "tolerance", 3: "rotation_bound", 4: "pcg_budget"}
TRACE_FIELDS = ("cost", "lambda", "accepted", "pcg_iterations")
ERR_SINGULAR = 10


class Params(C.Structure):
    _fields_ = [("function_tolerance", C.c_double), ("pcg_tolerance", C.c_double), ("max_iterations", C.c_int32),
                ("max_pcg_iterations", C.c_int32), ("pcg_budget", C.c_int32), ("preconditioner", C.c_int32)]


class Edge(C.Structure):
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("z", C.c_double * 3), ("information", C.c_double * 9), ("huber_delta", C.c_double)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("trials", C.c_int32), ("termination", C.c_int32),
                ("pcg_iterations", C.c_int32), ("free_vertices", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    sr.load()
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    graph = [C.c_int32, _pd, _pu8, C.c_int32, C.POINTER(Edge)]
    lib.visfs_pose_graph_abi_version.restype = C.c_int
    lib.visfs_pose_graph_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_pose_graph_default_params.restype = None
    lib.visfs_pose_graph_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_pose_graph_create.restype = C.c_int
    lib.visfs_pose_graph_destroy.argtypes = [C.c_void_p]
    lib.visfs_pose_graph_destroy.restype = None
    lib.visfs_pose_graph_last_error.argtypes = [C.c_void_p]
    lib.visfs_pose_graph_last_error.restype = C.c_char_p
    lib.visfs_pose_graph_optimize.argtypes = [C.c_void_p, C.POINTER(Params)] + graph + [_pd, _pd, C.POINTER(Result)]
    lib.visfs_pose_graph_optimize.restype = C.c_int
    lib.visfs_pose_graph_download_trace.argtypes = [C.c_void_p, C.c_int32, _pd, _pi32]
    lib.visfs_pose_graph_download_trace.restype = C.c_int
    lib.visfs_pose_graph_linearize.argtypes = [C.c_void_p] + graph + [_pi32, _pd, _pd, _pd, _pd, _pd, _pd]
    lib.visfs_pose_graph_linearize.restype = C.c_int
    lib.visfs_pose_graph_precondition.argtypes = [C.c_void_p, C.c_int32, C.c_double] + graph + [_pd, _pd]
    lib.visfs_pose_graph_precondition.restype = C.c_int
    lib.visfs_pose_graph_plan.argtypes = [C.c_int32, _pu8, C.c_int32, C.POINTER(Edge), _pi32, _pi32, _pi32, _pi32, _pi32, _pi32]
    lib.visfs_pose_graph_plan.restype = C.c_int
    lib.visfs_pose_graph_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_pose_graph_last_counts.restype = C.c_int
    lib.visfs_pose_graph_edge_from_refine.argtypes = [_pd, C.POINTER(sr.Result), _pd, _pd]
    lib.visfs_pose_graph_edge_from_refine.restype = C.c_int
    if lib.visfs_pose_graph_abi_version() != ABI_VERSION:
        raise backend.BackendError("visfs_pose_graph ABI version mismatch")
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_pose_graph_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def make_edges(edges):
    """A ctypes array of Edge from (i, j, z, information[, huber_delta]) tuples (or the array itself)."""
    if isinstance(edges, C.Array):
        return edges
    arr = (Edge * max(len(edges), 1))()
    for k, e in enumerate(edges):
        arr[k].i, arr[k].j = int(e[0]), int(e[1])
        arr[k].z[:] = [float(v) for v in e[2]]
        arr[k].information[:] = [float(v) for v in np.asarray(e[3], dtype=np.float64).reshape(9)]
        arr[k].huber_delta = float(e[4]) if len(e) > 4 else 0.0
    return arr


def edge_from_refine(anchor_pose, refined):
    """visfs_pose_graph_edge_from_refine: (status, z[3], information[3][3]); `refined` is a scan_refine result dict or Result."""
    r = refined if isinstance(refined, sr.Result) else sr.Result.from_buffer_copy(refined["bytes"])
    a = np.ascontiguousarray(np.asarray(anchor_pose, dtype=np.float64).reshape(3))
    z, W = np.zeros(3), np.zeros((3, 3))
    rc = load().visfs_pose_graph_edge_from_refine(_ptr(a, C.c_double), C.byref(r), _ptr(z, C.c_double), _ptr(W, C.c_double))
    return rc, z, W


def plan(fixed, edges):
    """visfs_pose_graph_plan: (status, dict) with rows, row_of [N], inc and chain as lists (one per row) of (edge, flag)."""
    f = np.ascontiguousarray(np.asarray(fixed).astype(np.uint8).reshape(-1))
    N, E = len(f), len(edges)
    row_of, inc_ptr, chain_ptr = np.zeros(N, np.int32), np.zeros(N + 1, np.int32), np.zeros(N + 1, np.int32)
    inc, chain, n = np.zeros(2 * max(E, 1), np.int32), np.zeros(max(E, 1), np.int32), C.c_int32(-1)
    rc = load().visfs_pose_graph_plan(N, _ptr(f, C.c_uint8), E, make_edges(edges), C.byref(n), _ptr(row_of, C.c_int32), _ptr(inc_ptr, C.c_int32),
                                      _ptr(inc, C.c_int32), _ptr(chain_ptr, C.c_int32), _ptr(chain, C.c_int32))
    if rc != abi.OK:
        return rc, None
    rows = n.value

    def lists(ptr, codes):
        return [[(int(c) >> 1, int(c) & 1) for c in codes[ptr[r]:ptr[r + 1]]] for r in range(rows)]

    return rc, {"rows": rows, "row_of": row_of.tolist(), "inc": lists(inc_ptr, inc), "chain": lists(chain_ptr, chain)}


class PoseGraph:
    def __init__(self, solver=None, max_vertices=MAX_VERTICES, max_edges=MAX_EDGES):
        self._lib = load()
        self.solver = solver
        h = C.c_void_p()
        rc = self._lib.visfs_pose_graph_create(solver.h if solver is not None else None, max_vertices, max_edges, C.byref(h))
        self.h = None
        if rc != abi.OK:
            raise backend.BackendError(f"visfs_pose_graph_create failed with status {rc}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_pose_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_pose_graph_last_error(self.h).decode()

    @staticmethod
    def _graph(poses, fixed, edges):
        p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        f = np.ascontiguousarray(np.asarray(fixed).astype(np.uint8).reshape(-1))
        assert len(f) == len(p)
        e = make_edges(edges)
        n_edges = len(edges)
        return p, f, e, n_edges

    def optimize(self, poses, fixed, edges, params=None, **kw):
        """(status, dict): poses [N][3], chi2 [E], the record's fields, `bytes` of the record."""
        prm = params if params is not None else default_params(**kw)
        p, f, e, ne = self._graph(poses, fixed, edges)
        out, chi2, r = np.zeros_like(p), np.zeros(max(ne, 1)), Result()
        rc = self._lib.visfs_pose_graph_optimize(self.h, C.byref(prm), len(p), _ptr(p, C.c_double), _ptr(f, C.c_uint8), ne, e,
                                                 _ptr(out, C.c_double), _ptr(chi2, C.c_double), C.byref(r))
        d = {name: getattr(r, name) for name, _ in Result._fields_}
        d.update(poses=out, chi2=chi2[:ne], bytes=bytes(r))
        return rc, d

    def trace(self):
        """The trials of the last successful optimize: [trials][4] in the order of TRACE_FIELDS."""
        n = C.c_int32(-1)
        rc = self._lib.visfs_pose_graph_download_trace(self.h, 0, None, C.byref(n))
        assert rc == abi.OK, rc
        out = np.zeros((max(n.value, 1), len(TRACE_FIELDS)))
        rc = self._lib.visfs_pose_graph_download_trace(self.h, n.value, _ptr(out, C.c_double), C.byref(n))
        assert rc == abi.OK, rc
        return out[:n.value]

    def linearize(self, poses, fixed, edges):
        """(status, dict): edge_blocks [E][3][3][3] (H_ii, H_ij, H_jj), g [n][3], D [n][3][3], C [n][3][3], cost, chi2 [E]."""
        p, f, e, ne = self._graph(poses, fixed, edges)
        n = int(np.sum(f == 0))
        eb, g, D, Cb = np.zeros((max(ne, 1), 3, 3, 3)), np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3, 3)), np.zeros((max(n, 1), 3, 3))
        cost, chi2, rows = C.c_double(), np.zeros(max(ne, 1)), C.c_int32(-1)
        rc = self._lib.visfs_pose_graph_linearize(self.h, len(p), _ptr(p, C.c_double), _ptr(f, C.c_uint8), ne, e, C.byref(rows),
                                                  _ptr(eb, C.c_double), _ptr(g, C.c_double), _ptr(D, C.c_double), _ptr(Cb, C.c_double),
                                                  C.byref(cost), _ptr(chi2, C.c_double))
        return rc, {"rows": rows.value, "edge_blocks": eb[:ne], "g": g[:n], "D": D[:n], "C": Cb[:n], "cost": cost.value, "chi2": chi2[:ne]}

    def precondition(self, poses, fixed, edges, lam, r, preconditioner=1):
        """(status, z [n][3]) with z = M^-1 r."""
        p, f, e, ne = self._graph(poses, fixed, edges)
        rr = np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 3))
        assert len(rr) == int(np.sum(f == 0))
        z = np.zeros_like(rr)
        rc = self._lib.visfs_pose_graph_precondition(self.h, preconditioner, float(lam), len(p), _ptr(p, C.c_double), _ptr(f, C.c_uint8), ne, e,
                                                     _ptr(rr, C.c_double), _ptr(z, C.c_double))
        return rc, z

    def last_counts(self):
        a, b, c = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        rc = self._lib.visfs_pose_graph_last_counts(self.h, C.byref(a), C.byref(b), C.byref(c))
        assert rc == abi.OK, rc
        return a.value, b.value, c.value
