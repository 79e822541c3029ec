"""ctypes binding of the verified place query (include/visfs_place_verify.h, in libvisfs_ba_hip.so) — plumbing only.

`Verifier(store)` answers `query_verify(set, ...)`: the place query, the PnP pose of every candidate and the guided second stage in
one call.  HIP kernels when the store lives on a solver's device, the one-core twin for `KeyFrameStore(None)`.  `closure_edge(T, cov)`
turns a verified candidate into what a pose-graph edge takes.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import place as _place
from . import pnp as _pnp

ABI_VERSION = 1
EXPORTS = [
    "visfs_place_verify_abi_version", "visfs_place_verify_default_params", "visfs_place_verifier_create", "visfs_place_verifier_destroy",
    "visfs_place_verifier_last_error", "visfs_place_query_verify", "visfs_place_verify_last_counts", "visfs_place_verify_download_pnp",
    "visfs_place_verify_download_guided", "visfs_place_verify_hook_window", "visfs_place_closure_edge",
]
LAUNCHES = 7
MAX_POINTS = _place.MAX_POINTS
MAX_CANDIDATES = _place.MAX_CANDIDATES


class Params(C.Structure):
    _fields_ = [("pnp", _pnp.Params), ("camera", _pnp.Camera), ("guided", C.c_int32), ("guided_radius", C.c_float),
                ("guided_max_distance", C.c_int32), ("pad", C.c_int32)]


class Stage1(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("matches", C.c_int32 * MAX_POINTS), ("inliers", C.c_int32 * MAX_POINTS),
                ("T", C.c_double * 16), ("cov", C.c_double * 36)]


class Stage2(C.Structure):
    _fields_ = [("ran", C.c_int32), ("n_rows", C.c_int32), ("row", _place.Row * MAX_POINTS), ("n_inliers", C.c_int32), ("pad", C.c_int32),
                ("inliers", C.c_int32 * MAX_POINTS), ("T", C.c_double * 16), ("cov", C.c_double * 36)]


class Candidate(C.Structure):
    _fields_ = [("stage1", Stage1), ("stage2", Stage2)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int32), ("best", C.c_int32), ("candidate", Candidate * MAX_CANDIDATES)]


_pf = C.POINTER(C.c_float)
_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    _place.load()
    _pnp.load()
    lib = backend.load_library()
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_place_verify_abi_version.restype = C.c_int
    lib.visfs_place_verify_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_place_verify_default_params.restype = None
    lib.visfs_place_verifier_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.visfs_place_verifier_create.restype = C.c_int
    lib.visfs_place_verifier_destroy.argtypes = [C.c_void_p]
    lib.visfs_place_verifier_destroy.restype = None
    lib.visfs_place_verifier_last_error.argtypes = [C.c_void_p]
    lib.visfs_place_verifier_last_error.restype = C.c_char_p
    lib.visfs_place_query_verify.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_place.Params), C.POINTER(Params), _pf, C.POINTER(_place.Result),
                                             C.POINTER(Result)]
    lib.visfs_place_query_verify.restype = C.c_int
    lib.visfs_place_verify_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32, _pi32]
    lib.visfs_place_verify_last_counts.restype = C.c_int
    lib.visfs_place_verify_download_pnp.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _pi32, _pi32, _pi32, _pi32, _pi32, _pd, _pi32, _pi32, _pd,
                                                    _pd, _pf, _pi32, _pi32]
    lib.visfs_place_verify_download_pnp.restype = C.c_int
    lib.visfs_place_verify_download_guided.argtypes = [C.c_void_p, C.c_int32, _pi32, _pi32]
    lib.visfs_place_verify_download_guided.restype = C.c_int
    lib.visfs_place_verify_hook_window.argtypes = [C.c_double, C.c_double, C.c_float, C.c_float, C.c_float]
    lib.visfs_place_verify_hook_window.restype = C.c_int
    lib.visfs_place_closure_edge.argtypes = [_pd, _pd, _pd, _pd, _pd]
    lib.visfs_place_closure_edge.restype = C.c_int
    if lib.visfs_place_verify_abi_version() != ABI_VERSION:
        raise backend.BackendError("ABI version mismatch between visfs_amd/place_verify.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(camera=None, pnp=None, **kw):
    """The defaults with `camera` (a pnp.Camera) put in; pnp: a dict of visfs_pnp_params fields; kw: the guided fields."""
    p = Params()
    load().visfs_place_verify_default_params(C.byref(p))
    if camera is not None:
        p.camera = camera
    for k, v in (pnp or {}).items():
        setattr(p.pnp, k, v)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def in_window(pu, pv, qx, qy, radius):
    """Test hook: the window test of the guided stage on one pair."""
    return bool(load().visfs_place_verify_hook_window(float(pu), float(pv), float(qx), float(qy), float(radius)))


def closure_edge_status(T, cov):
    """(status, z [3], information [3][3], out_of_plane [3])"""
    T = None if T is None else np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(16))
    cov = None if cov is None else np.ascontiguousarray(np.asarray(cov, dtype=np.float64).reshape(36))
    z, info, oop = np.zeros(3), np.zeros((3, 3)), np.zeros(3)
    rc = load().visfs_place_closure_edge(_ptr(T, C.c_double) if T is not None else None, _ptr(cov, C.c_double) if cov is not None else None,
                                         _ptr(z, C.c_double), _ptr(info, C.c_double), _ptr(oop, C.c_double))
    return rc, z, info, oop


def closure_edge(T, cov):
    rc, z, info, oop = closure_edge_status(T, cov)
    if rc != abi.OK:
        raise backend.BackendError(f"visfs_place_closure_edge: status {rc}")
    return z, info, oop


class Verifier:
    """The verifier of a place.KeyFrameStore.  Close it before the store."""

    def __init__(self, store):
        self._lib = load()
        self.store = store
        h = C.c_void_p()
        self.status = self._lib.visfs_place_verifier_create(store.h, C.byref(h))
        if self.status != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_place_verifier_create failed with status {self.status}: {store.last_error()}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_place_verifier_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_place_verifier_last_error(self.h).decode()

    def query_verify_raw(self, dset, verify_params, query_xyz=None, **place_params):
        """(status, place.Result, Result)"""
        pp = _place.default_params(**place_params)
        q = None if query_xyz is None else np.ascontiguousarray(np.asarray(query_xyz, dtype=np.float32).reshape(-1, 3))
        r, v = _place.Result(), Result()
        rc = self._lib.visfs_place_query_verify(self.h, dset.h, C.byref(pp), C.byref(verify_params), _ptr(q, C.c_float) if q is not None else None,
                                                C.byref(r), C.byref(v))
        return rc, r, v

    def query_verify(self, dset, verify_params, query_xyz=None, **place_params):
        """(place.unpack of the place block, unpack of the verify block)"""
        rc, r, v = self.query_verify_raw(dset, verify_params, query_xyz, **place_params)
        if rc != abi.OK:
            raise backend.BackendError(f"query_verify: status {rc}: {self.last_error()}")
        return _place.unpack(r), unpack(v, r.n_candidates)

    def last_counts(self):
        """(uploads, launches, downloads, waits) of the last query_verify."""
        v = [C.c_int32(-1) for _ in range(4)]
        rc = self._lib.visfs_place_verify_last_counts(self.h, *[C.byref(x) for x in v])
        if rc != abi.OK:
            raise backend.BackendError(f"last_counts: status {rc}")
        return tuple(x.value for x in v)

    def download_pnp(self, c, stage):
        """The state of candidate c's stage (1 or 2), as pnp.Pnp.download gives it, with n_hypotheses and n_passes."""
        m, H, R = C.c_int32(), C.c_int32(), C.c_int32()
        none = [None] * 10
        rc = self._lib.visfs_place_verify_download_pnp(self.h, c, stage, C.byref(m), C.byref(H), C.byref(R), *none)
        if rc != abi.OK:
            raise backend.BackendError(f"download_pnp: status {rc}: {self.last_error()}")
        m, H, R = m.value, H.value, R.value
        out = {"m": m, "n_hypotheses": H, "n_passes": R, "samples": np.zeros((H, 4), dtype=np.int32), "valid": np.zeros(H, dtype=np.int32),
               "models": np.zeros((H, 3, 4)), "counts": np.zeros(H, dtype=np.int32), "refit_tq": np.zeros(7), "pass_tq": np.zeros((R, 7)),
               "pass_threshold": np.zeros(R, dtype=np.float32), "pass_count": np.zeros(R, dtype=np.int32),
               "pass_inliers": np.zeros((R, m), dtype=np.int32)}
        w = C.c_int32()
        rc = self._lib.visfs_place_verify_download_pnp(
            self.h, c, stage, None, None, None, _ptr(out["samples"], C.c_int32), _ptr(out["valid"], C.c_int32), _ptr(out["models"], C.c_double),
            _ptr(out["counts"], C.c_int32), C.byref(w), _ptr(out["refit_tq"], C.c_double), _ptr(out["pass_tq"], C.c_double),
            _ptr(out["pass_threshold"], C.c_float), _ptr(out["pass_count"], C.c_int32), _ptr(out["pass_inliers"], C.c_int32))
        if rc != abi.OK:
            raise backend.BackendError(f"download_pnp: status {rc}: {self.last_error()}")
        out["winner"] = w.value
        return out

    def download_guided(self, c):
        """(pick int32 [512] per entry, keep int32 [512] per query) of candidate c; -1: none."""
        pick, keep = np.zeros(MAX_POINTS, dtype=np.int32), np.zeros(MAX_POINTS, dtype=np.int32)
        rc = self._lib.visfs_place_verify_download_guided(self.h, c, _ptr(pick, C.c_int32), _ptr(keep, C.c_int32))
        if rc != abi.OK:
            raise backend.BackendError(f"download_guided: status {rc}: {self.last_error()}")
        return pick, keep


def unpack(v, n_candidates=MAX_CANDIDATES):
    """dict(best, candidates: list of dict(stage1: dict(matches, inliers, T, cov), stage2: dict(ran, rows, inliers, T, cov)), raw)."""
    cands = []
    for c in range(n_candidates):
        k = v.candidate[c]
        a, b = k.stage1, k.stage2
        rows = np.frombuffer(bytes(memoryview(b.row)), dtype=_place.ROW_DTYPE)[:b.n_rows].copy()
        cands.append(dict(
            stage1=dict(matches=np.array(a.matches[:a.n_matches], dtype=np.int32), inliers=np.array(a.inliers[:a.n_inliers], dtype=np.int32),
                        T=np.array(a.T[:]).reshape(4, 4), cov=np.array(a.cov[:]).reshape(6, 6)),
            stage2=dict(ran=b.ran, rows=rows, inliers=np.array(b.inliers[:b.n_inliers], dtype=np.int32), T=np.array(b.T[:]).reshape(4, 4),
                        cov=np.array(b.cov[:]).reshape(6, 6))))
    return dict(status=v.status, best=v.best, candidates=cands, raw=bytes(memoryview(v)))
