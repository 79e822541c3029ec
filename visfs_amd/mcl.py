"""ctypes binding of the Monte-Carlo localisation (include/visfs_mcl.h, in libvisfs_ba_hip.so) — plumbing only.

`Field.from_map(global_map)` / `Field.from_grid(cells, limits, solver=...)` make a likelihood field (device with a solver or a
device map, the one-core host twin otherwise); `Filter(field, n, seed)` is a particle filter of the field's flavour:
`.init(mean, sigma)`, `.update(odom_delta, points, ...)`, `.download()`.  `.last_counts()`, `.upload()`, `.set_lanes()` and
`hook_sincos()` are the test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import global_map as gm
from . import submap as sm

ABI_VERSION = 1
EXPORTS = [
    "visfs_mcl_abi_version", "visfs_mcl_field_default_params", "visfs_mcl_default_params", "visfs_mcl_field_create_from_map",
    "visfs_mcl_field_create_from_grid", "visfs_mcl_field_destroy", "visfs_mcl_field_describe", "visfs_mcl_field_download",
    "visfs_mcl_field_last_counts", "visfs_mcl_create", "visfs_mcl_destroy", "visfs_mcl_last_error", "visfs_mcl_init", "visfs_mcl_update",
    "visfs_mcl_last_result", "visfs_mcl_download", "visfs_mcl_upload", "visfs_mcl_hook_set_lanes", "visfs_mcl_last_counts",
    "visfs_mcl_hook_sincos",
]
MAX_RADIUS = 255
MAX_PARTICLES = 65536
MAX_BEAMS = 16384
FIELD_LAUNCHES, INIT_LAUNCHES, UPDATE_LAUNCHES = 2, 1, 4
FIELD_COUNTS = (FIELD_LAUNCHES, 1, 1)        # launches, copies, waits
INIT_COUNTS = (INIT_LAUNCHES, 1, 1)
UPDATE_COUNTS = (UPDATE_LAUNCHES, 2, 1)      # one upload and one download


class FieldInfo(C.Structure):
    _fields_ = [("limits", sm.Info), ("R", C.c_int32), ("T", C.c_int32), ("v_occ", C.c_int32), ("device", C.c_int32)]


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pi64 = C.POINTER(C.c_int64)
_pu16 = C.POINTER(C.c_uint16)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    lib.visfs_mcl_abi_version.restype = C.c_int
    lib.visfs_mcl_field_default_params.argtypes = [C.POINTER(abi.MclFieldParams)]
    lib.visfs_mcl_field_default_params.restype = None
    lib.visfs_mcl_default_params.argtypes = [C.POINTER(abi.MclParams)]
    lib.visfs_mcl_default_params.restype = None
    lib.visfs_mcl_field_create_from_map.argtypes = [C.c_void_p, C.POINTER(abi.MclFieldParams), C.POINTER(C.c_void_p)]
    lib.visfs_mcl_field_create_from_map.restype = C.c_int
    lib.visfs_mcl_field_create_from_grid.argtypes = [C.c_void_p, C.POINTER(sm.Info), _pu16, C.POINTER(abi.MclFieldParams), C.POINTER(C.c_void_p)]
    lib.visfs_mcl_field_create_from_grid.restype = C.c_int
    lib.visfs_mcl_field_destroy.argtypes = [C.c_void_p]
    lib.visfs_mcl_field_destroy.restype = None
    lib.visfs_mcl_field_describe.argtypes = [C.c_void_p, C.POINTER(FieldInfo)]
    lib.visfs_mcl_field_describe.restype = C.c_int
    lib.visfs_mcl_field_download.argtypes = [C.c_void_p, _pu16, _pi64, _pi32, _pi32]
    lib.visfs_mcl_field_download.restype = C.c_int
    lib.visfs_mcl_field_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_mcl_field_last_counts.restype = C.c_int
    lib.visfs_mcl_create.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]
    lib.visfs_mcl_create.restype = C.c_int
    lib.visfs_mcl_destroy.argtypes = [C.c_void_p]
    lib.visfs_mcl_destroy.restype = None
    lib.visfs_mcl_last_error.argtypes = [C.c_void_p]
    lib.visfs_mcl_last_error.restype = C.c_char_p
    lib.visfs_mcl_init.argtypes = [C.c_void_p, _pd, _pd]
    lib.visfs_mcl_init.restype = C.c_int
    lib.visfs_mcl_update.argtypes = [C.c_void_p, C.POINTER(abi.MclParams), _pd, C.c_int32, _pd, C.POINTER(abi.MclResult)]
    lib.visfs_mcl_update.restype = C.c_int
    lib.visfs_mcl_last_result.argtypes = [C.c_void_p, C.POINTER(abi.MclResult)]
    lib.visfs_mcl_last_result.restype = C.c_int
    lib.visfs_mcl_download.argtypes = [C.c_void_p, _pd, _pd, _pd, _pd, _pi64, _pi32]
    lib.visfs_mcl_download.restype = C.c_int
    lib.visfs_mcl_upload.argtypes = [C.c_void_p, _pd, _pd, _pd, _pd]
    lib.visfs_mcl_upload.restype = C.c_int
    lib.visfs_mcl_hook_set_lanes.argtypes = [C.c_void_p, C.c_int32]
    lib.visfs_mcl_hook_set_lanes.restype = C.c_int
    lib.visfs_mcl_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_mcl_last_counts.restype = C.c_int
    lib.visfs_mcl_hook_sincos.argtypes = [C.c_int32, _pd, _pd, _pd]
    lib.visfs_mcl_hook_sincos.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def field_params(**kw):
    """The header's defaults (the shipped amcl.yaml's values), with keyword overrides."""
    p = abi.MclFieldParams()
    load().visfs_mcl_field_default_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def default_params(**kw):
    p = abi.MclParams()
    load().visfs_mcl_default_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _counts(fn, h):
    v = [C.c_int32(-1) for _ in range(3)]
    rc = fn(h, *[C.byref(x) for x in v])
    assert rc == abi.OK, rc
    return tuple(x.value for x in v)


class Field:
    """A visfs_mcl_field over the C ABI; `status` is the creation's, `h` None when it was refused."""

    def __init__(self, h, status, solver=None):
        self._lib = load()
        self.h, self.status, self.solver = h, status, solver

    @classmethod
    def from_map(cls, gmap, params=None):
        lib = load()
        p = params if params is not None else field_params()
        h = C.c_void_p()
        rc = lib.visfs_mcl_field_create_from_map(gmap.h, C.byref(p), C.byref(h))
        return cls(h if rc == abi.OK else None, rc, gmap.solver)

    @classmethod
    def from_grid(cls, cells, limits, params=None, solver=None):
        """cells [ny][nx] uint16 and a limits dict as GlobalMap.download / compose hand them out."""
        lib = load()
        p = params if params is not None else field_params()
        info = gm.limits_info(limits)
        c = np.ascontiguousarray(cells, dtype=np.uint16)
        assert c.size == max(info.num_x_cells, 0) * max(info.num_y_cells, 0) or info.num_x_cells < 1 or info.num_y_cells < 1
        h = C.c_void_p()
        rc = lib.visfs_mcl_field_create_from_grid(solver.h if solver is not None else None, C.byref(info), _ptr(c, C.c_uint16), C.byref(p), C.byref(h))
        return cls(h if rc == abi.OK else None, rc, solver)

    def close(self):
        if self.h:
            self._lib.visfs_mcl_field_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def describe(self):
        info = FieldInfo()
        rc = self._lib.visfs_mcl_field_describe(self.h, C.byref(info))
        assert rc == abi.OK, rc
        d = {k: getattr(info.limits, k) for k in gm.LIMIT_KEYS}
        d.update(R=info.R, T=info.T, v_occ=info.v_occ, device=info.device)
        return d

    def download(self):
        """(t [ny][nx] uint16, q [T + 1] int64, v_occ, T)."""
        d = self.describe()
        t = np.zeros((d["num_y_cells"], d["num_x_cells"]), dtype=np.uint16)
        q = np.zeros(d["T"] + 1, dtype=np.int64)
        v, T = C.c_int32(-1), C.c_int32(-1)
        rc = self._lib.visfs_mcl_field_download(self.h, _ptr(t, C.c_uint16), _ptr(q, C.c_int64), C.byref(v), C.byref(T))
        assert rc == abi.OK, rc
        return t, q, v.value, T.value

    def last_counts(self):
        return _counts(self._lib.visfs_mcl_field_last_counts, self.h)


class Filter:
    """A visfs_mcl over the C ABI, of the field's flavour.  The field must outlive it (a reference is kept)."""

    def __init__(self, field, n_particles, seed=0):
        self._lib = load()
        self.field = field
        self.n = int(n_particles)
        h = C.c_void_p()
        rc = self._lib.visfs_mcl_create(field.h, self.n, C.c_uint64(seed), C.byref(h))
        self.status = rc
        self.h = h if rc == abi.OK else None

    def close(self):
        if self.h:
            self._lib.visfs_mcl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_mcl_last_error(self.h).decode()

    def init(self, mean, sigma):
        m = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(3))
        s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(3))
        return self._lib.visfs_mcl_init(self.h, _ptr(m, C.c_double), _ptr(s, C.c_double))

    def update(self, odom_delta, points_xyz, params=None):
        """(status, result dict).  points_xyz [n][3] in the robot frame (the block ScanFilter hands out)."""
        p = params if params is not None else default_params()
        d = np.ascontiguousarray(np.asarray(odom_delta, dtype=np.float64).reshape(3))
        pts = np.ascontiguousarray(np.asarray(points_xyz, dtype=np.float64).reshape(-1, 3))
        res = abi.MclResult()
        rc = self._lib.visfs_mcl_update(self.h, C.byref(p), _ptr(d, C.c_double), len(pts), _ptr(pts, C.c_double) if len(pts) else None, C.byref(res))
        return rc, res.as_dict()

    def last_result(self):
        res = abi.MclResult()
        rc = self._lib.visfs_mcl_last_result(self.h, C.byref(res))
        return rc, res.as_dict()

    def download(self):
        """dict of x, y, yaw, w (float64 [N]), Q (int64 [N]) and ancestors (int32 [N])."""
        out = {k: np.zeros(self.n, dtype=np.float64) for k in ("x", "y", "yaw", "w")}
        out["Q"] = np.zeros(self.n, dtype=np.int64)
        out["ancestors"] = np.zeros(self.n, dtype=np.int32)
        rc = self._lib.visfs_mcl_download(self.h, *[_ptr(out[k], C.c_double) for k in ("x", "y", "yaw", "w")], _ptr(out["Q"], C.c_int64),
                                          _ptr(out["ancestors"], C.c_int32))
        assert rc == abi.OK, self.last_error()
        return out

    def upload(self, x, y, yaw, w):
        a = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(self.n)) for v in (x, y, yaw, w)]
        return self._lib.visfs_mcl_upload(self.h, *[_ptr(v, C.c_double) for v in a])

    def set_lanes(self, lanes):
        return self._lib.visfs_mcl_hook_set_lanes(self.h, lanes)

    def last_counts(self):
        return _counts(self._lib.visfs_mcl_last_counts, self.h)


def hook_sincos(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    s, c = np.zeros_like(a), np.zeros_like(a)
    rc = load().visfs_mcl_hook_sincos(len(a), _ptr(a, C.c_double), _ptr(s, C.c_double), _ptr(c, C.c_double))
    assert rc == abi.OK, rc
    return s, c
