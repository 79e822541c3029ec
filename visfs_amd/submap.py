"""ctypes binding of the laser sub-maps (include/visfs_submap.h, in libvisfs_ba_hip.so) — plumbing only.

`Submaps(params, solver=s)` keeps the grids on the device of `backend.Solver` `s` and inserts with HIP kernels;
`Submaps(params)` without a solver is the host restatement (one core) the parity tests compare against.
"""
import ctypes as C

import numpy as np

from . import abi, backend

ABI_VERSION = 1
EXPORTS = [
    "visfs_submap_abi_version", "visfs_submap_default_params", "visfs_submaps_create", "visfs_submaps_create_host",
    "visfs_submaps_destroy", "visfs_submaps_last_error", "visfs_submaps_insert", "visfs_submaps_describe",
    "visfs_submaps_download", "visfs_submaps_solve_window", "visfs_submap_hook_ray", "visfs_submap_hook_odds_table",
    "visfs_submap_hook_value_tables", "visfs_submap_hook_crop", "visfs_submap_hook_mark_items",
]


class Params(C.Structure):
    _fields_ = [("num_range_data_limit", C.c_int32), ("grid_map_type", C.c_int32), ("map_resolution", C.c_double),
                ("insert_free_space", C.c_int32), ("hit_probability", C.c_double), ("miss_probability", C.c_double)]


class RangeData(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("n_returns", C.c_int32), ("returns", C.POINTER(C.c_double)),
                ("n_misses", C.c_int32), ("misses", C.POINTER(C.c_double))]


class Info(C.Structure):
    _fields_ = [("num_range_data", C.c_int32), ("finished", C.c_int32), ("resolution", C.c_double),
                ("max_x", C.c_double), ("max_y", C.c_double), ("num_x_cells", C.c_int32), ("num_y_cells", C.c_int32),
                ("known_min_x", C.c_int32), ("known_min_y", C.c_int32), ("known_max_x", C.c_int32), ("known_max_y", C.c_int32)]

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
    lib.visfs_submap_abi_version.restype = C.c_int
    lib.visfs_submap_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_submap_default_params.restype = None
    lib.visfs_submaps_create.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(C.c_void_p)]
    lib.visfs_submaps_create.restype = C.c_int
    lib.visfs_submaps_create_host.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p)]
    lib.visfs_submaps_create_host.restype = C.c_int
    lib.visfs_submaps_destroy.argtypes = [C.c_void_p]
    lib.visfs_submaps_destroy.restype = None
    lib.visfs_submaps_last_error.argtypes = [C.c_void_p]
    lib.visfs_submaps_last_error.restype = C.c_char_p
    lib.visfs_submaps_insert.argtypes = [C.c_void_p, _pd, C.c_int32, C.POINTER(RangeData)]
    lib.visfs_submaps_insert.restype = C.c_int
    lib.visfs_submaps_describe.argtypes = [C.c_void_p, _pi32, C.POINTER(Info)]
    lib.visfs_submaps_describe.restype = C.c_int
    lib.visfs_submaps_download.argtypes = [C.c_void_p, C.c_int32, _pu16, C.POINTER(C.c_float)]
    lib.visfs_submaps_download.restype = C.c_int
    lib.visfs_submaps_solve_window.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.Window), C.POINTER(abi.Result)]
    lib.visfs_submaps_solve_window.restype = C.c_int
    lib.visfs_submap_hook_ray.argtypes = [_pi32, _pi32, C.c_int32, C.c_int32, _pi32]
    lib.visfs_submap_hook_ray.restype = C.c_int
    lib.visfs_submap_hook_mark_items.argtypes = [_pi32, _pi32, C.c_int32, C.c_int32, _pi32, C.POINTER(C.c_int64)]
    lib.visfs_submap_hook_mark_items.restype = C.c_int
    lib.visfs_submap_hook_odds_table.argtypes = [C.c_double, _pu16]
    lib.visfs_submap_hook_odds_table.restype = C.c_int
    lib.visfs_submap_hook_value_tables.argtypes = [_pd, _pu16]
    lib.visfs_submap_hook_value_tables.restype = C.c_int
    lib.visfs_submap_hook_crop.argtypes = [C.c_int32, C.c_int32, _pu16, _pi32, C.c_int64, _pi32, _pu16, _pi32]
    lib.visfs_submap_hook_crop.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def default_params(**kw):
    p = Params()
    load().visfs_submap_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Submaps:
    """ActiveSubmaps2D over the C ABI.  solver: a backend.Solver (device grids) or None (host restatement)."""

    def __init__(self, params=None, solver=None):
        self._lib = load()
        self.params = params if params is not None else default_params()
        self.solver = solver
        h = C.c_void_p()
        if solver is None:
            rc = self._lib.visfs_submaps_create_host(C.byref(self.params), C.byref(h))
        else:
            rc = self._lib.visfs_submaps_create(solver.h, C.byref(self.params), C.byref(h))
        self.status = rc
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_submaps_create failed with status {rc}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_submaps_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_submaps_last_error(self.h).decode()

    def insert(self, Twr, range_data):
        """range_data: list of (origin[3], returns[k][3], misses[m][3]) in the robot frame; Twr 3x4 (or 12 values)."""
        T = np.ascontiguousarray(np.asarray(Twr, dtype=np.float64).reshape(12))
        keep = []
        arr = (RangeData * max(len(range_data), 1))()
        for i, (o, ret, mis) in enumerate(range_data):
            ret = np.ascontiguousarray(np.asarray(ret, dtype=np.float64).reshape(-1, 3))
            mis = np.ascontiguousarray(np.asarray(mis, dtype=np.float64).reshape(-1, 3))
            keep += [ret, mis]
            arr[i].origin[:] = [float(v) for v in o]
            arr[i].n_returns = len(ret)
            arr[i].returns = _ptr(ret, C.c_double)
            arr[i].n_misses = len(mis)
            arr[i].misses = _ptr(mis, C.c_double)
        return self._lib.visfs_submaps_insert(self.h, _ptr(T, C.c_double), len(range_data), arr)

    def describe(self):
        n = C.c_int32()
        info = (Info * 2)()
        rc = self._lib.visfs_submaps_describe(self.h, C.byref(n), info)
        assert rc == abi.OK, rc
        return [info[i].as_dict() for i in range(n.value)]

    def download(self, index):
        d = self.describe()[index]
        cells = np.zeros((d["num_y_cells"], d["num_x_cells"]), dtype=np.uint16)
        cost = np.zeros((d["num_y_cells"], d["num_x_cells"]), dtype=np.float32)
        rc = self._lib.visfs_submaps_download(self.h, index, _ptr(cells, C.c_uint16), _ptr(cost, C.c_float))
        assert rc == abi.OK, (rc, self.last_error())
        return cells, cost

    def solve_window(self, wb, solver=None):
        """visfs_submaps_solve_window on `solver` (default: the one the sub-maps live on) for abi.WindowBuffers `wb`."""
        s = solver or self.solver
        rb = abi.ResultBuffers(wb.struct.n_poses, wb.struct.n_refs)
        rc = self._lib.visfs_submaps_solve_window(s.h, self.h, C.byref(wb.struct), C.byref(rb.struct))
        return rc, rb


# ---- host-only hooks
def hook_ray(begin, end, scale=1000):
    lib = load()
    b = np.asarray(begin, dtype=np.int32); e = np.asarray(end, dtype=np.int32)
    n = lib.visfs_submap_hook_ray(_ptr(b, C.c_int32), _ptr(e, C.c_int32), scale, 0, None)
    assert n >= 0, n
    out = np.zeros((max(n, 1), 2), dtype=np.int32)
    n2 = lib.visfs_submap_hook_ray(_ptr(b, C.c_int32), _ptr(e, C.c_int32), scale, n, _ptr(out, C.c_int32))
    assert n2 == n
    return [tuple(int(v) for v in c) for c in out[:n]]


def hook_mark_items(begin, end, scale=1000):
    """(cells, items): the ray's cells as the mark kernel's work items enumerate them, and the number of work items."""
    lib = load()
    b = np.asarray(begin, dtype=np.int32); e = np.asarray(end, dtype=np.int32)
    items = C.c_int64()
    n = lib.visfs_submap_hook_mark_items(_ptr(b, C.c_int32), _ptr(e, C.c_int32), scale, 0, None, C.byref(items))
    assert n >= 0, n
    out = np.zeros((max(n, 1), 2), dtype=np.int32)
    n2 = lib.visfs_submap_hook_mark_items(_ptr(b, C.c_int32), _ptr(e, C.c_int32), scale, n, _ptr(out, C.c_int32), C.byref(items))
    assert n2 == n
    return [tuple(int(v) for v in c) for c in out[:n]], int(items.value)


def hook_odds_table(odds):
    t = np.zeros(32768, dtype=np.uint16)
    assert load().visfs_submap_hook_odds_table(odds, _ptr(t, C.c_uint16)) == abi.OK
    return t


def hook_value_tables():
    cost = np.zeros(32768, dtype=np.float64)
    crop = np.zeros(32768, dtype=np.uint16)
    assert load().visfs_submap_hook_value_tables(_ptr(cost, C.c_double), _ptr(crop, C.c_uint16)) == abi.OK
    return cost, crop


def hook_crop(cells, box):
    cells = np.ascontiguousarray(cells, dtype=np.uint16)
    ny, nx = cells.shape
    b = np.asarray(box, dtype=np.int32)
    dims = np.zeros(4, dtype=np.int32)
    obox = np.zeros(4, dtype=np.int32)
    out = np.zeros(nx * ny, dtype=np.uint16)
    rc = load().visfs_submap_hook_crop(nx, ny, _ptr(cells, C.c_uint16), _ptr(b, C.c_int32), out.size, _ptr(dims, C.c_int32),
                                       _ptr(out, C.c_uint16), _ptr(obox, C.c_int32))
    assert rc == abi.OK, rc
    ox, oy, cx, cy = (int(v) for v in dims)
    return (ox, oy), out[:cx * cy].reshape(cy, cx), tuple(int(v) for v in obox)
