"""ctypes binding of the global occupancy map (include/visfs_map.h, in libvisfs_ba_hip.so) — plumbing only.

`GlobalMap(solver)` keeps the tiles and the composed grid on the device of `backend.Solver` `solver` and composes with a HIP
kernel; `GlobalMap()` is the one-core host twin.  `.add_submap(submaps, index, pose)` / `.add_grid(cells, limits, pose)` freeze a
tile, `.set_poses(first, poses)` moves tiles, `.compose(...)` draws them, `.download()` fetches cells and counts, `.freeze(depth)`
makes a `scan_fast.ScanStack` of the composed grid.  `plan(...)`, `hook_odds_table()` and `.last_counts()` are the test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import scan_fast as sf
from . import submap as sm

ABI_VERSION = 1
EXPORTS = [
    "visfs_map_abi_version", "visfs_map_default_params", "visfs_map_create", "visfs_map_destroy", "visfs_map_last_error",
    "visfs_map_add_submap", "visfs_map_add_grid", "visfs_map_set_poses", "visfs_map_clear", "visfs_map_describe_tile",
    "visfs_map_compose", "visfs_map_download", "visfs_scan_stack_create_from_map", "visfs_map_pose_from_anchor",
    "visfs_map_hook_odds_table", "visfs_map_plan", "visfs_map_last_counts",
]
MAX_TILES = 256
MAX_CELLS = 1 << 26
MAX_TILE_BYTES = 1 << 30
ODDS, LATEST, OCCUPIED = 0, 1, 2
LIMIT_KEYS = ("resolution", "max_x", "max_y", "num_x_cells", "num_y_cells")


class Params(C.Structure):
    _fields_ = [("combine", C.c_int32), ("resolution", C.c_double), ("explicit_limits", C.c_int32), ("limits", sm.Info)]


class Info(C.Structure):
    _fields_ = [("limits", sm.Info), ("tiles", C.c_int32), ("tiles_drawn", C.c_int32)]

    def as_dict(self):
        d = self.limits.as_dict()
        d["tiles"] = self.tiles
        d["tiles_drawn"] = self.tiles_drawn
        return d


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_pu16 = C.POINTER(C.c_uint16)
_pu8 = C.POINTER(C.c_uint8)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    lib.visfs_map_abi_version.restype = C.c_int
    lib.visfs_map_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_map_default_params.restype = None
    lib.visfs_map_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.visfs_map_create.restype = C.c_int
    lib.visfs_map_destroy.argtypes = [C.c_void_p]
    lib.visfs_map_destroy.restype = None
    lib.visfs_map_last_error.argtypes = [C.c_void_p]
    lib.visfs_map_last_error.restype = C.c_char_p
    lib.visfs_map_add_submap.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, _pd, _pi32]
    lib.visfs_map_add_submap.restype = C.c_int
    lib.visfs_map_add_grid.argtypes = [C.c_void_p, C.POINTER(sm.Info), _pu16, _pd, _pi32]
    lib.visfs_map_add_grid.restype = C.c_int
    lib.visfs_map_set_poses.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _pd]
    lib.visfs_map_set_poses.restype = C.c_int
    lib.visfs_map_clear.argtypes = [C.c_void_p]
    lib.visfs_map_clear.restype = C.c_int
    lib.visfs_map_describe_tile.argtypes = [C.c_void_p, C.c_int32, C.POINTER(sm.Info), _pd]
    lib.visfs_map_describe_tile.restype = C.c_int
    lib.visfs_map_compose.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Info)]
    lib.visfs_map_compose.restype = C.c_int
    lib.visfs_map_download.argtypes = [C.c_void_p, _pu16, _pu8]
    lib.visfs_map_download.restype = C.c_int
    lib.visfs_scan_stack_create_from_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.visfs_scan_stack_create_from_map.restype = C.c_int
    lib.visfs_map_pose_from_anchor.argtypes = [_pd, _pd, _pd]
    lib.visfs_map_pose_from_anchor.restype = C.c_int
    lib.visfs_map_hook_odds_table.argtypes = [_pi32]
    lib.visfs_map_hook_odds_table.restype = C.c_int
    lib.visfs_map_plan.argtypes = [C.c_int32, C.POINTER(sm.Info), _pd, C.POINTER(Params), C.POINTER(sm.Info), _pi32, _pi32]
    lib.visfs_map_plan.restype = C.c_int
    lib.visfs_map_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_map_last_counts.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def limits_info(limits):
    """A dict with resolution, max_x, max_y, num_x_cells, num_y_cells (as Submaps.describe gives it) as a visfs_submap_info."""
    info = sm.Info()
    for k in LIMIT_KEYS:
        setattr(info, k, limits[k])
    return info


def make_params(combine=ODDS, resolution=0.05, limits=None):
    """limits: None (from the tiles' extents) or a dict with the five limit keys (explicit limits)."""
    p = Params()
    load().visfs_map_default_params(C.byref(p))
    p.combine = combine
    p.resolution = resolution
    if limits is not None:
        p.explicit_limits = 1
        p.limits = limits_info(limits)
    return p


def _pose(pose):
    return np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(3))


class GlobalMap:
    """A visfs_map over the C ABI.  solver: a backend.Solver (device) or None (the host twin)."""

    def __init__(self, solver=None):
        self._lib = load()
        self.solver = solver
        h = C.c_void_p()
        rc = self._lib.visfs_map_create(solver.h if solver is not None else None, C.byref(h))
        self.status = rc
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_map_create failed with status {rc}")
        self.h = h
        self.limits = None                    # of the last successful compose

    def close(self):
        if self.h:
            self._lib.visfs_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_map_last_error(self.h).decode()

    def add_submap(self, submaps, index=0, pose=(0.0, 0.0, 0.0)):
        """(status, tile index)."""
        t = C.c_int32(-1)
        rc = self._lib.visfs_map_add_submap(self.h, submaps.h, index, _ptr(_pose(pose), C.c_double), C.byref(t))
        return rc, t.value

    def add_grid(self, cells, limits, pose=(0.0, 0.0, 0.0), check_size=True):
        """cells [ny][nx] uint16 as Submaps.download hands them out; limits: a dict as Submaps.describe gives it.  (status, tile)."""
        info = limits_info(limits)
        c = np.ascontiguousarray(cells, dtype=np.uint16)
        if check_size:
            assert c.size == info.num_x_cells * info.num_y_cells
        t = C.c_int32(-1)
        rc = self._lib.visfs_map_add_grid(self.h, C.byref(info), _ptr(c, C.c_uint16), _ptr(_pose(pose), C.c_double), C.byref(t))
        return rc, t.value

    def set_poses(self, first, poses):
        p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        return self._lib.visfs_map_set_poses(self.h, first, len(p), _ptr(p, C.c_double))

    def clear(self):
        return self._lib.visfs_map_clear(self.h)

    def describe_tile(self, tile):
        """(status, limits dict, pose)."""
        info = sm.Info()
        pose = np.zeros(3)
        rc = self._lib.visfs_map_describe_tile(self.h, tile, C.byref(info), _ptr(pose, C.c_double))
        return rc, {k: getattr(info, k) for k in LIMIT_KEYS}, pose

    def compose(self, combine=ODDS, resolution=0.05, limits=None, params=None):
        """(status, info dict)."""
        p = params if params is not None else make_params(combine, resolution, limits)
        info = Info()
        rc = self._lib.visfs_map_compose(self.h, C.byref(p), C.byref(info))
        d = info.as_dict()
        if rc == abi.OK:
            self.limits = d
        return rc, d

    def download(self):
        """(status, cells [ny][nx] uint16, counts [ny][nx] uint8) of the last composed grid."""
        if self.limits is None:
            return self._lib.visfs_map_download(self.h, None, None), None, None
        ny, nx = self.limits["num_y_cells"], self.limits["num_x_cells"]
        cells = np.zeros((ny, nx), dtype=np.uint16)
        count = np.zeros((ny, nx), dtype=np.uint8)
        rc = self._lib.visfs_map_download(self.h, _ptr(cells, C.c_uint16), _ptr(count, C.c_uint8))
        return rc, cells, count

    def freeze(self, depth=7):
        """The last composed grid as a scan_fast.ScanStack of the map's flavour."""
        h = C.c_void_p()
        rc = self._lib.visfs_scan_stack_create_from_map(self.h, depth, C.byref(h))
        return sf.ScanStack(h if rc == abi.OK else None, rc, self.solver)

    def last_counts(self):
        v = [C.c_int32(-1) for _ in range(3)]
        rc = self._lib.visfs_map_last_counts(self.h, *[C.byref(x) for x in v])
        assert rc == abi.OK, rc
        return tuple(x.value for x in v)


def pose_from_anchor(frozen, now):
    out = np.zeros(3)
    rc = load().visfs_map_pose_from_anchor(_ptr(_pose(frozen), C.c_double), _ptr(_pose(now), C.c_double), _ptr(out, C.c_double))
    return rc, out


def hook_odds_table():
    t = np.zeros(32768, dtype=np.int32)
    assert load().visfs_map_hook_odds_table(_ptr(t, C.c_int32)) == abi.OK
    return t


def plan(tile_limits, poses, combine=ODDS, resolution=0.05, limits=None, params=None):
    """visfs_map_plan: (status, composed limits dict with the known box, boxes [n][4] int32, tiles drawn)."""
    n = len(tile_limits)
    arr = (sm.Info * max(n, 1))()
    for i, l in enumerate(tile_limits):
        arr[i] = limits_info(l)
    p = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
    assert len(p) == n
    prm = params if params is not None else make_params(combine, resolution, limits)
    out = sm.Info()
    boxes = np.zeros((max(n, 1), 4), dtype=np.int32)
    drawn = C.c_int32(-1)
    rc = load().visfs_map_plan(n, arr, _ptr(p, C.c_double) if n else None, C.byref(prm), C.byref(out), _ptr(boxes, C.c_int32), C.byref(drawn))
    return rc, out.as_dict(), boxes[:n], drawn.value
