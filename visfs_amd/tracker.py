"""ctypes binding of the resident front end (include/visfs_tracker.h, in libvisfs_ba_hip.so) — plumbing only.

`Tracker(flow_obj, cam, **params)` keeps the word table of Tracker::imageProcess next to the pyramids of a `flow.Flow`: HIP kernels
when that object lives on a solver's device, the one-core host restatement otherwise.  `process(left, right, ...)` is one frame.
`TrackerGroup(members)` (include/visfs_tracker_group.h) takes the frames of several trackers of one solver in one call.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import clahe as _clahe
from . import corners as _corners
from . import fund as _fund

ABI_VERSION = 2
EXPORTS = [
    "visfs_tracker_abi_version", "visfs_tracker_default_params", "visfs_tracker_create", "visfs_tracker_destroy",
    "visfs_tracker_last_error", "visfs_tracker_reset", "visfs_tracker_process", "visfs_tracker_download",
    "visfs_tracker_download_cull",
]
GROUP_ABI_VERSION = 1
GROUP_EXPORTS = [
    "visfs_tracker_group_abi_version", "visfs_tracker_group_create", "visfs_tracker_group_destroy", "visfs_tracker_group_last_error",
    "visfs_tracker_group_process", "visfs_tracker_group_last_counts",
]
GROUP_MAX = 64
MAX_FEATURES = 4096
MAX_OUTLIERS = 4096
NO_PREVIOUS, BOOTSTRAPPED, LOST = 1, 2, 4

_pf = C.POINTER(C.c_float)
_pu8 = C.POINTER(C.c_uint8)
_pi32 = C.POINTER(C.c_int32)
_pu64 = C.POINTER(C.c_uint64)
_pd = C.POINTER(C.c_double)


class Params(C.Structure):
    _fields_ = [("max_features", C.c_int32), ("quality_level", C.c_double), ("min_distance", C.c_int32), ("min_inliers", C.c_int32),
                ("clahe", C.c_int32), ("clahe_params", _clahe.Params), ("cull", C.c_int32), ("cull_params", _fund.Params)]


class Result(C.Structure):
    _fields_ = [("flags", C.c_int32), ("n_covisible", C.c_int32), ("n_new", C.c_int32), ("n_words", C.c_int32), ("n_blocked", C.c_int32),
                ("next_id", C.c_uint64),
                ("covisible_id", _pu64), ("covisible_from_xy", _pf), ("covisible_from_xyz", _pf), ("covisible_to_xy", _pf),
                ("new_id", _pu64), ("new_xy", _pf),
                ("word_id", _pu64), ("word_left_xy", _pf), ("word_right_xy", _pf), ("word_xyz", _pf), ("word_count", _pi32),
                ("blocked_id", _pu64)]


class Frame(C.Structure):
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("stride", C.c_int32), ("delta_guess", _pd), ("n_outliers", C.c_int32),
                ("outlier_ids", _pu64)]


_lib = None


def load(require_group=True):
    """require_group=False: for a library of a parent commit (the timing tools load one): it may lack the tracker groups, and it may
    have ABI 1, which knows neither the cull fields behind clahe_params, which it does not read, nor visfs_tracker_download_cull."""
    global _lib
    if _lib is not None:
        return _lib
    lib = backend.load_library()
    if not hasattr(lib, "visfs_tracker_abi_version"):
        raise backend.BackendError("libvisfs_ba_hip.so does not export visfs_tracker_abi_version")
    lib.visfs_tracker_abi_version.restype = C.c_int
    older = lib.visfs_tracker_abi_version() == 1 and not require_group          # ABI 1: a parent commit's build, for the timing tools alone
    for name in EXPORTS + (GROUP_EXPORTS if require_group else []):
        if older and name == "visfs_tracker_download_cull":
            continue
        if not hasattr(lib, name):
            raise backend.BackendError(f"libvisfs_ba_hip.so does not export {name}")
    lib.visfs_tracker_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_tracker_default_params.restype = None
    lib.visfs_tracker_create.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(C.c_void_p)]
    lib.visfs_tracker_create.restype = C.c_int
    lib.visfs_tracker_destroy.argtypes = [C.c_void_p]
    lib.visfs_tracker_destroy.restype = None
    lib.visfs_tracker_last_error.argtypes = [C.c_void_p]
    lib.visfs_tracker_last_error.restype = C.c_char_p
    lib.visfs_tracker_reset.argtypes = [C.c_void_p]
    lib.visfs_tracker_reset.restype = C.c_int
    lib.visfs_tracker_process.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _pd, C.c_int32, _pu64, C.POINTER(Result)]
    lib.visfs_tracker_process.restype = C.c_int
    lib.visfs_tracker_download.argtypes = [C.c_void_p, _pi32, _pf, _pf, _pu8, _pu8, _pi32, C.c_void_p, _pu8, _pi32, _pu8]
    lib.visfs_tracker_download.restype = C.c_int
    if not older:
        lib.visfs_tracker_download_cull.argtypes = [C.c_void_p, _pi32, _pi32, _pi32, _pi32, _pu8, _pu8, _pd, _pd, _pd, _pi32, _pi32]
        lib.visfs_tracker_download_cull.restype = C.c_int
    if lib.visfs_tracker_abi_version() != ABI_VERSION and not older:
        raise backend.BackendError("ABI version mismatch between visfs_amd/tracker.py and libvisfs_ba_hip.so")
    if require_group:
        lib.visfs_tracker_group_abi_version.restype = C.c_int
        lib.visfs_tracker_group_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        lib.visfs_tracker_group_create.restype = C.c_int
        lib.visfs_tracker_group_destroy.argtypes = [C.c_void_p]
        lib.visfs_tracker_group_destroy.restype = None
        lib.visfs_tracker_group_last_error.argtypes = [C.c_void_p]
        lib.visfs_tracker_group_last_error.restype = C.c_char_p
        lib.visfs_tracker_group_process.argtypes = [C.c_void_p, C.POINTER(Frame), C.POINTER(Result)]
        lib.visfs_tracker_group_process.restype = C.c_int
        lib.visfs_tracker_group_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
        lib.visfs_tracker_group_last_counts.restype = C.c_int
        if lib.visfs_tracker_group_abi_version() != GROUP_ABI_VERSION:
            raise backend.BackendError("tracker group ABI version mismatch between visfs_amd/tracker.py and libvisfs_ba_hip.so")
    _lib = lib
    return lib


def default_params(clahe_params=None, cull_params=None, **kw):
    """cull=1 with a flow object whose flow_back is 0 runs Tracker/CullByFundationMatrix inside the call; cull_params: a fund.Params."""
    p = Params()
    load().visfs_tracker_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    if clahe_params is not None:
        p.clahe_params = clahe_params
    if cull_params is not None:
        p.cull_params = cull_params
    return p


_FIELDS = (("covisible_id", 1, np.uint64), ("covisible_from_xy", 2, np.float32), ("covisible_from_xyz", 3, np.float32),
           ("covisible_to_xy", 2, np.float32), ("new_id", 1, np.uint64), ("new_xy", 2, np.float32), ("word_id", 1, np.uint64),
           ("word_left_xy", 2, np.float32), ("word_right_xy", 2, np.float32), ("word_xyz", 3, np.float32), ("word_count", 1, np.int32),
           ("blocked_id", 1, np.uint64))


def create_status(flow_obj, cam, params):
    """(status, handle or None) without raising: what the argument tests look at."""
    h = C.c_void_p()
    rc = load().visfs_tracker_create(flow_obj.h, C.byref(params), C.byref(cam) if cam is not None else None, C.byref(h))
    return rc, (h if rc == abi.OK else None)


class Tracker:
    """The resident front end over the C ABI.  flow_obj: a flow.Flow (device or host twin), which must stay open while this is used."""

    def __init__(self, flow_obj, cam, params=None, **kw):
        self._lib = load()
        self.flow = flow_obj
        self.params = params if params is not None else default_params(**kw)
        self.cam = cam
        rc, h = create_status(flow_obj, cam, self.params)
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_tracker_create failed with status {rc}: {flow_obj.last_error()}")
        self.h = h
        self._views = {}                               # result field -> (address, NumPy view of the tracker's own array)

    def _take(self, res, name, n, width, dtype):
        """A copy of the first n rows of a result array.  The arrays belong to the tracker and do not move, so the view over each
        is made once."""
        ptr = getattr(res, name)
        addr = C.cast(ptr, C.c_void_p).value
        cached = self._views.get(name)
        if cached is None or cached[0] != addr:
            cap = int(self.params.max_features) * width
            cached = (addr, np.frombuffer((C.c_char * (cap * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype))
            self._views[name] = cached
        a = cached[1][:n * width].copy()
        return a.reshape(n, width) if width > 1 else a

    def close(self):
        if self.h:
            self._lib.visfs_tracker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_tracker_last_error(self.h).decode()

    def reset(self):
        rc = self._lib.visfs_tracker_reset(self.h)
        if rc != abi.OK:
            raise backend.BackendError(f"tracker reset: status {rc}: {self.last_error()}")

    def _arguments(self, left, right, delta_guess, outliers, n_outliers):
        """The arrays of a call, checked and contiguous: (left, right, guess or None, ids, n_outliers)."""
        f = self.flow
        imgs = []
        for im in (left, right):
            if im is None:
                imgs.append(None)
                continue
            im = np.ascontiguousarray(im)
            if im.dtype != np.uint8 or im.shape != (f.height, f.width):
                raise ValueError("images must be uint8 [height][width]")
            imgs.append(im)
        g = None
        if delta_guess is not None:
            g = np.ascontiguousarray(np.asarray(delta_guess, dtype=np.float64).reshape(-1)[:12])
        ids = np.ascontiguousarray(np.asarray(list(outliers), dtype=np.uint64))
        return imgs[0], imgs[1], g, ids, (len(ids) if n_outliers is None else int(n_outliers))

    def _unpack(self, res):
        counts = dict(covisible=res.n_covisible, new=res.n_new, word=res.n_words, blocked=res.n_blocked)
        out = dict(flags=res.flags, next_id=int(res.next_id))
        for name, width, dtype in _FIELDS:
            out[name] = self._take(res, name, counts[name.split("_")[0]], width, dtype)
        return out

    def process_status(self, left, right, delta_guess=None, outliers=(), n_outliers=None):
        """(status, result dict or None).  delta_guess: None or 3x4 (or 4x4) row-major; outliers: ids."""
        left, right, g, ids, n = self._arguments(left, right, delta_guess, outliers, n_outliers)
        res = Result()
        rc = self._lib.visfs_tracker_process(self.h, left.ctypes.data if left is not None else None,
                                             right.ctypes.data if right is not None else None, self.flow.width,
                                             g.ctypes.data_as(_pd) if g is not None else None, n,
                                             ids.ctypes.data_as(_pu64) if len(ids) else None, C.byref(res))
        if rc != abi.OK:
            return rc, None
        return rc, self._unpack(res)

    def process(self, left, right, delta_guess=None, outliers=()):
        rc, out = self.process_status(left, right, delta_guess, outliers)
        if rc != abi.OK:
            raise backend.BackendError(f"tracker process: status {rc}: {self.last_error()}")
        return out

    def download(self):
        """Intermediate state of the last call: dict(guess_xy, to_xy, lk_status, in_bounds per from-row; discs (DISC_DTYPE, draw
        order), disc_drawn; stereo_status per row of kept + new)."""
        m = int(self.params.max_features)
        guess = np.zeros((m, 2), dtype=np.float32); to = np.zeros((m, 2), dtype=np.float32)
        st = np.zeros(m, dtype=np.uint8); inb = np.zeros(m, dtype=np.uint8)
        discs = np.zeros(2 * m, dtype=_corners.DISC_DTYPE); drawn = np.zeros(2 * m, dtype=np.uint8)
        sst = np.zeros(m, dtype=np.uint8)
        nf, nd, nr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rc = self._lib.visfs_tracker_download(self.h, C.byref(nf), guess.ctypes.data_as(_pf), to.ctypes.data_as(_pf), st.ctypes.data_as(_pu8),
                                              inb.ctypes.data_as(_pu8), C.byref(nd), discs.ctypes.data, drawn.ctypes.data_as(_pu8),
                                              C.byref(nr), sst.ctypes.data_as(_pu8))
        if rc != abi.OK:
            raise backend.BackendError(f"tracker download: status {rc}: {self.last_error()}")
        return dict(guess_xy=guess[:nf.value].copy(), to_xy=to[:nf.value].copy(), lk_status=st[:nf.value].copy(),
                    in_bounds=inb[:nf.value].copy(), discs=discs[:nd.value].copy(), disc_drawn=drawn[:nd.value].copy(),
                    stereo_status=sst[:nr.value].copy())

    def download_cull(self):
        """The fundamental-matrix cull of the last call, as fund.Fund.cull and fund.Fund.download report it for the same from-rows:
        dict(applied, m, n_hypotheses, n_inliers, mask and status per from-row (status: after the AND), F, T1, T2 [3][3], winner
        (h, k)).  A tracker whose cull is inactive reports applied 0, m 0 and empty mask and status."""
        n = int(self.params.max_features)
        mask = np.zeros(n, dtype=np.uint8); status = np.zeros(n, dtype=np.uint8)
        F, T1, T2 = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
        ap, m, nh, ni, wh, wk, nf = (C.c_int32(0) for _ in range(7))
        rc = self._lib.visfs_tracker_download_cull(self.h, C.byref(ap), C.byref(m), C.byref(nh), C.byref(ni), mask.ctypes.data_as(_pu8),
                                                   status.ctypes.data_as(_pu8), F.ctypes.data_as(_pd), T1.ctypes.data_as(_pd),
                                                   T2.ctypes.data_as(_pd), C.byref(wh), C.byref(wk))
        if rc == abi.OK:
            rc = self._lib.visfs_tracker_download(self.h, C.byref(nf), None, None, None, None, None, None, None, None, None)
        if rc != abi.OK:
            raise backend.BackendError(f"tracker download_cull: status {rc}: {self.last_error()}")
        active = bool(self.params.cull) and not self.flow.params.flow_back
        rows = nf.value if active else 0
        return dict(applied=ap.value, m=m.value, n_hypotheses=nh.value, n_inliers=ni.value, mask=mask[:rows].copy(),
                    status=status[:rows].copy(), F=F, T1=T1, T2=T2, winner=(wh.value, wk.value))


def group_create_status(members):
    """(status, handle or None, error text) without raising: what the argument tests look at."""
    lib = load()
    arr = (C.c_void_p * max(len(members), 1))(*[m.h for m in members])
    h = C.c_void_p()
    rc = lib.visfs_tracker_group_create(len(members), arr, C.byref(h))
    return rc, (h if rc == abi.OK else None), lib.visfs_tracker_group_last_error(None).decode()


class TrackerGroup:
    """Several Trackers (each on a Flow of its own, all on one solver or all host twins, equal parameters and image size) processed by
    one call.  The members stay usable on their own and must stay open while the group is used."""

    def __init__(self, members):
        self._lib = load()
        self.members = list(members)
        rc, h, why = group_create_status(self.members)
        if rc != abi.OK:
            self.h = None
            raise backend.BackendError(f"visfs_tracker_group_create failed with status {rc}: {why}")
        self.h = h

    def close(self):
        if self.h:
            self._lib.visfs_tracker_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_tracker_group_last_error(self.h).decode()

    def last_counts(self):
        """dict(kernel_launches, copies_and_memsets, synchronisations) of the last process call; all zero for host twins."""
        k, c, s = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rc = self._lib.visfs_tracker_group_last_counts(self.h, C.byref(k), C.byref(c), C.byref(s))
        if rc != abi.OK:
            raise backend.BackendError(f"tracker group counts: status {rc}")
        return dict(kernel_launches=k.value, copies_and_memsets=c.value, synchronisations=s.value)

    def process_status(self, frames):
        """frames: per member (left, right[, delta_guess[, outliers[, n_outliers]]]).  (status, [result dict] or None)."""
        if len(frames) != len(self.members):
            raise ValueError("one frame per member")
        n = len(frames)
        arr, keep = (Frame * n)(), []
        for i, (m, fr) in enumerate(zip(self.members, frames)):
            fr = tuple(fr) + (None, (), None)[len(fr) - 2:]
            left, right, g, ids, n_out = m._arguments(*fr)
            keep.append((left, right, g, ids))
            arr[i].left = left.ctypes.data if left is not None else None
            arr[i].right = right.ctypes.data if right is not None else None
            arr[i].stride = m.flow.width
            arr[i].delta_guess = g.ctypes.data_as(_pd) if g is not None else None
            arr[i].n_outliers = n_out
            arr[i].outlier_ids = ids.ctypes.data_as(_pu64) if len(ids) else None
        res = (Result * n)()
        rc = self._lib.visfs_tracker_group_process(self.h, arr, res)
        if rc != abi.OK:
            return rc, None
        return rc, [m._unpack(res[i]) for i, m in enumerate(self.members)]

    def process(self, frames):
        rc, out = self.process_status(frames)
        if rc != abi.OK:
            raise backend.BackendError(f"tracker group process: status {rc}: {self.last_error()}")
        return out
