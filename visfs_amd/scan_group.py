"""ctypes binding of the scan stack group (include/visfs_scan_group.h, in libvisfs_ba_hip.so) — plumbing only.

`ScanStackGroup(stacks)` takes `scan_fast.ScanStack`s of one flavour (device stacks of one solver, or host twins) with equal
resolution and depth; `.match(guesses, points, **params)` matches one scan against all of them in one call and returns
(results, status, best_member); `.match_download(member)` and `.last_counts()` are the test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import scan_fast as sf

ABI_VERSION = 1
EXPORTS = [
    "visfs_scan_group_abi_version", "visfs_scan_group_create", "visfs_scan_group_destroy", "visfs_scan_group_last_error",
    "visfs_scan_group_match", "visfs_scan_group_match_download", "visfs_scan_group_last_counts",
]
MAX_MEMBERS = 64
MAX_FRONTIER = 1 << 26

_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    sf.load()
    lib = backend.load_library()
    lib.visfs_scan_group_abi_version.restype = C.c_int
    lib.visfs_scan_group_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.visfs_scan_group_create.restype = C.c_int
    lib.visfs_scan_group_destroy.argtypes = [C.c_void_p]
    lib.visfs_scan_group_destroy.restype = None
    lib.visfs_scan_group_last_error.argtypes = [C.c_void_p]
    lib.visfs_scan_group_last_error.restype = C.c_char_p
    lib.visfs_scan_group_match.argtypes = [C.c_void_p, C.POINTER(sf.Params), _pd, C.c_int32, _pd, C.POINTER(sf.Result), _pi32, _pi32]
    lib.visfs_scan_group_match.restype = C.c_int
    lib.visfs_scan_group_match_download.argtypes = [C.c_void_p, C.c_int32, _pi32, _pi32, _pi32, C.c_int64, _pi32, C.c_int64, _pi32]
    lib.visfs_scan_group_match_download.restype = C.c_int
    lib.visfs_scan_group_last_counts.argtypes = [C.c_void_p, _pi32, _pi32, _pi32]
    lib.visfs_scan_group_last_counts.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def create_error():
    """The reason of this thread's last failed create."""
    return load().visfs_scan_group_last_error(None).decode()


class ScanStackGroup:
    """A visfs_scan_group over the C ABI.  `status` is the constructor's return code; `h` is None when it failed (create_error()
    says why).  `stacks`: ScanStack objects (None stands for a NULL member); the group keeps them alive."""

    def __init__(self, stacks):
        self._lib = load()
        self.stacks = list(stacks)
        m = len(self.stacks)
        arr = (C.c_void_p * max(m, 1))(*[(s.h if s is not None else None) for s in self.stacks])
        h = C.c_void_p()
        self.status = self._lib.visfs_scan_group_create(m, arr, C.byref(h))
        self.h = h if self.status == abi.OK else None
        self.rc = self.status

    def close(self):
        if self.h:
            self._lib.visfs_scan_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._lib.visfs_scan_group_last_error(self.h).decode()

    def match(self, guesses, points, params=None, **kw):
        """visfs_scan_group_match: (results, status, best_member).  guesses [m][3] (or one guess for all), points [n][3] in the
        robot frame; the keywords are the fields of visfs_scan_stack_params (or `params`, a scan_fast.Params).  results[i] is
        member i's result dict, None where status[i] is not OK.  `self.rc` holds the call's return code; when it is not OK the
        three are None."""
        p = params if params is not None else sf.default_params(**kw)
        m = len(self.stacks)
        g = np.asarray(guesses, dtype=np.float64)
        if g.size == 3:
            g = np.tile(g.reshape(1, 3), (m, 1))
        g = np.ascontiguousarray(g.reshape(m, 3))
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        res = (sf.Result * m)()
        status = np.full(m, -1, dtype=np.int32)
        best = C.c_int32(-2)
        self.rc = self._lib.visfs_scan_group_match(self.h, C.byref(p), _ptr(g, C.c_double), len(pts), _ptr(pts, C.c_double), res,
                                                   _ptr(status, C.c_int32), C.byref(best))
        if self.rc != abi.OK:
            return None, None, None
        st = [int(v) for v in status]
        return [res[i].as_dict() if st[i] == abi.OK else None for i in range(m)], st, int(best.value)

    def match_download(self, member):
        """The hook of one member after a match, as ScanStack.match_download gives it; None when the member's status was not OK
        (or before any match)."""
        hdr = np.zeros(8, dtype=np.int32)
        scored = np.zeros(16, dtype=np.int32)
        kept = np.zeros(16, dtype=np.int32)
        rc = self._lib.visfs_scan_group_match_download(self.h, member, _ptr(hdr, C.c_int32), _ptr(scored, C.c_int32), _ptr(kept, C.c_int32), 0, None, 0, None)
        assert rc == abi.OK, (rc, self.last_error())
        S, L, n, H, per, m, B = (int(v) for v in hdr[:7])
        if S == 0:
            assert not hdr.any()
            return None
        bounds = np.zeros((S, per), dtype=np.int32)
        surv = np.zeros((m, 2), dtype=np.int32)
        rc = self._lib.visfs_scan_group_match_download(self.h, member, _ptr(hdr, C.c_int32), _ptr(scored, C.c_int32), _ptr(kept, C.c_int32),
                                                       bounds.size, _ptr(bounds, C.c_int32), m, _ptr(surv, C.c_int32))
        assert rc == abi.OK, (rc, self.last_error())
        return dict(S=S, L=L, n=n, H=H, B=B, scored=scored[:H + 1].tolist(), kept=kept[:H + 1].tolist(), bounds=bounds, survivors=surv)

    def last_counts(self):
        k, c, s = C.c_int32(), C.c_int32(), C.c_int32()
        rc = self._lib.visfs_scan_group_last_counts(self.h, C.byref(k), C.byref(c), C.byref(s))
        assert rc == abi.OK, rc
        return dict(kernel_launches=k.value, copies_and_memsets=c.value, synchronisations=s.value)
