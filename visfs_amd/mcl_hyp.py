"""ctypes binding of AMCL's pose hypotheses on the KLD filter (include/visfs_mcl_hyp.h, in libvisfs_ba_hip.so) — plumbing only.

Every function takes a `mcl.Filter` that `mcl_kld.enable()` made a KLD filter: `enable(f)` switches the hypotheses on, `last(f)` gives
those of the last resampling.  `labels()` and `rounds()` are the test hooks.
"""
import ctypes as C

import numpy as np

from . import backend
from . import mcl_kld

ABI_VERSION = 1
EXPORTS = ["visfs_mcl_hyp_abi_version", "visfs_mcl_hyp_enable", "visfs_mcl_hyp_last", "visfs_mcl_hyp_download_labels", "visfs_mcl_hyp_hook_rounds"]
HYP_MAX = 8


class Hypothesis(C.Structure):
    _fields_ = [("label", C.c_int32), ("count", C.c_int32), ("bins", C.c_int32), ("pad", C.c_int32), ("weight", C.c_double),
                ("mean", C.c_double * 3), ("covariance", C.c_double * 9)]

    def as_dict(self):
        return dict(label=self.label, count=self.count, bins=self.bins, pad=self.pad, weight=self.weight, mean=list(self.mean),
                    covariance=list(self.covariance))


class Result(C.Structure):
    _fields_ = [("fresh", C.c_int32), ("n_clusters", C.c_int32), ("n_hypotheses", C.c_int32), ("n", C.c_int32), ("update", C.c_int64),
                ("hyp", Hypothesis * HYP_MAX)]

    def as_dict(self):
        return dict(fresh=self.fresh, n_clusters=self.n_clusters, n_hypotheses=self.n_hypotheses, n=self.n, update=self.update,
                    hyp=[h.as_dict() for h in self.hyp])


_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    mcl_kld.load()
    lib = backend.load_library()
    lib.visfs_mcl_hyp_abi_version.restype = C.c_int
    lib.visfs_mcl_hyp_enable.argtypes = [C.c_void_p]
    lib.visfs_mcl_hyp_enable.restype = C.c_int
    lib.visfs_mcl_hyp_last.argtypes = [C.c_void_p, C.POINTER(Result)]
    lib.visfs_mcl_hyp_last.restype = C.c_int
    lib.visfs_mcl_hyp_download_labels.argtypes = [C.c_void_p, _pi32]
    lib.visfs_mcl_hyp_download_labels.restype = C.c_int
    lib.visfs_mcl_hyp_hook_rounds.argtypes = [C.c_void_p, _pi32]
    lib.visfs_mcl_hyp_hook_rounds.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def enable(f):
    """Switches the hypotheses of the KLD filter `f` on; the status."""
    return load().visfs_mcl_hyp_enable(f.h)


def last(f):
    """(status, dict of fresh, n_clusters, n_hypotheses, n, update and hyp, a list of HYP_MAX dicts) of the last resampling."""
    r = Result()
    rc = load().visfs_mcl_hyp_last(f.h, C.byref(r))
    return rc, r.as_dict()


def last_bytes(f):
    """(status, the bytes of visfs_mcl_hyp_result)."""
    r = Result()
    rc = load().visfs_mcl_hyp_last(f.h, C.byref(r))
    return rc, bytes(r)


def labels(f, n):
    """(status, label [n] int32 of the last resampling); n is its n_after."""
    out = np.zeros(max(n, 1), dtype=np.int32)
    rc = load().visfs_mcl_hyp_download_labels(f.h, out.ctypes.data_as(_pi32))
    return rc, out[:n]


def rounds(f):
    """(status, the propagation rounds of the last device resampling)."""
    v = C.c_int32(0)
    rc = load().visfs_mcl_hyp_hook_rounds(f.h, C.byref(v))
    return rc, v.value
