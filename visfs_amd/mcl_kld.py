"""ctypes binding of the KLD-adaptive particle counts (include/visfs_mcl_kld.h, in libvisfs_ba_hip.so) — plumbing only.

Every function takes a `mcl.Filter`: `enable(f, ...)` makes it a KLD filter, `last(f)` and `count(f)` tell what the last update did
to the count, `download(f)` is `f.download()` cut to the active count.  `upload()`, `limits()`, `set_hash_bits()` and `hook_bins()` are the
test hooks.
"""
import ctypes as C

import numpy as np

from . import abi, backend
from . import mcl

ABI_VERSION = 1
EXPORTS = [
    "visfs_mcl_kld_abi_version", "visfs_mcl_kld_default_params", "visfs_mcl_kld_enable", "visfs_mcl_kld_last", "visfs_mcl_kld_count",
    "visfs_mcl_kld_upload", "visfs_mcl_kld_limits", "visfs_mcl_kld_hook_set_hash_bits", "visfs_mcl_kld_hook_bins",
]
MAX_PARTICLES = 16384
BIN_CLAMP = 1 << 24


class Params(C.Structure):
    _fields_ = [("min_particles", C.c_int32), ("kld_err", C.c_double), ("kld_z", C.c_double), ("bin_xy", C.c_double), ("bin_yaw", C.c_double)]


class Result(C.Structure):
    _fields_ = [("n_before", C.c_int32), ("n_after", C.c_int32), ("bins", C.c_int32), ("limit", C.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


_pd = C.POINTER(C.c_double)
_pi32 = C.POINTER(C.c_int32)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    mcl.load()
    lib = backend.load_library()
    lib.visfs_mcl_kld_abi_version.restype = C.c_int
    lib.visfs_mcl_kld_default_params.argtypes = [C.POINTER(Params)]
    lib.visfs_mcl_kld_default_params.restype = None
    lib.visfs_mcl_kld_enable.argtypes = [C.c_void_p, C.POINTER(Params)]
    lib.visfs_mcl_kld_enable.restype = C.c_int
    lib.visfs_mcl_kld_last.argtypes = [C.c_void_p, C.POINTER(Result)]
    lib.visfs_mcl_kld_last.restype = C.c_int
    lib.visfs_mcl_kld_count.argtypes = [C.c_void_p]
    lib.visfs_mcl_kld_count.restype = C.c_int32
    lib.visfs_mcl_kld_upload.argtypes = [C.c_void_p, C.c_int32, _pd, _pd, _pd, _pd]
    lib.visfs_mcl_kld_upload.restype = C.c_int
    lib.visfs_mcl_kld_limits.argtypes = [C.c_void_p, _pi32]
    lib.visfs_mcl_kld_limits.restype = C.c_int
    lib.visfs_mcl_kld_hook_set_hash_bits.argtypes = [C.c_void_p, C.c_int32]
    lib.visfs_mcl_kld_hook_set_hash_bits.restype = C.c_int
    lib.visfs_mcl_kld_hook_bins.argtypes = [C.c_int32, _pd, C.c_double, _pi32]
    lib.visfs_mcl_kld_hook_bins.restype = C.c_int
    for name in EXPORTS:
        getattr(lib, name)
    _lib = lib
    return lib


def default_params(**kw):
    """The header's defaults (the shipped amcl.yaml's values and AMCL's histogram), with keyword overrides."""
    p = Params()
    load().visfs_mcl_kld_default_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def enable(f, params=None, **kw):
    """Makes the mcl.Filter `f` a KLD filter (or replaces its parameters); the status."""
    p = params if params is not None else default_params(**kw)
    return load().visfs_mcl_kld_enable(f.h, C.byref(p))


def last(f):
    """(status, dict of n_before, n_after, bins, limit) of the last update."""
    r = Result()
    rc = load().visfs_mcl_kld_last(f.h, C.byref(r))
    return rc, r.as_dict()


def count(f):
    return load().visfs_mcl_kld_count(f.h)


def upload(f, x, y, yaw, w):
    """Replaces the particles by len(x) of them, 1 .. N, which becomes the active count; the status."""
    a = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (x, y, yaw, w)]
    assert all(len(v) == len(a[0]) for v in a)
    return load().visfs_mcl_kld_upload(f.h, len(a[0]), *[v.ctypes.data_as(_pd) for v in a])


def limits(f):
    """limit [N + 1] int32 as the filter holds it."""
    out = np.zeros(f.n + 1, dtype=np.int32)
    rc = load().visfs_mcl_kld_limits(f.h, out.ctypes.data_as(_pi32))
    assert rc == abi.OK, f.last_error()
    return out


def set_hash_bits(f, bits):
    return load().visfs_mcl_kld_hook_set_hash_bits(f.h, bits)


def download(f):
    """f.download() cut to the active count: x, y, yaw, w, Q and ancestors, each [n]."""
    n = count(f)
    return {k: v[:n].copy() for k, v in f.download().items()}


def hook_bins(v, size):
    """(status, floor(v / size) clamped to +-2^24 as the filter forms it, int32)."""
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    out = np.zeros(len(a), dtype=np.int32)
    rc = load().visfs_mcl_kld_hook_bins(len(a), a.ctypes.data_as(_pd), size, out.ctypes.data_as(_pi32))
    return rc, out
