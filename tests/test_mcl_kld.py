"""KLD-adaptive particle counts (include/visfs_mcl_kld.h) on the CPU: the one-core host twin against the
checker of tests/mcl_kld_oracle.py, byte for byte in the particles (the first n), Q, the ancestors, every field of both results and
the limit table, on the cases of tests/mcl_kld_cases.py.  Before the library is compared, the checker's output alone must show
that each case does what its name says.  tests/test_gpu_mcl_kld.py holds the device to the twin."""
import functools
import math

import numpy as np
import pytest

import mcl_cases as mc
import mcl_kld_cases as kc
import mcl_kld_lib as kl
import mcl_kld_oracle as ko
from visfs_amd import abi, mcl
from visfs_amd import mcl_kld as kld

SIZE_CASES = kc.size_cases()
CRAFTED = kc.crafted_cases()


@functools.lru_cache(maxsize=None)
def room_twin():
    cells, lim = mc.room()
    f = mcl.Field.from_grid(cells, lim)
    assert f.status == abi.OK
    return f


def twin_trace(case, **kw):
    lib = kl.Library(case, room_twin(), **kw)
    same_limits(lib, case)
    out = kc.play(case, lib)
    assert lib.counts and all(c == (0, 0, 0) for c in lib.counts)             # the twin issues nothing
    lib.close()
    return out


def same_limits(lib, case):
    kl.same(lib.limits(), ko.limit_table(case["N"], **case["kld"]), "limit")


# ---------------------------------------------------------------- the limit table
def test_limit_table_known_answers():
    t = ko.limit_table(3000, 100, 0.01, 0.99)
    assert t.dtype == np.int32 and len(t) == 3001
    want = {0: 3000, 1: 3000, 2: 100, 3: 182, 4: 257, 5: 327, 8: 525, 16: 1014, 32: 1935, 64: 3000, 1000: 3000, 3000: 3000}
    assert {k: int(t[k]) for k in want} == want and (t[64:] == 3000).all()
    f = mcl.Filter(room_twin(), 3000, 1)
    assert kld.enable(f) == abi.OK
    kl.same(kld.limits(f), t)
    assert kld.load().visfs_mcl_kld_abi_version() == kld.ABI_VERSION == 1 and mcl.load().visfs_mcl_abi_version() == 1
    p = kld.default_params()
    assert (p.min_particles, p.kld_err, p.kld_z, p.bin_xy, p.bin_yaw) == (100, 0.01, 0.99, 0.5, ko.KLD_DEFAULTS["bin_yaw"])
    f.close()


@pytest.mark.parametrize("kw", [dict(min_particles=1, kld_err=0.3, kld_z=2.5), dict(min_particles=700, kld_err=0.002, kld_z=0.5),
                                dict(min_particles=5, kld_err=0.999, kld_z=1e-3)], ids=["loose", "tight", "edge"])
def test_limit_table_twin_equals_checker(kw):
    for N in (1, 2, 700, 4097):
        f = mcl.Filter(room_twin(), N, 1)
        p = dict(ko.KLD_DEFAULTS, **kw)
        p["min_particles"] = min(N, p["min_particles"])
        assert kld.enable(f, **p) == abi.OK
        kl.same(kld.limits(f), ko.limit_table(N, **p), (N, kw))
        f.close()


def test_the_bin_function_at_its_edges():
    """floor(v / size) as the filter forms it against the checker's, on the poses of the edge case and beyond what an upload takes:
    +-1e12 (the clamp sends them to two different bins), +-2^24 bins exactly, the doubles beside them."""
    assert kc.bins_of(dict(x=[p[0] for p in kc.EDGE_POSES], y=[p[1] for p in kc.EDGE_POSES], yaw=[p[2] for p in kc.EDGE_POSES]),
                      ko.KLD_DEFAULTS) == kc.EDGE_BINS
    assert (ko.bin_index(1e12, 0.5), ko.bin_index(-1e12, 0.5)) == (1 << 24, -(1 << 24))
    rng = np.random.default_rng(2)
    for size in (0.5, math.pi / 18, 0.1, 3.0):
        edge = size * float(1 << 24)
        v = np.concatenate([[1e12, -1e12, 1e300, -1e300, 0.0, -0.0, 5e-324, -5e-324, edge, -edge, math.nextafter(edge, 0.0), math.nextafter(-edge, 0.0),
                             math.nextafter(edge, math.inf), math.nextafter(-edge, -math.inf)],
                            size * np.arange(-40, 41), np.nextafter(size * np.arange(-40, 41), -np.inf), np.nextafter(size * np.arange(-40, 41), np.inf),
                            [p[k] for p in kc.EDGE_POSES for k in range(3)], 50.0 * rng.normal(size=500), 1e8 * rng.normal(size=100)])
        rc, got = kld.hook_bins(v, size)
        assert rc == abi.OK
        kl.same(got, np.array([ko.bin_index(float(a), size) for a in v], dtype=np.int32), size)
        assert got[0] == 1 << 24 and got[1] == -(1 << 24) and got[0] != got[1]
    assert kld.hook_bins([float("nan")], 0.5)[0] == abi.ERR_BAD_ARGUMENT and kld.hook_bins([1.0], 0.0)[0] == abi.ERR_BAD_ARGUMENT


# ---------------------------------------------------------------- sizes
@pytest.mark.parametrize("case", SIZE_CASES, ids=[c["name"] for c in SIZE_CASES])
def test_sizes_twin_equals_checker(case):
    ref = kc.reference(case["name"])
    N = case["N"]
    assert [r["resampled"] for r, _, _ in ref] == ([0, 1] * 3 if N > 1 else [0] * 6)
    assert all(k["n_before"] == len(st["x"]) == k["n_after"] for r, k, st in ref if not r["resampled"])
    if N >= 1023:                                                              # the count moved, and updates ran at a count below N
        assert ref[1][1]["n_after"] < N and ref[2][1]["n_before"] == ref[1][1]["n_after"] and ref[3][1]["n_before"] < N
        assert len({k["n_after"] for _, k, _ in ref}) >= 2
    kl.same_trace(twin_trace(case), ref, case["name"])


def test_the_fullest_table_and_the_capacity_above_it():
    case = kc.fullest_case()
    ref = kc.reference(case["name"])
    (_, k0, _), (r, k, st) = ref
    assert k0 == dict(n_before=16384, n_after=16384, bins=0, limit=0) and r["resampled"] == 1
    assert k["n_before"] == 16384 and k["bins"] > 2000 and len(st["x"]) == k["n_after"]       # thousands of bins in the table
    kl.same_trace(twin_trace(case), ref, case["name"])
    f = mcl.Filter(room_twin(), 16385, 1)
    assert f.status == abi.OK and kld.enable(f) == abi.ERR_UNSUPPORTED and kld.count(f) == 16385
    assert kld.last(f)[0] == abi.ERR_BAD_ARGUMENT and f.update((0.1, 0, 0), mc.cloud(np.random.default_rng(1), 5))[0] == abi.OK    # still a plain filter
    f.close()


# ---------------------------------------------------------------- the crafted sets
@pytest.mark.parametrize("case", CRAFTED, ids=[c["name"] for c in CRAFTED])
def test_crafted_twin_equals_checker(case):
    kc.check_crafted(case["name"])
    kl.same_trace(twin_trace(case), kc.reference(case["name"]), case["name"])


def test_hash_bits_and_lanes_leave_the_twin_alone():
    case = SIZE_CASES[-1]
    assert case["N"] == 1025
    ref = kc.reference(case["name"])
    for kw in (dict(hash_bits=0), dict(hash_bits=3), dict(lanes=1), dict(lanes=64)):
        kl.same_trace(twin_trace(case, **kw), ref, kw)


# ---------------------------------------------------------------- beside the plain filter
def test_a_kld_filter_of_77_equals_a_plain_filter_of_77():
    kl.check_plain_equality(room_twin())


def test_life_cycle_on_the_twin():
    kl.check_life_cycle(room_twin())


# ---------------------------------------------------------------- it localises, with fewer particles at the end
# The checker's final pose error (metres, radians) and its counts after the first and the last resampling on the scene of
# tests/mcl_cases.py with N = 3000 and the reference's settings, seeds 1 .. 5, measured on the CPU; the test holds the checker, and
# so the twin that equals it, to three times the worst of the errors.
MEASURED = [(0.0544, 0.0193, 3000, 1366), (0.0659, 0.0192, 3000, 1308), (0.0567, 0.0151, 3000, 1710), (0.0564, 0.0247, 3000, 1596),
            (0.0712, 0.0181, 3000, 1366)]
LOCALISE_BOUND = (3.0 * max(e[0] for e in MEASURED), 3.0 * max(e[1] for e in MEASURED))


def test_it_localises_and_the_count_falls():
    s = mc.localisation_scene()
    for seed in kc.LOCALISE_SEEDS:
        ref = kc.localise_reference(seed)
        ran = [k for r, k, _ in ref if r["resampled"]]
        et, er = mc.pose_error(ref[-1][0]["mean"], s["poses"][-1])
        print(f"seed {seed}: final error {et:.4f} m, {er:.4f} rad; counts {[k['n_after'] for k in ran]}; bins {[k['bins'] for k in ran]}")
        assert len(ran) == 10 and ran[0]["n_before"] == 3000
        assert ran[0]["n_after"] == 3000                                       # the belief is wide: the first resampling keeps all
        assert ran[-1]["n_after"] < 3000                                       # ... and it has narrowed at the end
        assert et <= LOCALISE_BOUND[0] and er <= LOCALISE_BOUND[1], (seed, et, er)
    case = kc.localise_case(1)
    kl.same_trace(twin_trace(case), kc.localise_reference(1), "seed 1")
