"""The library behind the steps of tests/mcl_kld_cases.py (a mcl.Filter made a KLD filter, on the twin or on the device), and the
byte-for-byte comparisons that tests/test_mcl_kld.py and tests/test_gpu_mcl_kld.py share."""
import numpy as np

import mcl_cases as mc
import mcl_kld_oracle as ko

from visfs_amd import abi, mcl
from visfs_amd import mcl_kld as kld

STATE_KEYS = ("x", "y", "yaw", "w", "Q", "ancestors")
RESULT_KEYS = ("status", "resampled", "best", "n_beams", "update", "mean", "covariance", "n_eff", "W", "best_pose", "best_weight")
KLD_KEYS = ("n_before", "n_after", "bins", "limit")


class Library:
    """A KLD filter of the library on `field` (its flavour decides twin or device)."""

    def __init__(self, case, field, hash_bits=None, lanes=None):
        self.f = mcl.Filter(field, case["N"], case["seed"])
        assert self.f.status == abi.OK
        assert kld.enable(self.f, **case["kld"]) == abi.OK, self.f.last_error()
        if hash_bits is not None:
            assert kld.set_hash_bits(self.f, hash_bits) == abi.OK
        if lanes is not None:
            assert self.f.set_lanes(lanes) == abi.OK
        self.counts = []

    def init(self, mean, sigma):
        assert self.f.init(mean, sigma) == abi.OK, self.f.last_error()

    def upload(self, x, y, yaw, w):
        assert kld.upload(self.f, x, y, yaw, w) == abi.OK, self.f.last_error()

    def update(self, delta, pts, params):
        rc, r = self.f.update(delta, pts, mcl.default_params(**params))
        assert rc == abi.OK, self.f.last_error()
        assert self.f.last_result() == (abi.OK, r)
        self.counts.append(self.f.last_counts())
        return r

    def snapshot(self):
        rc, k = kld.last(self.f)
        assert rc == abi.OK and kld.count(self.f) == k["n_after"]
        return k, kld.download(self.f)

    def limits(self):
        return kld.limits(self.f)

    def close(self):
        self.f.close()


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_result(got, want, what=""):
    for k in RESULT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            assert a.astype(np.float64).tobytes() == b.astype(np.float64).tobytes(), (what, k, got[k], want[k])
        else:
            assert np.array_equal(a, b), (what, k, got[k], want[k])


def same_trace(got, want, what=""):
    """Every update of two traces of play(): both results and the state, byte for byte."""
    assert len(got) == len(want)
    for i, ((ra, ka, sa), (rb, kb, sb)) in enumerate(zip(got, want)):
        same_result(ra, rb, (what, i))
        assert {k: ka[k] for k in KLD_KEYS} == {k: kb[k] for k in KLD_KEYS}, (what, i, ka, kb)
        for k in STATE_KEYS:
            same(sa[k], np.asarray(sb[k]), (what, i, k))


# ---------------------------------------------------------------- beside the plain filter, and the life cycle: on either flavour
def particles(rng, n):
    return 3.0 + rng.random(n), 3.2 + rng.random(n), rng.random(n) - 0.5, rng.random(n) + 0.05


def plain_and_kld(field, n=77, cap=300, seed=5):
    rng = np.random.default_rng(9)
    x, y, yaw, w = particles(rng, n)
    a, b = mcl.Filter(field, cap, seed), mcl.Filter(field, n, seed)
    assert kld.enable(a) == abi.OK and kld.upload(a, x, y, yaw, w) == abi.OK and b.upload(x, y, yaw, w) == abi.OK
    assert kld.count(a) == n and kld.count(b) == n
    return a, b, mc.cloud(rng, 40)


def check_plain_equality(field):
    """A KLD filter of capacity 300 that holds 77 particles and a plain filter of 77: one update with the gate closed."""
    a, b, pts = plain_and_kld(field)
    (rca, ra), (rcb, rb) = a.update((0.1, 0.01, 0.03), pts), b.update((0.1, 0.01, 0.03), pts)
    assert rca == rcb == abi.OK and ra["resampled"] == 0 and ra["update"] == 1
    same_result(ra, rb)
    sa, sb = kld.download(a), b.download()
    for k in STATE_KEYS:
        same(sa[k], sb[k], k)
    assert kld.last(a) == (abi.OK, dict(n_before=77, n_after=77, bins=0, limit=0)) and kld.last(b)[0] == abi.ERR_BAD_ARGUMENT
    assert (sa["ancestors"] == np.arange(77)).all() and sa["Q"].any()          # the closed gate: n stays, the ancestors are the indices
    assert a.last_counts() == b.last_counts()
    a.close(); b.close()


def check_life_cycle(field):
    rng = np.random.default_rng(3)
    N = 400
    f = mcl.Filter(field, N, 8)
    x, y, yaw, w = particles(rng, 120)
    assert kld.upload(f, x, y, yaw, w) == abi.ERR_BAD_ARGUMENT and kld.count(f) == N       # no KLD filter yet
    assert kld.set_hash_bits(f, 2) == abi.ERR_BAD_ARGUMENT
    assert f.init(mc.ROOM_CENTRE, (0.05, 0.05, 0.02)) == abi.OK
    before = f.download()
    assert kld.enable(f, min_particles=50, kld_err=0.05) == abi.OK and kld.count(f) == N      # the particles, the counter and n are kept
    for k in STATE_KEYS:
        same(kld.download(f)[k], before[k], k)
    pts = mc.cloud(rng, 30)
    counts = []
    for _ in range(4):
        assert f.update((0.1, 0.0, 0.02), pts)[0] == abi.OK
        counts.append(kld.count(f))
    assert counts[0] == N and counts[1] < N and counts[2] == counts[1] and kld.last(f)[1]["n_before"] == counts[2]
    st, last, res, lim = kld.download(f), kld.last(f), f.last_result(), kld.limits(f)
    n = kld.count(f)

    def unchanged():
        assert kld.count(f) == n and kld.last(f) == last and f.last_result() == res
        same(kld.limits(f), lim)
        now = kld.download(f)
        for k in STATE_KEYS:
            same(now[k], st[k], k)

    assert f.update((float("nan"), 0, 0), pts)[0] == abi.ERR_BAD_ARGUMENT
    unchanged()
    for bad in (dict(min_particles=0), dict(min_particles=N + 1), dict(kld_err=0.0), dict(kld_err=1.0), dict(kld_err=float("nan")), dict(kld_z=-1.0),
                dict(kld_z=float("inf")), dict(bin_xy=0.0), dict(bin_yaw=float("nan")), dict(bin_yaw=-0.1)):
        p = dict(ko.KLD_DEFAULTS, min_particles=50)
        p.update(bad)
        assert kld.enable(f, **p) == abi.ERR_BAD_ARGUMENT, bad
        unchanged()
    bad_w = np.zeros(120)
    assert kld.upload(f, x, y, yaw, bad_w) == abi.ERR_BAD_ARGUMENT
    assert kld.upload(f, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)) == abi.ERR_BAD_ARGUMENT
    big = np.full(N + 1, 1.0)
    assert kld.upload(f, big, big, big * 0.1, big) == abi.ERR_BAD_ARGUMENT
    unchanged()
    assert kld.enable(f, min_particles=60, kld_err=0.04) == abi.OK and kld.count(f) == n      # again: new parameters, the rest kept
    same(kld.limits(f), ko.limit_table(N, **dict(ko.KLD_DEFAULTS, min_particles=60, kld_err=0.04)))
    assert kld.upload(f, x, y, yaw, w) == abi.OK and kld.count(f) == 120 and len(kld.download(f)["x"]) == 120
    same(kld.download(f)["yaw"], yaw)
    full = particles(rng, N)
    assert f.upload(*full) == abi.OK and kld.count(f) == N                     # the plain upload returns n to N
    same(kld.download(f)["w"], full[3])
    assert kld.upload(f, x, y, yaw, w) == abi.OK and kld.count(f) == 120
    assert f.init(mc.ROOM_CENTRE, (0.05, 0.05, 0.02)) == abi.OK and kld.count(f) == N            # ... and so does init
    now = kld.download(f)
    for k in STATE_KEYS:
        same(now[k], before[k], k)
    f.close()
