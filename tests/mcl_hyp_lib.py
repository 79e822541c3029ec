"""The library behind the steps of tests/mcl_hyp_cases.py (a KLD filter with hypotheses, on the twin or on the device), and the
byte-for-byte comparisons that tests/test_mcl_hyp.py and tests/test_gpu_mcl_hyp.py share."""
import numpy as np

import mcl_cases as mc
import mcl_hyp_cases as hc
import mcl_hyp_oracle as ho
import mcl_kld_lib as kl

from visfs_amd import abi, mcl
from visfs_amd import mcl_hyp as hyp
from visfs_amd import mcl_kld as kld


def field_of(world, solver=None):
    """The library's field of a world: on the device with a solver, the twin's without."""
    (cells, lim), _ = hc.world(world)
    f = mcl.Field.from_grid(cells, lim, solver=solver) if solver is not None else mcl.Field.from_grid(cells, lim)
    assert f.status == abi.OK
    return f


class Library(kl.Library):
    """kl.Library with the hypotheses switched on (or left off)."""

    def __init__(self, case, field, hypotheses=True, **kw):
        super().__init__(case, field, **kw)
        self.on = hypotheses
        if hypotheses:
            assert hyp.enable(self.f) == abi.OK, self.f.last_error()
        self.rounds = []

    def snapshot(self):
        k, st = super().snapshot()
        if not self.on:
            assert hyp.last(self.f) == (abi.ERR_BAD_ARGUMENT, ho.no_hypotheses())
            return k, st, None, None
        rc, h = hyp.last(self.f)
        assert rc == abi.OK
        rc, lab = hyp.labels(self.f, h["n"])
        assert rc == (abi.OK if h["n_hypotheses"] else abi.ERR_BAD_ARGUMENT)
        self.rounds.append(hyp.rounds(self.f)[1])
        return k, st, h, lab


def pack(h):
    """The bytes of visfs_mcl_hyp_result that hold the dict h."""
    r = hyp.Result()
    for k in ("fresh", "n_clusters", "n_hypotheses", "n", "update"):
        setattr(r, k, h[k])
    for q, e in enumerate(h["hyp"]):
        for k in ("label", "count", "bins", "pad", "weight"):
            setattr(r.hyp[q], k, e[k])
        r.hyp[q].mean[:] = e["mean"]
        r.hyp[q].covariance[:] = e["covariance"]
    return bytes(r)


def same_trace(got, want, what=""):
    """Every update of two traces of hc.play(): both results, the state, every field of the hypotheses and the labels, byte for
    byte."""
    kl.same_trace([t[:3] for t in got], [t[:3] for t in want], what)
    for i, (a, b) in enumerate(zip(got, want)):
        assert pack(a[3]) == pack(b[3]), (what, i, a[3], b[3])
        kl.same(np.asarray(a[4], dtype=np.int32), np.asarray(b[4], dtype=np.int32), (what, i, "labels"))


def particles(rng, n):
    return kl.particles(rng, n)


def check_life_cycle(field):
    """Every refusal, enabling twice, and what removes the hypotheses."""
    rng = np.random.default_rng(4)
    N = 400
    f = mcl.Filter(field, N, 9)
    assert hyp.enable(f) == abi.ERR_BAD_ARGUMENT                              # a plain filter
    assert hyp.last(f) == (abi.ERR_BAD_ARGUMENT, ho.no_hypotheses()) and hyp.labels(f, 4)[0] == abi.ERR_BAD_ARGUMENT
    assert hyp.rounds(f)[0] == abi.ERR_BAD_ARGUMENT
    pts = mc.cloud(rng, 30)
    assert f.init(mc.ROOM_CENTRE, (0.05, 0.05, 0.02)) == abi.OK and f.update((0.1, 0.0, 0.02), pts)[0] == abi.OK       # still a plain filter
    assert kld.enable(f, min_particles=50, kld_err=0.05) == abi.OK
    assert hyp.last(f)[0] == abi.ERR_BAD_ARGUMENT                             # a KLD filter without hypotheses
    before = kld.download(f)
    assert hyp.enable(f) == abi.OK and hyp.last(f) == (abi.OK, ho.no_hypotheses())
    now = kld.download(f)
    for k in kl.STATE_KEYS:
        kl.same(now[k], before[k], k)                                         # enabling keeps the particles
    assert hyp.labels(f, 4)[0] == abi.ERR_BAD_ARGUMENT and hyp.rounds(f) == (abi.OK, 0)
    rc, r = f.update((0.1, 0.0, 0.02), pts)                                   # update 2 resamples
    assert rc == abi.OK and r["resampled"] == 1
    rc, h = hyp.last(f)
    assert rc == abi.OK and h["fresh"] == 1 and h["update"] == 2 and h["n"] == kld.count(f) and 1 <= h["n_hypotheses"] <= hyp.HYP_MAX
    assert hyp.labels(f, h["n"])[0] == abi.OK
    assert hyp.enable(f) == abi.OK and hyp.last(f) == (abi.OK, h)             # idempotent
    st, lab = kld.download(f), hyp.labels(f, h["n"])[1]

    def unchanged(want):
        assert hyp.last(f) == (abi.OK, want)
        kl.same(hyp.labels(f, want["n"])[1], lab)
        now = kld.download(f)
        for k in kl.STATE_KEYS:
            kl.same(now[k], st[k], k)

    assert f.update((float("nan"), 0, 0), pts)[0] == abi.ERR_BAD_ARGUMENT     # a refused update leaves everything
    unchanged(h)
    assert kld.enable(f, min_particles=0) == abi.ERR_BAD_ARGUMENT
    unchanged(h)
    x, y, yaw, w = particles(rng, 120)
    assert kld.upload(f, x, y, yaw, np.zeros(120)) == abi.ERR_BAD_ARGUMENT    # a refused upload too
    unchanged(h)
    rc, r = f.update((0.1, 0.0, 0.02), pts)                                   # update 3 does not resample: kept, no longer fresh
    assert rc == abi.OK and r["resampled"] == 0 and hyp.last(f) == (abi.OK, dict(h, fresh=0))
    kl.same(hyp.labels(f, h["n"])[1], lab)
    assert kld.enable(f, min_particles=60, kld_err=0.04) == abi.OK and hyp.last(f) == (abi.OK, dict(h, fresh=0))      # new KLD parameters keep them
    assert kld.upload(f, x, y, yaw, w) == abi.OK and hyp.last(f) == (abi.OK, ho.no_hypotheses())
    assert hyp.labels(f, 4)[0] == abi.ERR_BAD_ARGUMENT
    assert f.update((0.1, 0.0, 0.02), pts)[0] == abi.OK and hyp.last(f)[1]["fresh"] == 1 and hyp.last(f)[1]["update"] == 4
    assert f.upload(*particles(rng, N)) == abi.OK and hyp.last(f) == (abi.OK, ho.no_hypotheses())
    for _ in range(2):
        assert f.update((0.1, 0.0, 0.02), pts)[0] == abi.OK
    assert hyp.last(f)[1]["n_hypotheses"] >= 1
    assert f.init(mc.ROOM_CENTRE, (0.05, 0.05, 0.02)) == abi.OK and hyp.last(f) == (abi.OK, ho.no_hypotheses())
    f.close()
