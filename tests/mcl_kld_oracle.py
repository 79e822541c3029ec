"""An independent checker of the KLD-adaptive particle counts, written from the definition on top of the
checker of tests/mcl_oracle.py: an update of the n active particles is that checker's update of a filter of n particles up to the
resampling; the resampling is the sequential loop as written: draw, insert the bin into a Python set of integer triples, stop
once the draw count exceeds the limit of the bin count.  It takes nothing from the library."""
import bisect
import math

import numpy as np

import mcl_oracle as mo

KLD_DEFAULTS = dict(min_particles=100, kld_err=0.01, kld_z=0.99, bin_xy=0.5, bin_yaw=math.pi / 18)
BIN_CLAMP = 1 << 24
DRAW = 3                                      # the motion uses draws 0 .. 2, the plain comb particle N with draw 0
NEVER = 1 << 62                               # an interval that no update counter is a multiple of: the base class never resamples


def limit_table(N, min_particles, kld_err, kld_z, **_):
    """limit[0 .. N] in Python floats, in the order the definition gives."""
    out = []
    for k in range(N + 1):
        if k <= 1:
            out.append(N)
            continue
        b = 2.0 / (9.0 * (k - 1))
        c = math.sqrt(b) * kld_z
        x = 1.0 - b + c
        v = math.ceil((k - 1) / (2.0 * kld_err) * x * x * x)
        out.append(min(max(v, min_particles), N))
    return np.array(out, dtype=np.int32)


def bin_index(v, size):
    q = math.floor(v / size)                  # one IEEE division, then the floor (exact, as an integer)
    return max(-BIN_CLAMP, min(BIN_CLAMP, q))


class KldFilter(mo.Filter):
    """The KLD filter of capacity N.  `n` is the active count; Q and the ancestors are kept at the capacity, as the library keeps
    them: an update writes the entries of its particles, state() hands out the first n."""

    def __init__(self, t, q, T, res, max_x, max_y, n_particles, seed, **kld):
        self.cap = n_particles
        self.kld = dict(KLD_DEFAULTS, **kld)
        self.limit = limit_table(n_particles, **self.kld)
        self.last = None
        super().__init__(t, q, T, res, max_x, max_y, n_particles, seed)

    def enable(self, **kld):
        self.kld = dict(KLD_DEFAULTS, **kld)
        self.limit = limit_table(self.cap, **self.kld)

    @property
    def n(self):
        return len(self.x)

    def init(self, mean, sigma):
        self.N = self.cap
        super().init(mean, sigma)
        self.Q_cap = self.Q.copy()
        self.anc_cap = self.ancestors.copy()

    def upload(self, x, y, yaw, w):
        self.x, self.y, self.yaw, self.w = (np.array(v, dtype=np.float64) for v in (x, y, yaw, w))
        assert 1 <= len(self.x) <= self.cap

    def state(self):
        n = self.n
        return dict(x=self.x, y=self.y, yaw=self.yaw, w=self.w, Q=self.Q_cap[:n].copy(), ancestors=self.anc_cap[:n].copy())

    def update(self, odom_delta, points_xyz, **kw):
        p = dict(mo.FILTER_DEFAULTS, **kw)
        n = self.n
        self.N = n                                                          # the plain update of a filter of n particles ...
        res = super().update(odom_delta, points_xyz, **dict(kw, resample_interval=NEVER))
        self.N = self.cap
        assert res["resampled"] == 0
        u = self.update_count
        self.Q_cap[:n] = self.Q
        self.anc_cap[:n] = self.ancestors                                  # the indices
        self.last = dict(n_before=n, n_after=n, bins=0, limit=0)
        if not (u % p["resample_interval"] == 0 and res["n_eff"] < p["n_eff_ratio"] * float(n)):       # ... up to the gate
            return res
        k = [int(math.floor(v * mo.TWO40)) for v in self.w.tolist()]
        C = [0] * n
        for j in range(1, n):
            C[j] = C[j - 1] + k[j - 1]
        K = C[-1] + k[-1]
        seen, anc = set(), []
        for i in range(self.cap):
            uu = mo.key_int(self.seed, u, i, DRAW) % K
            a = bisect.bisect_right(C, uu) - 1
            assert C[a] <= uu < C[a] + k[a]
            anc.append(a)
            seen.add((bin_index(float(self.x[a]), self.kld["bin_xy"]), bin_index(float(self.y[a]), self.kld["bin_xy"]),
                      bin_index(float(self.yaw[a]), self.kld["bin_yaw"])))
            if len(anc) > int(self.limit[len(seen)]):
                break
        m = len(anc)
        ia = np.array(anc, dtype=np.int64)
        self.x, self.y, self.yaw, self.w = self.x[ia], self.y[ia], self.yaw[ia], np.full(m, 1.0 / m)
        self.anc_cap[:m] = ia
        self.last = dict(n_before=n, n_after=m, bins=len(seen), limit=int(self.limit[len(seen)]))
        res["resampled"] = 1
        return res
