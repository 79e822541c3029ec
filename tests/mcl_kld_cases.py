"""The cases of the KLD-adaptive particle counts (tests/test_mcl_kld.py on the CPU, tests/test_gpu_mcl_kld.py on the device), on the
room of tests/mcl_cases.py.  A case is a filter (N, seed, KLD parameters) and a list of steps: ("init", mean, sigma),
("upload", x, y, yaw, w) with any count 1 .. N, ("update", delta, points, filter parameters).  play() runs one on anything that has
those three methods plus snapshot(); Checker is the checker of tests/mcl_kld_oracle.py behind them.  Nothing here calls the
library."""
import functools
import math

import numpy as np

import mcl_cases as mc
import mcl_kld_oracle as ko
import mcl_oracle as mo

ZERO = dict(alpha1=0.0, alpha2=0.0, alpha3=0.0, alpha4=0.0)
OPEN = dict(ZERO, resample_interval=1, n_eff_ratio=2.0)     # n_eff <= n < 2 n: the gate is open at every update
STILL = (0.0, 0.0, 0.0)
NO_POINTS = np.zeros((0, 3))
TWO40 = 1 << 40


class Checker:
    def __init__(self, case):
        t, q, _, T, _ = mc.room_field()
        _, lim = mc.room()
        self.f = ko.KldFilter(t, q, T, lim["resolution"], lim["max_x"], lim["max_y"], case["N"], case["seed"], **case["kld"])

    def init(self, mean, sigma):
        self.f.init(mean, sigma)

    def upload(self, x, y, yaw, w):
        self.f.upload(x, y, yaw, w)

    def update(self, delta, pts, params):
        return self.f.update(delta, pts, **params)

    def snapshot(self):
        """(the last KLD result, the state cut to n)."""
        return dict(self.f.last), {k: np.array(v) for k, v in self.f.state().items()}

    def limits(self):
        return self.f.limit


def play(case, flt):
    """[(result, kld result, state)] after every update of the case."""
    out = []
    for step in case["steps"]:
        if step[0] == "init":
            flt.init(step[1], step[2])
        elif step[0] == "upload":
            flt.upload(*step[1:])
        else:
            r = flt.update(step[1], step[2], step[3])
            out.append((r,) + flt.snapshot())
    return out


def case(name, N, seed, steps, **kld):
    return dict(name=name, N=N, seed=seed, steps=steps, kld=dict(ko.KLD_DEFAULTS, **kld))


# ---------------------------------------------------------------- runs in the room
def room_run(name, N, n_beams, seed, updates, sigma=(0.25, 0.25, 0.15), params=None, **kld):
    rng = np.random.default_rng(seed)
    d = mc.deltas(rng, max(updates, 7))[:updates]
    steps = [("init", mc.ROOM_CENTRE, sigma)]
    steps += [("update", d[k], mc.cloud(rng, n_beams), dict(params or {})) for k in range(updates)]
    return case(name, N, 0xBEEF + seed, steps, **kld)


SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def size_cases():
    """Six updates with 30 beams: three resamplings.  kld_err = 0.05 lets the count move at these sizes."""
    return [room_run(f"N{N}_n30", N, 30, N, 6, min_particles=max(1, N // 8), kld_err=0.05) for N in SIZES]


@functools.lru_cache(maxsize=None)
def fullest_case():
    """N = 16384: the table has its 32768 slots; a wide belief and small bins give it thousands of bins.  One resampling."""
    return room_run("N16384_n30", 16384, 30, 77, 2, sigma=(1.0, 1.0, 1.0), min_particles=100, kld_err=0.01, bin_xy=0.1, bin_yaw=0.05)


# ---------------------------------------------------------------- crafted particle sets: one update, no motion, no beams, the gate open
def crafted(name, N, seed, x, y, yaw, w, params=OPEN, **kld):
    x, y, yaw, w = (np.asarray(v, dtype=np.float64) for v in (x, y, yaw, w))
    steps = [("init", mc.ROOM_CENTRE, (0.0, 0.0, 0.0)), ("upload", x, y, yaw, w), ("update", STILL, NO_POINTS, dict(params))]
    return case(name, N, seed, steps, **kld)


def one_bin():
    N = 300
    rng = np.random.default_rng(1)
    return crafted("one_bin", N, 31, 3.0 + 0.49 * rng.random(N), 3.0 + 0.49 * rng.random(N), 0.17 * rng.random(N), rng.random(N) + 0.1)


def own_bins():
    N = 300
    j = np.arange(N)
    return crafted("own_bins", N, 32, 0.25 + 0.5 * (j % 20), 0.25 + 0.5 * (j // 20), np.full(N, 0.05), np.full(N, 1.0 / N))


def two_bins():
    N = 3000
    j = np.arange(N)
    return crafted("two_bins", N, 33, np.where(j % 2 == 0, 2.25, 2.75), np.full(N, 3.25), np.full(N, 0.05), np.full(N, 1.0 / N))


def draw_values(seed, update, count):
    """u_i of the first `count` draws when K = 2^40."""
    return [mo.key_int(seed, update, i, ko.DRAW) % TWO40 for i in range(count)]


def far_bin(name, seed, at_draw):
    """Two bins and one particle of count 1 in a far bin.  The weights are integer counts over 2^40 whose sum is 2^40, so W = 1,
    the counts are those integers and K = 2^40: draw i lands on u_i = key(seed, 1, i, 3) mod 2^40.  Particle 0 (bin A) takes the
    counts 0 .. u - 1 and particle 1, the far one, the count u = u_at_draw alone: draw `at_draw` is its one draw."""
    N = 3000
    u = draw_values(seed, 1, N)
    assert u.count(u[at_draw]) == 1 and 0 < u[at_draw] < TWO40 - N
    counts = np.zeros(N, dtype=np.int64)
    counts[0], counts[1] = u[at_draw], 1
    rest = TWO40 - u[at_draw] - 1
    counts[2:] = rest // (N - 2)
    counts[2] += rest - int(counts[2:].sum())
    assert int(counts.sum()) == TWO40
    j = np.arange(N)
    x = np.where(j % 2 == 0, 2.25, 2.75)
    y = np.full(N, 3.25)
    x[1], y[1] = 40.25, -17.75
    return crafted(name, N, seed, x, y, np.full(N, 0.05), counts.astype(np.float64) / float(TWO40))


def late_bin():
    return far_bin("late_bin", 34, 500)


def late_bin_before():
    return far_bin("late_bin_before", 34, 50)


PI = mo.PI
EDGE_POSES = [
    (-0.25, -0.25, -0.05), (0.25, 0.25, 0.05), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0),       # around zero, and both zeros
    (0.5, -0.5, math.pi / 18), (-1.5, 1.5, -math.pi / 18), (1.0, 2.0, 2 * (math.pi / 18)),   # exactly on m * size
    (math.nextafter(0.5, 0.0), math.nextafter(-0.5, -1.0), math.nextafter(math.pi / 18, 0.0)),
    (2.0, 2.0, PI), (2.0, 2.0, math.nextafter(-PI, 0.0)),                                    # the ends of (-pi, pi]
    (1e9, 0.0, 0.0), (-1e9, 0.0, 0.0), (0.0, 1e9, 0.0), (0.0, -1e9, 0.0),                    # the clamp, on both sides
    (8388608.0, 0.0, 0.0), (8388607.75, 0.0, 0.0), (-8388608.0, 0.0, 0.0), (-8388608.25, 0.0, 0.0),    # 2^24 bins and the last below
]
EDGE_BINS = [
    (-1, -1, -1), (0, 0, 0), (0, 0, 0), (0, 0, 0),
    (1, -1, 1), (-3, 3, -1), (2, 4, 2),
    (0, -2, 0),
    (4, 4, 18), (4, 4, -18),
    (1 << 24, 0, 0), (-(1 << 24), 0, 0), (0, 1 << 24, 0), (0, -(1 << 24), 0),
    (1 << 24, 0, 0), ((1 << 24) - 1, 0, 0), (-(1 << 24), 0, 0), (-(1 << 24), 0, 0),
]


def exact_edges():
    """Every pose of EDGE_POSES three times, equal weights, N = 54 with min_particles = 54: the limit is N, so all N are drawn
    and almost every particle is an ancestor."""
    P = EDGE_POSES * 3
    N = len(P)
    x, y, yaw = (np.array([p[k] for p in P]) for k in range(3))
    return crafted("exact_edges", N, 35, x, y, yaw, np.full(N, 1.0 / N), min_particles=N)


def far_apart():
    """x = mean + 1e12 g: the particles lie around +-1e12, where floor(x / 0.5) is far beyond the clamp on both sides."""
    steps = [("init", (0.0, 3.0, 0.1), (1e12, 0.0, 0.0)), ("update", STILL, NO_POINTS, dict(OPEN))]
    return case("far_apart", 200, 36, steps, min_particles=10)


ZERO_COUNT = (3, 17, 40, 41, 199)


def zero_counts():
    """Five particles of weight below 2^-40 (2^-41, 2^-60, 0), each in a bin of its own; the others share two bins."""
    N = 200
    j = np.arange(N)
    x, y, w = np.where(j % 2 == 0, 2.25, 2.75), np.full(N, 3.25), np.full(N, 1.0 / (N - len(ZERO_COUNT)))
    for m, jj in enumerate(ZERO_COUNT):
        x[jj], y[jj], w[jj] = 10.25 + m, 10.25, (2.0 ** -41, 2.0 ** -60, 0.0, 2.0 ** -41, 0.0)[m]
    return crafted("zero_counts", N, 37, x, y, np.full(N, 0.05), w, min_particles=150)


@functools.lru_cache(maxsize=None)
def crafted_cases():
    return [one_bin(), own_bins(), two_bins(), late_bin(), late_bin_before(), exact_edges(), far_apart(), zero_counts()]


def bins_of(state, kld):
    """The bin triples of a state's particles, by the checker's function."""
    return [(ko.bin_index(float(a), kld["bin_xy"]), ko.bin_index(float(b), kld["bin_xy"]), ko.bin_index(float(c), kld["bin_yaw"]))
            for a, b, c in zip(state["x"], state["y"], state["yaw"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The checker's trace of a case, computed once and shared."""
    c = {c["name"]: c for c in size_cases() + [fullest_case()] + crafted_cases()}[name]
    return play(c, Checker(c))


def check_crafted(name):
    """On the checker's output alone: the case does what its name says."""
    c = {c["name"]: c for c in crafted_cases()}[name]
    (r, k, st), = reference(name)
    N, anc = c["N"], st["ancestors"]
    up = c["steps"][1]
    assert r["resampled"] == 1 and k["n_before"] == N and len(anc) == k["n_after"]
    if name == "one_bin":
        assert (k["n_after"], k["bins"], k["limit"]) == (N, 1, N)
    elif name == "own_bins":
        assert k["n_after"] == N and k["bins"] == len(set(anc.tolist())) > 100 and k["limit"] == N
    elif name == "two_bins":
        assert (k["n_after"], k["bins"], k["limit"]) == (101, 2, 100)
    elif name == "late_bin":
        assert (k["n_after"], k["bins"], k["limit"]) == (101, 2, 100) and 1 not in anc.tolist()
    elif name == "late_bin_before":
        assert (k["n_after"], k["bins"], k["limit"]) == (183, 3, 182) and anc.tolist().index(1) == 50 and anc.tolist().count(1) == 1
    elif name == "exact_edges":
        x, y, yaw = up[1:4]
        got = bins_of(dict(x=x, y=y, yaw=yaw), c["kld"])
        assert got == EDGE_BINS * 3, got
        assert k["n_after"] == N and k["bins"] == len({got[a] for a in anc.tolist()}) >= 10
        drawn = {got[a] for a in anc.tolist()}
        assert (1 << 24, 0, 0) in drawn and (-(1 << 24), 0, 0) in drawn and (4, 4, 18) in drawn and (4, 4, -18) in drawn
    elif name == "far_apart":
        b = bins_of(st, c["kld"])
        assert {v[0] for v in b} == {1 << 24, -(1 << 24)} and k["bins"] == 2 and np.abs(st["x"]).min() > 1e9 and np.abs(st["x"]).max() > 1e12
    elif name == "zero_counts":
        assert not set(anc.tolist()) & set(ZERO_COUNT) and (k["n_after"], k["bins"], k["limit"]) == (151, 2, 150)


# ---------------------------------------------------------------- the localisation scene with KLD
LOCALISE_N = 3000
LOCALISE_SEEDS = (1, 2, 3, 4, 5)


def localise_case(seed):
    s = mc.localisation_scene()
    start = tuple(a + b for a, b in zip(s["poses"][0], s["offset"]))
    steps = [("init", start, s["sigma"])] + [("update", d, pts, {}) for d, pts in zip(s["odometry"], s["scans"])]
    return case(f"localise_seed{seed}", LOCALISE_N, seed, steps)


@functools.lru_cache(maxsize=None)
def localise_reference(seed):
    c = localise_case(seed)
    return play(c, Checker(c))
