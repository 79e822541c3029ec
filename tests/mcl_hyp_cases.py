"""The cases of AMCL's pose hypotheses on the KLD filter (tests/test_mcl_hyp.py on the CPU, tests/test_gpu_mcl_hyp.py on the
device).  A case is one of tests/mcl_kld_cases.py (a filter and its steps) with a `world`: the room of tests/mcl_cases.py or the
plain box below.  play() runs one on anything that has init, upload, update and snapshot(); Checker is the checker of
tests/mcl_hyp_oracle.py behind them.  check_case() asserts, on the checker's output alone, that a case does what its name says.
Nothing here calls the library."""
import functools
import math

import numpy as np

import mcl_cases as mc
import mcl_hyp_oracle as ho
import mcl_kld_cases as kc
import mcl_kld_oracle as ko
import mcl_oracle as mo

BIN_XY, BIN_YAW = ko.KLD_DEFAULTS["bin_xy"], ko.KLD_DEFAULTS["bin_yaw"]
CLOSED = dict(kc.ZERO, resample_interval=1, n_eff_ratio=0.0)     # n_eff < 0 never holds: the gate stays closed


# ---------------------------------------------------------------- the worlds
BOX_NX, BOX_NY = 150, 110


@functools.lru_cache(maxsize=None)
def box():
    """A plain rectangular room of 6.0 m x 4.0 m with walls two cells thick: turned by 180 degrees about its centre it looks the
    same.  (cells, limits); the outside of the walls is unknown."""
    c = np.zeros((BOX_NY, BOX_NX), dtype=np.uint16)
    x0, x1, y0, y1 = 15, 135, 15, 95
    c[y0 - 2:y1 + 2, x0 - 2:x1 + 2] = mc.OCC
    c[y0:y1, x0:x1] = mc.FREE
    c.setflags(write=False)
    return c, mc.limits(BOX_NX, BOX_NY)


BOX_CENTRE = (BOX_NY * mc.RES / 2.0, BOX_NX * mc.RES / 2.0)     # X, Y of the point the box is symmetric about


@functools.lru_cache(maxsize=None)
def box_field():
    cells, lim = box()
    out = mo.field(cells, lim["resolution"])
    for a in out[:2]:
        a.setflags(write=False)
    return out


def world(name):
    """((cells, limits), the checker's field) of a world."""
    return (mc.room(), mc.room_field()) if name == "room" else (box(), box_field())


class Checker:
    def __init__(self, case):
        (_, lim), (t, q, _, T, _) = world(case.get("world", "room"))
        self.f = ho.HypFilter(t, q, T, lim["resolution"], lim["max_x"], lim["max_y"], case["N"], case["seed"], **case["kld"])

    def init(self, mean, sigma):
        self.f.init(mean, sigma)

    def upload(self, x, y, yaw, w):
        self.f.upload(x, y, yaw, w)

    def update(self, delta, pts, params):
        return self.f.update(delta, pts, **params)

    def snapshot(self):
        """(the last KLD result, the state cut to n, the hypotheses, the labels of the last resampling)."""
        return dict(self.f.last), {k: np.array(v) for k, v in self.f.state().items()}, self.f.hyp, self.f.labels.copy()

    def limits(self):
        return self.f.limit


def play(case, flt):
    """[(result, kld result, state, hypotheses, labels)] after every update of the case."""
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


# ---------------------------------------------------------------- pure resamplings: an upload, no motion, no beams, the gate open
def centre(b, size):
    return (b + 0.5) * size


def weights(rng, n):
    """Not all equal."""
    return 1.0 + 0.25 * rng.random(n)


def spread(N):
    """N particles spread over a few metres and all yaws; min_particles = N, so all N are drawn."""
    rng = np.random.default_rng(100 + N)
    return kc.crafted(f"spread_N{N}", N, 50 + N, 1.5 + 3.0 * rng.random(N), 1.5 + 3.0 * rng.random(N), rng.uniform(-3.1, 3.1, N), weights(rng, N),
                      min_particles=N)


SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025)


def in_bins(name, seed, bins, per_bin, share=None, **kld):
    """per_bin particles at random places inside each of the bins (integer triples); `share` weighs the bins."""
    rng = np.random.default_rng(seed)
    b = np.repeat(np.array(bins, dtype=np.float64), per_bin, axis=0)
    N = len(b)
    j = 0.05 + 0.9 * rng.random((N, 3))
    w = weights(rng, N) * (np.repeat(np.asarray(share, dtype=np.float64), per_bin) if share is not None else 1.0)
    kld.setdefault("min_particles", N)
    return kc.crafted(name, N, seed, (b[:, 0] + j[:, 0]) * BIN_XY, (b[:, 1] + j[:, 1]) * BIN_XY, (b[:, 2] + j[:, 2]) * BIN_YAW, w, **kld)


def one_cluster():
    return in_bins("one_cluster", 61, [(5, 5, 0), (6, 5, 0), (5, 6, 1), (6, 6, 0)], 100)


MODE_A, MODE_B = (2.2, 2.3, 0.3), (4.6, 4.2, -1.0)


def two_modes(name="two_modes", second=kc.OPEN):
    """N = 3000: 60 % of the weight about A and 40 % about B, 3 m away; two updates, the second's mean is that of both modes."""
    rng = np.random.default_rng(62)
    N = 3000
    at_a = np.arange(N) % 2 == 0
    m = np.where(at_a[:, None], np.array(MODE_A), np.array(MODE_B))
    p = m + rng.normal(size=(N, 3)) * (0.05, 0.05, 0.03)
    w = weights(rng, N)
    w[at_a] *= 0.6 / w[at_a].sum()
    w[~at_a] *= 0.4 / w[~at_a].sum()
    c = kc.crafted(name, N, 62, p[:, 0], p[:, 1], p[:, 2], w)
    c["steps"].append(("update", kc.STILL, kc.NO_POINTS, dict(second)))
    return c


def closed_gate():
    return two_modes("closed_gate", CLOSED)


def corner_touch():
    return in_bins("corner_touch", 63, [(4, 4, 0), (5, 5, 1)], 100)


def gap():
    return in_bins("gap", 64, [(4, 4, 0), (6, 4, 0)], 100)


def yaw_edge():
    return in_bins("yaw_edge", 65, [(4, 4, 17), (4, 4, -18)], 100)


def snake_bins():
    """512 bins, one wide: out along by = 0, two bins across, back along by = 3."""
    b = [(bx, 0, 2) for bx in range(254)] + [(253, 1, 2), (253, 2, 2)] + [(bx, 3, 2) for bx in range(253, -3, -1)]
    assert len(b) == len(set(b)) == 512
    return b


def snake():
    return in_bins("snake", 66, snake_bins(), 32)


TIE_BINS = [(2, 2, 0), (2, 8, 0), (8, 2, 0), (8, 8, 0), (14, 2, 0), (14, 8, 0)]


def ties():
    """Six clusters and 36 draws: some have the same count."""
    return in_bins("ties", 67, TIE_BINS, 6)


NINE_BINS = [(3 * k, 3 * (k % 2), k - 4) for k in range(9)]
NINE_SHARE = [10, 2, 9, 8, 7, 6, 5, 4, 3]


def nine():
    return in_bins("nine", 68, NINE_BINS, 100, share=NINE_SHARE)


def late_bin():
    return dict(kc.late_bin(), name="late_bin")


def late_bin_before():
    return dict(kc.late_bin_before(), name="late_bin_before")


def clamp():
    """The bins +2^24 (x = 1e9), 2^24 - 1 beside it and -2^24 (x = -1e9): a neighbour's index goes to 2^24 + 1."""
    N = 300
    rng = np.random.default_rng(69)
    x = np.array([1e9, 8388607.75, -1e9] * (N // 3))
    return kc.crafted("clamp", N, 69, x, np.full(N, 0.25), np.full(N, 0.05), weights(rng, N), min_particles=N)


@functools.lru_cache(maxsize=None)
def size_cases():
    return [spread(N) for N in SIZES]


@functools.lru_cache(maxsize=None)
def fullest_case():
    """N = 16384 with thousands of bins, the case of tests/mcl_kld_cases.py."""
    return dict(kc.fullest_case(), name="fullest")


@functools.lru_cache(maxsize=None)
def crafted_cases():
    return [one_cluster(), two_modes(), closed_gate(), corner_touch(), gap(), yaw_edge(), snake(), ties(), nine(), late_bin(), late_bin_before(),
            clamp()]


# ---------------------------------------------------------------- the localisation scenes
LOCALISE_N = kc.LOCALISE_N
LOCALISE_SEEDS = kc.LOCALISE_SEEDS


def room_case(seed):
    return dict(kc.localise_case(seed), name=f"room_seed{seed}")


def turned(pose):
    """The pose's image under the box's symmetry: turned by 180 degrees about the centre."""
    return (2.0 * BOX_CENTRE[0] - pose[0], 2.0 * BOX_CENTRE[1] - pose[1], float(mo.wrap(pose[2] + math.pi)))


def box_cast(pose, n):
    """mcl_cases.cast on the box."""
    cells, lim = box()
    x, y, yaw = pose
    pts = []
    for k in range(n):
        a = -math.pi + 2.0 * math.pi * (k + 0.5) / n
        ca, sa = math.cos(yaw + a), math.sin(yaw + a)
        r = 0.0
        while r < 8.0:
            r += 0.01
            ix, iy = mc.cell_of(lim, x + r * ca, y + r * sa)
            if not (0 <= ix < BOX_NX and 0 <= iy < BOX_NY):
                break
            if 1 <= cells[iy, ix] <= 9000:
                pts.append((r * math.cos(a), r * math.sin(a), 0.0))
                break
    return np.array(pts, dtype=np.float64).reshape(-1, 3)


MIRROR_SEEDS = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def mirror_scene(n_beams=60, noise_seed=4):
    """A 20-step arc through the box, its scans and its odometry with seeded noise."""
    rng = np.random.default_rng(noise_seed)
    poses = [(1.3, 1.6, 0.3)]                                               # stays more than a metre from the centre, where the modes would meet
    for k in range(20):
        x, y, yaw = poses[-1]
        poses.append((x + 0.12 * math.cos(yaw), y + 0.12 * math.sin(yaw), yaw + (0.03 if k < 10 else -0.05)))
    scans = [box_cast(p, n_beams) for p in poses[1:]]
    assert all(len(s) >= 0.9 * n_beams for s in scans)
    odo = [mc.relative(a, b) + rng.normal(size=3) * (0.01, 0.005, 0.01) for a, b in zip(poses[:-1], poses[1:])]
    return dict(poses=poses, scans=scans, odometry=odo)


def mirror_case(seed):
    """The belief starts half on the true pose and half on its image; the reference's settings from there on."""
    s = mirror_scene()
    rng = np.random.default_rng(1000 + seed)
    N = LOCALISE_N
    start, image = s["poses"][0], turned(s["poses"][0])
    m = np.where((np.arange(N) % 2 == 0)[:, None], np.array(start), np.array(image))
    p = m + rng.normal(size=(N, 3)) * (0.2, 0.2, 0.1)
    steps = [("init", start, (0.0, 0.0, 0.0)), ("upload", p[:, 0], p[:, 1], mo.wrap(p[:, 2]), np.full(N, 1.0 / N))]
    steps += [("update", d, pts, {}) for d, pts in zip(s["odometry"], s["scans"])]
    return dict(kc.case(f"mirror_seed{seed}", N, seed, steps), world="box")


# ---------------------------------------------------------------- the checker's traces, computed once and shared
def all_cases():
    out = size_cases() + [fullest_case()] + crafted_cases()
    out += [room_case(s) for s in LOCALISE_SEEDS] + [mirror_case(s) for s in MIRROR_SEEDS]
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def reference(name):
    c = all_cases()[name]
    return play(c, Checker(c))


def hyps(h):
    return h["hyp"][:h["n_hypotheses"]]


def near(mean, pose, xy=BIN_XY, yaw=BIN_YAW):
    return abs(mean[0] - pose[0]) <= xy and abs(mean[1] - pose[1]) <= xy and mc.pose_error(mean, pose)[1] <= yaw


def check_case(name):
    """On the checker's output alone: the case does what its name says."""
    c = all_cases()[name]
    ref = reference(name)
    at = 1 if name == "fullest" else 0                                      # the update that resamples first
    r, k, st, h, lab = ref[at]
    N = c["N"]
    assert r["resampled"] == 1 and h["fresh"] == 1 and h["n"] == k["n_after"] == len(lab) == len(st["x"]) and h["update"] == at + 1
    H = hyps(h)
    counts = [e["count"] for e in H]
    assert h["n_hypotheses"] == min(h["n_clusters"], ho.HYP_MAX) and len(set(lab.tolist())) == h["n_clusters"]
    assert counts == sorted(counts, reverse=True) and all(e["count"] == int((lab == e["label"]).sum()) for e in H)
    assert all(e == ho.empty_hypothesis() for e in h["hyp"][h["n_hypotheses"]:])
    if h["n_clusters"] <= ho.HYP_MAX:
        assert sum(counts) == h["n"] and abs(sum(e["weight"] for e in H) - 1.0) < 1e-12
    if name.startswith("spread_N"):
        assert k["n_after"] == N and (N < 1000 or h["n_clusters"] >= 2 or H[0]["bins"] > 100)
    elif name == "one_cluster":
        assert h["n_clusters"] == 1 and H[0]["count"] == N == h["n"] and H[0]["bins"] == 4 and H[0]["label"] == 0
        ms, mc_ = np.sin(st["yaw"]).mean(), np.cos(st["yaw"]).mean()
        assert abs(H[0]["mean"][0] - st["x"].mean()) < 1e-12 and abs(H[0]["mean"][1] - st["y"].mean()) < 1e-12
        assert abs(H[0]["mean"][2] - math.atan2(ms, mc_)) < 1e-12
    elif name in ("two_modes", "closed_gate"):
        assert h["n_clusters"] == 2 and near(H[0]["mean"], MODE_A) and near(H[1]["mean"], MODE_B) and H[0]["count"] > H[1]["count"]
        assert abs(H[0]["weight"] + H[1]["weight"] - 1.0) < 1e-12 and 0.5 < H[0]["weight"] < 0.7
        r2, k2, _, h2, lab2 = ref[1]
        d = math.hypot(MODE_A[0] - MODE_B[0], MODE_A[1] - MODE_B[1])
        assert d >= 2.0 and all(math.hypot(r2["mean"][0] - m[0], r2["mean"][1] - m[1]) > 0.3 * d for m in (MODE_A, MODE_B))
        if name == "closed_gate":                                           # the block is kept, fresh is cleared
            assert r2["resampled"] == 0 and h2 == dict(h, fresh=0) and (lab2 == lab).all()
        else:
            assert r2["resampled"] == 1 and h2["fresh"] == 1 and h2["update"] == 2 and h2["n_clusters"] == 2
    elif name == "corner_touch":
        assert h["n_clusters"] == 1 and H[0]["bins"] == 2 and H[0]["count"] == N
    elif name == "gap":
        assert h["n_clusters"] == 2 and [e["bins"] for e in H] == [1, 1]
    elif name == "yaw_edge":
        assert h["n_clusters"] == 2 and [e["bins"] for e in H] == [1, 1]
        assert {ko.bin_index(float(v), BIN_YAW) for v in st["yaw"]} == {17, -18}
    elif name == "snake":
        assert h["n_clusters"] == 1 and H[0]["bins"] == 512 and H[0]["count"] == N == 16384 and H[0]["label"] == 0
    elif name == "ties":
        assert h["n_clusters"] == len(TIE_BINS) and len(set(counts)) < len(counts)
        assert all(a["label"] < b["label"] for a, b in zip(H, H[1:]) if a["count"] == b["count"])
    elif name == "nine":
        assert h["n_clusters"] == 9 and h["n_hypotheses"] == 8
        left = set(lab.tolist()) - {e["label"] for e in H}
        assert len(left) == 1 and 0 < int((lab == left.pop()).sum()) < min(counts)         # the smallest is left out
        assert sum(counts) < h["n"]
    elif name == "late_bin":
        assert h["n_clusters"] == 1 and H[0]["bins"] == 2 and 1 not in st["ancestors"].tolist() and k["n_after"] == 101
    elif name == "late_bin_before":
        assert h["n_clusters"] == 2 and [e["count"] for e in H] == [182, 1] and H[1]["label"] == 50
    elif name == "clamp":
        b = {ko.bin_index(float(v), BIN_XY) for v in st["x"]}
        assert b == {1 << 24, (1 << 24) - 1, -(1 << 24)} and h["n_clusters"] == 2 and sorted(e["bins"] for e in H) == [1, 2]
    elif name == "fullest":
        assert ref[0][3] == ho.no_hypotheses() and k["bins"] > 2000 and h["n_clusters"] > 50 and h["n_hypotheses"] == 8


# The final error (metres, radians) of hypothesis 0 on the checker in the room scene with N = 3000 and the reference's settings,
# seeds 1 .. 5, measured on the CPU; the tests hold three times the worst.
ROOM_MEASURED = [(0.0522, 0.0202), (0.0695, 0.0131), (0.0571, 0.0154), (0.0625, 0.0225), (0.0759, 0.0220)]
ROOM_BOUND = (3.0 * max(e[0] for e in ROOM_MEASURED), 3.0 * max(e[1] for e in ROOM_MEASURED))


def room_errors(seed):
    """(metres, radians) of hypothesis 0 after the last resampling against the pose it was computed at."""
    s = mc.localisation_scene()
    ref = reference(f"room_seed{seed}")
    last = max(i for i, t in enumerate(ref) if t[0]["resampled"])
    h = ref[last][3]
    assert h["update"] == last + 1
    return mc.pose_error(h["hyp"][0]["mean"], s["poses"][last + 1])


def check_mirror(seed):
    """Both hypotheses survive the arc; at every resampling one of the two best lies within the room's bound of the truth while the
    mean of the whole set does not."""
    s = mirror_scene()
    ref = reference(f"mirror_seed{seed}")
    ran = [(i, t) for i, t in enumerate(ref) if t[0]["resampled"]]
    assert len(ran) == 10
    for i, (r, k, st, h, lab) in ran:
        truth = s["poses"][i + 1]
        assert h["n_hypotheses"] >= 2, (seed, i)
        errs = [mc.pose_error(e["mean"], truth) for e in h["hyp"][:2]]
        assert any(et <= ROOM_BOUND[0] and er <= ROOM_BOUND[1] for et, er in errs), (seed, i, errs)
        assert mc.pose_error(r["mean"], truth)[0] > ROOM_BOUND[0], (seed, i)
    h = ran[-1][1][3]
    t, m = s["poses"][ran[-1][0] + 1], turned(s["poses"][ran[-1][0] + 1])
    e0, e1 = h["hyp"][0]["mean"], h["hyp"][1]["mean"]
    assert (near(e0, t) and near(e1, m)) or (near(e0, m) and near(e1, t)), (seed, e0, e1)
