"""The cases of the laser pretreatment with its voxel filters (include/visfs_scan_filter.h), shared by tests/test_scan_filter.py
(the twin against tests/scan_filter_oracle.py) and tests/test_gpu_scan_filter.py (the device against the twin).

A case: dict(name, scans [(points[n][3], T[12], origin[3])], params {keyword: value} over visfs_scan_filter_default_params) and,
for the adaptive cases, `branch`: what branch_of() must read from the trace ((kind,) or ("halving", j, a move the bisection must
make)).  known_answers(): voxel filters whose result is known without any code."""
import numpy as np

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
ZERO = (0.0, 0.0, 0.0)
# every point a return, whatever its range: the filter alone
ALL_RETURNS = dict(min_range=0.0, max_range=1e9)
M64 = (1 << 64) - 1


def bare(points):
    return (np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3), IDENTITY, ZERO)


def pose(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    return tuple(np.concatenate([R, np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1).reshape(12))


def lattice(ell, nx, ny=1, nz=1, start=(0, 0, 0)):
    """Every point k * ell of an nx x ny x nz block of integer triples k, from `start`."""
    k = np.stack(np.meshgrid(np.arange(nx) + start[0], np.arange(ny) + start[1], np.arange(nz) + start[2], indexing="ij"), axis=-1).reshape(-1, 3)
    return k.astype(np.float64) * ell


# ---------------------------------------------------------------- known answers

def known_answers():
    """[(name, points, length, indices kept)] with ell = 0.25, a power of two: k * ell / ell == k exactly."""
    ell = 0.25
    out = []
    lat = lattice(ell, 5, 4, 3, start=(-2, -1, 0))
    out.append(("lattice_all_kept", lat, ell, list(range(len(lat)))))
    k = 3
    inter = np.concatenate([lat] * k, axis=0)                               # copy c of point i at c * len + i: interleaved copies
    out.append(("copies_first_of_each", inter, ell, list(range(len(lat)))))
    rev = np.concatenate([lat[::-1], lat], axis=0)
    out.append(("copies_reversed_first", rev, ell, list(range(len(lat)))))
    # ties: 0.5 and 1.5 voxels either side fall away from zero, so 0.125 joins 0.25 (voxel 1), not 0 (half-to-even would say 0),
    # and 0.375 joins 0.5 (voxel 2); the same mirrored
    xs = [0.0, 0.125, 0.25, -0.125, -0.25, 0.375, 0.5, -0.375, -0.5]
    ties = np.array([[x, 0.0, 0.0] for x in xs])
    out.append(("ties_away_from_zero_x", ties, ell, [0, 1, 3, 5, 7]))
    out.append(("ties_away_from_zero_z", ties[:, ::-1].copy(), ell, [0, 1, 3, 5, 7]))
    neg = np.array([[-0.26, -0.26, -0.26], [-0.24, -0.24, -0.24], [-0.13, -0.2, -0.3], [0.24, 0.26, 0.3], [-0.24, 0.26, 0.3], [-0.3, -0.3, -0.3]])
    out.append(("negative_coordinates", neg, ell, [0, 3, 4]))             # all of -1,-1,-1 but [3] (1,1,1) and [4] (-1,1,1)
    return out


# ---------------------------------------------------------------- the table's hash, restated to construct the collision case

def table_slots(count):
    s = 16
    while s < 2 * count:
        s <<= 1
    return s


def hash_slot(voxel, list_id, slots):
    key = sum((int(voxel[c]) + (1 << 20)) << (21 * c) for c in range(3))
    k = (key + list_id * 0x9E3779B97F4A7C15) & M64
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    return k & (slots - 1)


def colliding_voxels(count, want, slot=5):
    """`want` voxels (vx, vy, 0) that all start probing at `slot` of the table a pass over `count` points uses."""
    slots, out, v = table_slots(count), [], 0
    while len(out) < want:
        vox = (v % 2001 - 1000, v // 2001 - 1000, 0)
        if hash_slot(vox, 0, slots) == slot:
            out.append(vox)
        v += 1
    return out


# ---------------------------------------------------------------- clouds

def room_scan(rng, n, far=0.0, near=0.0, noise=0.01):
    """n returns off the walls of a 16 x 10 m room seen from inside, in scan order; fractions beyond max_range and below min_range."""
    a = np.sort(rng.uniform(-np.pi, np.pi, n))
    c, s = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore"):
        r = np.minimum(np.where(c > 0, 9.0 / c, -7.0 / c), np.where(s > 0, 6.0 / s, -4.0 / s))
    r = r + rng.normal(0.0, noise, n)
    u = rng.uniform(0.0, 1.0, n)
    r = np.where(u < far, rng.uniform(40.0, 90.0, n), r)
    r = np.where(u > 1.0 - near, rng.uniform(0.0, 0.09, n), r)
    return np.stack([r * c, r * s, rng.normal(0.0, 0.02, n)], axis=1)


def line(n, d):
    """x_i = i * d on the x axis: filtered at length l it has about (n - 1) d / l + 1 voxels."""
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n) * d
    return p


def adaptive_cases():
    """max_length L = 0.5, 257 points at spacing L / 256: the filter at L / 2^j keeps exactly 2^j + 1 of them."""
    L = 0.5
    base = dict(ALL_RETURNS, voxel_size=0.0, adaptive_max_length=L)
    pts = line(257, L / 256)
    out = [dict(name="adaptive_at_most_min_unchanged", scans=[bare(pts)], params=dict(base, adaptive_min_num_points=257), branch=("unchanged",)),
           dict(name="adaptive_enough_at_max_length", scans=[bare(lattice(1.0, 20, 15))], params=dict(base, adaptive_min_num_points=200),
                branch=("at_max",))]
    # M = 2^j + 1: enough first at halving j, and not at the first midpoint, 1.5 low, which keeps round(2^j / 1.5) + 1: high moves
    for j in range(1, 8):
        out.append(dict(name=f"adaptive_halving_{j}", scans=[bare(pts)], params=dict(base, adaptive_min_num_points=2 ** j + 1),
                        branch=("halving", j, "high")))
    # M = 2^4 + 2: halving 5 has 33 >= 18; the midpoint 1.5 low has about 2/3 of them: low moves first
    out.append(dict(name="adaptive_bisection_moves_low", scans=[bare(pts)], params=dict(base, adaptive_min_num_points=18), branch=("halving", 5, "low")))
    dup = np.concatenate([np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0]])] * 100, axis=0)
    out.append(dict(name="adaptive_never_enough", scans=[bare(dup)], params=dict(base, adaptive_min_num_points=200), branch=("never",)))
    # 150 points inside 50 m and 150 beyond (their range from the origin at x = 30 is below max_range: they are returns): the cut
    # comes first, and 150 <= 200 come back unchanged
    inside, beyond = lattice(1.0, 15, 10, start=(-7, -5, 0)), lattice(1.0, 15, 10, start=(51, -5, 0))
    mix = np.empty((300, 3))
    mix[0::2], mix[1::2] = inside, beyond
    out.append(dict(name="adaptive_range_cut_first", scans=[(mix, IDENTITY, (30.0, 0.0, 0.0))],
                    params=dict(min_range=0.0, max_range=40.0, voxel_size=0.0, adaptive_max_length=L, adaptive_min_num_points=200), branch=("unchanged",)))
    return out


def branch_of(record, trace, params):
    """The branch of the adaptive search a result took, read from its trace alone."""
    L, M = params["adaptive_max_length"], params["adaptive_min_num_points"]
    if not trace:
        return ("unchanged",) if record["match_length"] == 0.0 and record["n_match"] == record["n_in_range"] <= M else ("?",)
    assert trace[0][0] == L
    if trace[0][1] >= M:
        return ("at_max",) if len(trace) == 1 and record["match_length"] == L else ("?",)
    for j in range(1, min(8, len(trace))):
        assert trace[j][0] == L / 2 ** j
        if trace[j][1] >= M:
            moves = tuple("low" if c >= M else "high" for _, c in trace[j + 1:])
            return ("halving", j, moves)
    return ("never",) if len(trace) == 8 and record["match_length"] == L / 128 and record["n_match"] == trace[7][1] else ("?",)


def shape_cases():
    rng = np.random.default_rng(41)
    fil = dict(ALL_RETURNS, voxel_size=0.25)
    out = [dict(name="n_1", scans=[bare([[0.3, -0.2, 0.1]])], params=fil),
           dict(name="n_2_one_voxel", scans=[bare([[0.3, -0.2, 0.1], [0.31, -0.19, 0.09]])], params=fil)]
    for n in (1023, 1024, 1025):                                            # the workgroup edge: a dense cloud, about three points a voxel
        out.append(dict(name=f"n_{n}", scans=[bare(rng.uniform(-1.0, 1.0, (n, 3)) * (2.0, 2.0, 0.25))], params=fil))
    out.append(dict(name="n_16384_one_voxel", scans=[bare(rng.uniform(0.26, 0.36, (16384, 3)))], params=fil))
    out.append(dict(name="n_16384_all_distinct", scans=[bare(lattice(0.25, 128, 128, start=(-64, -64, 0)))], params=fil))
    # 64 voxels that all start probing at slot 5 of the 256 slots a pass over 128 points uses (colliding_voxels() walks the voxels
    # (vx, vy, 0) and keeps those hash_slot() sends there), each twice, the second copies in reverse: a probe chain of 64 on
    # which every later point has to compare keys.  test_scan_filter.py holds hash_slot() to visfs_scan_filter_hook_slot.
    vox = np.array(colliding_voxels(128, 64), dtype=np.float64) * 0.25
    out.append(dict(name="colliding_keys", scans=[bare(np.concatenate([vox, vox[::-1]], axis=0))], params=dict(fil, adaptive_max_length=0.0)))
    return out


def pretreat_cases():
    rng = np.random.default_rng(42)
    T = pose(0.3, -0.05, (0.2, -0.1, 0.4))
    scan = room_scan(rng, 1440, far=0.15, near=0.05)
    off = dict(voxel_size=0.0, adaptive_max_length=0.0)
    out = [dict(name=f"pretreat_only_{S}_subdivisions", scans=[(scan, T, (0.01, 0.02, -0.01))], params=dict(off, num_subdivisions=S), pretreat_only=True)
           for S in (1, 3, 16)]
    out.append(dict(name="more_subdivisions_than_points", scans=[(scan[::300], T, ZERO)], params=dict(num_subdivisions=16)))
    out.append(dict(name="all_below_min_range", scans=[bare(rng.uniform(-0.05, 0.05, (300, 3)))], params=dict(num_subdivisions=2)))
    out.append(dict(name="all_misses", scans=[(room_scan(rng, 700) * 10.0, T, ZERO)], params=dict(num_subdivisions=3)))
    out.append(dict(name="filtered_room_4_subdivisions", scans=[(room_scan(rng, 4000, far=0.1, near=0.02), T, (0.01, 0.0, 0.0))],
                    params=dict(num_subdivisions=4, voxel_size=0.05)))
    return out


def batch_case():
    """64 scans of different n, among them n = 0; scan 20 is taken 30 km out by its transform: its voxels at 0.025 m are beyond 2^20."""
    rng = np.random.default_rng(43)
    ns = [0, 1, 2, 3, 1024, 1025] + [int(v) for v in rng.integers(5, 1500, 58)]
    scans = []
    for b, n in enumerate(ns):
        T = pose(0.1 * b, 0.01 * b, (0.01 * b, -0.02 * b, 0.1))
        pts = room_scan(rng, n, far=0.1, near=0.03) if n else np.zeros((0, 3))
        if b == 20:
            T = pose(0.1 * b, 0.0, (3.0e4, 10.0, 0.0))
        scans.append((pts, T, (0.0, 0.0, 0.05)))
    return dict(name="batch_64", scans=scans, params=dict(num_subdivisions=4), bad=[20])


def cases():
    return shape_cases() + pretreat_cases() + adaptive_cases() + [batch_case()]


def big_batch():
    """The largest call: 64 scans of 16384 points (the device against the twin only)."""
    rng = np.random.default_rng(44)
    return dict(name="batch_64_x_16384", scans=[bare(room_scan(rng, 16384, far=0.05, near=0.01)) for _ in range(64)], params=dict(num_subdivisions=2))
