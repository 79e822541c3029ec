"""The cases of the Monte-Carlo localisation tests (tests/test_mcl.py on the CPU, tests/test_gpu_mcl.py on the device): grids for the
likelihood field, a room with an alcove and its ray walk, and the filter runs.  Nothing here calls the library."""
import functools
import math

import numpy as np

import mcl_oracle as mo

OCC, FREE = 2000, 30000                       # a probable obstacle, a probable free cell
RES = 0.05


def limits(nx, ny, res=RES, max_x=None, max_y=None):
    """The grid's cell (ix, iy) has its centre at X = max_x - (iy + 0.5) res, Y = max_y - (ix + 0.5) res."""
    return dict(resolution=res, max_x=ny * res if max_x is None else max_x, max_y=nx * res if max_y is None else max_y,
                num_x_cells=nx, num_y_cells=ny)


def grid(nx, ny, occupied=(), fill=FREE):
    c = np.full((ny, nx), fill, dtype=np.uint16)
    for x, y in occupied:
        c[y, x] = OCC
    return c


def fcase(name, cells, lim=None, **params):
    ny, nx = cells.shape
    return dict(name=name, cells=cells, limits=lim if lim is not None else limits(nx, ny), params=params)


def sprinkled(rng, nx, ny, share):
    c = np.where(rng.random((ny, nx)) < 0.3, 0, FREE).astype(np.uint16)
    occ = rng.random((ny, nx)) < share
    c[occ] = rng.integers(1, 9000, size=int(occ.sum()))
    return c


@functools.lru_cache(maxsize=None)
def field_cases():
    rng = np.random.default_rng(77)
    v_occ = mo.v_occ_of(0.65)
    pair = grid(12, 5)
    pair[2, 3], pair[2, 8] = v_occ, v_occ + 1
    beside = grid(9, 3, [(4, 1)])
    beside[1, 5] = 0
    marked = sprinkled(rng, 200, 150, 0.004)
    marked |= np.where(rng.random(marked.shape) < 0.5, 32768, 0).astype(np.uint16)      # update markers are ignored
    out = [
        fcase("no_obstacle", grid(20, 15), max_dist=0.5),
        fcase("one_by_one", grid(1, 1, [(0, 0)])),
        fcase("corner", grid(30, 20, [(0, 0)]), max_dist=0.5),
        fcase("middle", grid(31, 21, [(15, 10)]), max_dist=0.5),
        fcase("two_equidistant", grid(21, 9, [(4, 4), (16, 4)]), max_dist=0.5),
        fcase("radius_one", grid(11, 9, [(5, 4), (0, 8)]), max_dist=0.075),
        fcase("radius_beyond_grid", grid(9, 7, [(2, 3)])),
        fcase("square_is_integer", grid(40, 30, [(3, 3)], ), limits(40, 30, res=0.25), max_dist=2.5),
        fcase("square_is_no_integer", grid(40, 30, [(20, 15), (3, 28)]), max_dist=0.33),
        fcase("v_occ_and_the_next", pair, max_dist=0.5),
        fcase("unknown_beside", beside, max_dist=0.2),
        fcase("other_threshold", sprinkled(rng, 40, 33, 0.02), max_dist=0.3, occupied_probability=0.8, z_hit=0.9, z_rand=0.1, sigma_hit=0.1,
              range_max=30.0),
        fcase("random_200x150_r40", marked, limits(200, 150, max_x=3.21, max_y=-1.07)),
    ]
    for nx, ny in ((63, 65), (64, 64), (65, 63), (257, 3), (3, 257)):
        out.append(fcase(f"shape_{nx}x{ny}", sprinkled(rng, nx, ny, 0.01), max_dist=0.3))
    return out


# ---------------------------------------------------------------- the room
ROOM_NX, ROOM_NY = 150, 130


@functools.lru_cache(maxsize=None)
def room():
    """A room of 6.0 m x 5.0 m (X across 5.0, Y across 6.0) with walls two cells thick, an alcove in one wall and a pillar: no
    symmetry is left.  (cells, limits); the outside of the walls is unknown."""
    c = np.zeros((ROOM_NY, ROOM_NX), dtype=np.uint16)
    x0, x1, y0, y1 = 15, 135, 15, 115                    # the inner box in cells
    c[y0 - 2:y1 + 2, x0 - 2:x1 + 2] = OCC
    c[y0:y1, x0:x1] = FREE
    c[y0 - 12:y0, 40:70] = OCC                           # the alcove: walls around ...
    c[y0 - 10:y0, 42:68] = FREE                          # ... a recess of 1.3 m x 0.5 m
    c[70:78, 100:108] = OCC                              # the pillar
    c.setflags(write=False)
    return c, limits(ROOM_NX, ROOM_NY)


@functools.lru_cache(maxsize=None)
def room_field():
    """The checker's field of the room at the default parameters, computed once: (t, q, v_occ, T, R)."""
    cells, lim = room()
    out = mo.field(cells, lim["resolution"])
    for a in out[:2]:
        a.setflags(write=False)
    return out


def cell_of(lim, X, Y):
    ix = math.floor((lim["max_y"] - Y) / lim["resolution"])
    iy = math.floor((lim["max_x"] - X) / lim["resolution"])
    return ix, iy


def cast(pose, n, fov=2.0 * math.pi, max_range=8.0):
    """The test's own ray walk on the room: n beams from `pose`, each stepped by a fifth of a cell until it enters an obstacle.
    Returns the hits in the robot frame, [m][3] with z = 0 (beams that leave the grid or reach max_range are dropped)."""
    cells, lim = room()
    x, y, yaw = pose
    pts = []
    for k in range(n):
        a = -0.5 * fov + fov * (k + 0.5) / n
        ca, sa = math.cos(yaw + a), math.sin(yaw + a)
        r = 0.0
        while r < max_range:
            r += 0.01
            ix, iy = cell_of(lim, x + r * ca, y + r * sa)
            if not (0 <= ix < ROOM_NX and 0 <= iy < ROOM_NY):
                break
            if 1 <= cells[iy, ix] <= 9000:
                pts.append((r * math.cos(a), r * math.sin(a), 0.0))
                break
    return np.array(pts, dtype=np.float64).reshape(-1, 3)


def inside_share(pose, pts):
    """The share of the beam endpoints of `pose` that lie inside the grid."""
    _, lim = room()
    if len(pts) == 0:
        return 0.0
    c, s = math.cos(pose[2]), math.sin(pose[2])
    hit = 0
    for px, py, _ in pts:
        ix, iy = cell_of(lim, pose[0] + c * px - s * py, pose[1] + s * px + c * py)
        hit += 0 <= ix < ROOM_NX and 0 <= iy < ROOM_NY
    return hit / len(pts)


ROOM_CENTRE = (3.2, 3.6, 0.3)                 # X, Y, yaw: inside the room, off its centre


def cloud(rng, n):
    """n points in the robot frame within 3.5 m: about the room's size, so endpoints fall on obstacles, free cells and outside."""
    r, a = 3.5 * np.sqrt(rng.random(n)), 2.0 * math.pi * rng.random(n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.normal(size=n)], axis=1)


def deltas(rng, steps=10):
    """Odometry steps of a slow arc, forwards and once backwards and once standing."""
    d = np.stack([0.08 + 0.04 * rng.random(steps), 0.02 * rng.normal(size=steps), 0.06 * rng.normal(size=steps)], axis=1)
    d[3] = (-0.05, 0.01, 0.02)
    d[6] = (0.0, 0.0, 0.0)
    return d


def run_case(name, N, n, seed, max_beams=0, steps=10):
    rng = np.random.default_rng(seed)
    return dict(name=name, N=N, seed=0xC0FFEE + seed, mean=ROOM_CENTRE, sigma=(0.25, 0.25, 0.15), deltas=deltas(rng, steps),
                clouds=[cloud(rng, n) for _ in range(steps)], params=dict(max_beams=max_beams))


@functools.lru_cache(maxsize=None)
def filter_cases():
    out = [run_case(f"N{N}_n30", N, 30, N) for N in (1, 2, 63, 64, 65, 1023, 1024, 1025)]
    out.append(run_case("N65536_n64", 65536, 64, 5))
    out.append(run_case("N64_n16384", 64, 16384, 6))
    out += [run_case(f"N300_n{n}", 300, n, 10 + n) for n in (1, 63, 65)]
    out.append(run_case("N300_n60_beams20", 300, 60, 7, max_beams=20))
    out.append(run_case("N300_n60_beams25", 300, 60, 8, max_beams=25))
    return out


# ---------------------------------------------------------------- the localisation scene
def arc(steps=20):
    """The true poses of a 20-step arc through the room, steps + 1 of them."""
    poses = [(1.6, 1.6, 0.9)]
    for k in range(steps):
        x, y, yaw = poses[-1]
        poses.append((x + 0.12 * math.cos(yaw), y + 0.12 * math.sin(yaw), yaw + (0.03 if k < 10 else -0.05)))
    return poses


def relative(a, b):
    """b in the frame of a: the odometry delta (dx, dy, dyaw)."""
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, b[2] - a[2]])


@functools.lru_cache(maxsize=None)
def localisation_scene(n_beams=60, noise_seed=3):
    """The arc, the scan of every step cast against the same grid and the odometry with seeded noise.  At least 90 % of the true
    pose's endpoints lie inside the grid at every step, and every scan has most of its beams: checked here."""
    rng = np.random.default_rng(noise_seed)
    poses = arc()
    scans, odo = [], []
    for k in range(1, len(poses)):
        pts = cast(poses[k], n_beams)
        assert len(pts) >= 0.9 * n_beams, (k, len(pts))
        assert inside_share(poses[k], pts) >= 0.9, k
        scans.append(pts)
        odo.append(relative(poses[k - 1], poses[k]) + rng.normal(size=3) * (0.01, 0.005, 0.01))
    return dict(poses=poses, scans=scans, odometry=odo, offset=(0.2, 0.0, 0.1), sigma=(0.3, 0.3, 0.2), N=2000)


def pose_error(mean, truth):
    d = (mean[2] - truth[2] + math.pi) % (2.0 * math.pi) - math.pi
    return math.hypot(mean[0] - truth[0], mean[1] - truth[1]), abs(d)
