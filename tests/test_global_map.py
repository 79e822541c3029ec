"""The global occupancy map (include/visfs_map.h) on the CPU: the one-core host twin against the NumPy checker
of tests/global_map_oracle.py, byte for byte in cells and counts, on the cases of tests/global_map_cases.py; the host plan, the
refusals, the pose helper and the stack frozen from a composed grid.  tests/test_gpu_global_map.py holds the device to the twin."""
import functools
import math

import numpy as np
import pytest

import global_map_cases as gc
import global_map_oracle as go
import scan_match_cases as smc
from visfs_amd import abi
from visfs_amd import global_map as gm
from visfs_amd import scan_fast as sf
from visfs_amd import submap as sm

CASES = gc.cases()
BY_NAME = {c["name"]: c for c in CASES}
MODES = [(gm.ODDS, "odds"), (gm.LATEST, "latest"), (gm.OCCUPIED, "occupied")]
RUNS = [(c["name"], m) for c in CASES for m, _ in MODES]
RUN_IDS = [f"{c['name']}-{n}" for c in CASES for _, n in MODES]


@functools.lru_cache(maxsize=None)
def table():
    return gm.hook_odds_table()


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """The checker's answer, computed once per (case, mode) and shared."""
    c = BY_NAME[name]
    lim, cells, count, drawn = go.compose(c["tiles"], table(), mode, c["resolution"], c["limits"])
    cells.setflags(write=False); count.setflags(write=False)
    return lim, cells, count, drawn


def fill(m, tiles):
    for k, t in enumerate(tiles):
        rc, idx = m.add_grid(t["cells"], t["limits"], t["pose"])
        assert rc == abi.OK and idx == k, m.last_error()


def composed(m, mode, resolution=0.05, limits=None):
    rc, info = m.compose(mode, resolution, limits)
    assert rc == abi.OK, m.last_error()
    rc, cells, count = m.download()
    assert rc == abi.OK, m.last_error()
    return info, cells, count


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def twin_of(tiles):
    m = gm.GlobalMap()
    fill(m, tiles)
    return m


# ---------------------------------------------------------------- known answers: the checker first, then the twin
def identity_tile():
    rng = np.random.default_rng(1)
    t = gc.tile(rng, 7, 5, max_x=0.31, max_y=-0.12)
    t["cells"] = t["cells"] | np.where(rng.random((5, 7)) < 0.5, 32768, 0).astype(np.uint16)
    return t


def quarter_turns(cells, k):
    """A square tile centred on the origin turned by k quarter turns, in exact integers: the centre of cell (jx, jy) in half cells
    is (u, w) = (n - (2 jy + 1), n - (2 jx + 1)) (the y index runs along -x, the x index along -y); a quarter turn takes
    (u, w) to (-w, u)."""
    n = cells.shape[0]
    out = np.zeros_like(cells)
    for jy in range(n):
        for jx in range(n):
            u, w = n - (2 * jy + 1), n - (2 * jx + 1)
            for _ in range(k):
                u, w = -w, u
            out[(n - u - 1) // 2, (n - w - 1) // 2] = cells[jy, jx]
    return out


@pytest.mark.parametrize("mode", [m for m, _ in MODES])
def test_checker_returns_a_tile_under_the_identity(mode):
    t = identity_tile()
    _, cells, count, _ = go.compose([t], table(), mode, limits=t["limits"])
    same(cells, t["cells"] & 32767)
    same(count, ((t["cells"] & 32767) > 0).astype(np.uint8))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_checker_permutes_a_square_tile_under_quarter_turns(k):
    t = gc.tile(np.random.default_rng(2), 6, 6, pose=(0.0, 0.0, k * math.pi / 2))
    for mode, _ in MODES:
        _, cells, _, _ = go.compose([t], table(), mode, limits=t["limits"])
        same(cells, quarter_turns(t["cells"], k))


@pytest.mark.parametrize("mode", [m for m, _ in MODES])
def test_twin_returns_a_tile_under_the_identity(mode):
    t = identity_tile()
    info, cells, count = composed(twin_of([t]), mode, limits=t["limits"])
    same(cells, t["cells"] & 32767)
    same(count, ((t["cells"] & 32767) > 0).astype(np.uint8))
    assert (info["tiles"], info["tiles_drawn"]) == (1, 1)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_twin_permutes_a_square_tile_under_quarter_turns(k):
    t = gc.tile(np.random.default_rng(2), 6, 6, pose=(0.0, 0.0, k * math.pi / 2))
    for mode, _ in MODES:
        _, cells, _ = composed(twin_of([t]), mode, limits=t["limits"])
        same(cells, quarter_turns(t["cells"], k))


# ---------------------------------------------------------------- the log-odds table
def test_odds_table():
    L = table().astype(np.int64)
    cost, _ = sm.hook_value_tables()
    assert np.max(np.abs(L[1:] - go.odds_table_numpy(cost)[1:])) <= 1
    d = L[1:-1] - L[2:]
    assert d.min() >= 102 and d.max() <= 285                               # strictly decreasing
    assert L[0] == 0 and L[16384] == 0
    v = np.arange(1, 32768)
    assert np.array_equal(L[v], -L[32768 - v])
    assert np.abs(L).max() <= 2303957 and 256 * int(np.abs(L).max()) < 2 ** 31
    assert gm.load().visfs_map_abi_version() == gm.ABI_VERSION == 1


# ---------------------------------------------------------------- twin against checker
@pytest.mark.parametrize("name,mode", RUNS, ids=RUN_IDS)
def test_twin_equals_checker(name, mode):
    c = BY_NAME[name]
    lim, cells, count, _ = reference(name, mode)
    m = twin_of(c["tiles"])
    info, got, got_count = composed(m, mode, c["resolution"], c["limits"])
    for k in gm.LIMIT_KEYS:
        assert info[k] == lim[k], k
    same(got, cells, "cells")
    same(got_count, count, "counts")
    assert m.last_counts() == (0, 0, 0)
    m.close()


def test_stack256_meets_its_known_answers():
    tiles = BY_NAME["stack256"]["tiles"]
    lim = tiles[0]["limits"]
    _, cells, count, _ = go.compose(tiles, table(), gm.ODDS, limits=lim)
    _, got, got_count = composed(twin_of(tiles), gm.ODDS, limits=lim)
    for c, n in ((cells, count), (got, got_count)):
        assert np.all(c[0] == 1) and np.all(c[1] == 32767) and np.all(c[2] == 16384)     # the two clamps, and pairs that cancel
        assert np.all(n == 255)                                            # 256 tiles, and 255 in the last cell: both read 255


# ---------------------------------------------------------------- set_poses, clear
def test_set_poses_equals_a_fresh_map_and_leaves_nothing_stale():
    rng = np.random.default_rng(11)
    tiles = [gc.tile(rng, 10, 8), gc.tile(rng, 9, 9, pose=(0.2, 0.1, 0.4)), gc.tile(rng, 5, 12, pose=(-0.1, 0.3, -1.0))]
    m = twin_of(tiles)
    composed(m, gm.ODDS)
    sizes = []
    for poses in ([(0.0, 0.0, 0.0), (2.0, 1.5, 0.9), (-1.0, 0.3, -1.0)], [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)],
                  [(0.3, 0.0, 0.1), (0.2, 0.1, 0.4), (-0.1, 0.3, -1.0)]):
        assert m.set_poses(0, poses[:1]) == abi.OK and m.set_poses(1, poses[1:]) == abi.OK
        for k in range(3):
            rc, lim, pose = m.describe_tile(k)
            assert rc == abi.OK and tuple(pose) == poses[k] and lim == tiles[k]["limits"]
        fresh = twin_of([dict(t, pose=p) for t, p in zip(tiles, poses)])
        for mode, _ in MODES:
            a, b = composed(m, mode), composed(fresh, mode)
            assert a[0] == b[0]
            same(a[1], b[1]); same(a[2], b[2])
        sizes.append(a[1].size)
    assert sizes[0] > sizes[1] < sizes[2]                                   # a larger grid, then a smaller one, then a larger one


def test_clear():
    rng = np.random.default_rng(12)
    a, b = gc.tile(rng, 6, 6), gc.tile(rng, 4, 7, pose=(0.1, 0.0, 0.3))
    m = twin_of([a])
    _, cells, count = composed(m, gm.ODDS)
    assert m.clear() == abi.OK
    assert m.describe_tile(0)[0] == abi.ERR_BAD_ARGUMENT
    assert m.compose(gm.ODDS)[0] == abi.ERR_BAD_ARGUMENT                    # no tile to take limits from
    rc, c2, n2 = m.download()
    assert rc == abi.OK
    same(c2, cells); same(n2, count)                                        # the last grid stays
    info, c3, n3 = composed(m, gm.ODDS, limits=gc.limits(3, 2))             # no tile, explicit limits: an unknown grid
    assert (info["tiles"], info["tiles_drawn"]) == (0, 0) and not c3.any() and not n3.any() and c3.shape == (2, 3)
    fill(m, [b])
    got, want = composed(m, gm.ODDS), composed(twin_of([b]), gm.ODDS)
    assert got[0] == want[0]
    same(got[1], want[1]); same(got[2], want[2])


# ---------------------------------------------------------------- the host plan
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_plan_limits_and_boxes(name):
    c = BY_NAME[name]
    lim, _, _, drawn = reference(name, gm.LATEST)
    rc, plim, boxes, ndrawn = gm.plan([t["limits"] for t in c["tiles"]], [t["pose"] for t in c["tiles"]], gm.LATEST, c["resolution"], c["limits"])
    assert rc == abi.OK
    for k in gm.LIMIT_KEYS:
        assert plim[k] == lim[k], k
    want = [go.box(t, lim) for t in c["tiles"]]
    assert ndrawn == sum(b is not None for b in want)
    known = None
    for k, (b, d) in enumerate(zip(want, drawn)):
        got = tuple(int(v) for v in boxes[k])
        if b is None:
            assert got[0] > got[2] or got[1] > got[3]
            assert not d.any()                                             # an empty box drops nothing
            continue
        assert got == b, k
        ys, xs = np.nonzero(d)
        if len(xs):
            assert b[0] <= xs.min() and xs.max() <= b[2] and b[1] <= ys.min() and ys.max() <= b[3], k
        known = b if known is None else (min(known[0], b[0]), min(known[1], b[1]), max(known[2], b[2]), max(known[3], b[3]))
    kb = (plim["known_min_x"], plim["known_min_y"], plim["known_max_x"], plim["known_max_y"])
    if known is None:
        assert kb[0] > kb[2] or kb[1] > kb[3]
    else:
        assert kb == known
    m = twin_of(c["tiles"])
    rc, info = m.compose(gm.LATEST, c["resolution"], c["limits"])
    assert rc == abi.OK and {k: info[k] for k in plim} == plim and (info["tiles"], info["tiles_drawn"]) == (len(c["tiles"]), ndrawn)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_last_grid():
    rng = np.random.default_rng(13)
    t = gc.tile(rng, 6, 5, pose=(0.1, 0.0, 0.3))
    m = gm.GlobalMap()
    assert m.download()[0] == abi.ERR_BAD_ARGUMENT                          # compose never run
    st = m.freeze(3)
    assert st.status == abi.ERR_BAD_ARGUMENT and st.h is None
    assert m.compose(gm.ODDS)[0] == abi.ERR_BAD_ARGUMENT                    # no tile and no explicit limits
    assert m.last_counts() == (0, 0, 0)
    fill(m, [t])
    _, cells, count = composed(m, gm.ODDS)
    nan, inf = float("nan"), float("inf")
    bad, uns = abi.ERR_BAD_ARGUMENT, abi.ERR_UNSUPPORTED

    def lim(**kw):
        return dict(t["limits"], **kw)

    refused = [
        (lambda: m.add_grid(t["cells"], t["limits"], (nan, 0.0, 0.0))[0], bad),
        (lambda: m.add_grid(t["cells"], t["limits"], (0.0, 0.0, inf))[0], bad),
        (lambda: m.add_grid(t["cells"], lim(max_x=inf), t["pose"])[0], bad),
        (lambda: m.add_grid(t["cells"], lim(resolution=0.0), t["pose"])[0], bad),
        (lambda: m.add_grid(t["cells"], lim(resolution=-0.05), t["pose"])[0], bad),
        (lambda: m.add_grid(t["cells"], lim(resolution=nan), t["pose"])[0], bad),
        (lambda: m.add_grid(t["cells"], lim(num_x_cells=0), t["pose"], check_size=False)[0], bad),
        (lambda: m.add_grid(t["cells"], lim(num_y_cells=-1), t["pose"], check_size=False)[0], bad),
        (lambda: m.add_grid(t["cells"], lim(num_x_cells=32768, num_y_cells=16385), t["pose"], check_size=False)[0], uns),    # above 1 GiB, refused unread
        (lambda: m.set_poses(0, [(0.0, nan, 0.0)]), bad),
        (lambda: m.set_poses(1, [(0.0, 0.0, 0.0)]), bad),
        (lambda: m.set_poses(-1, [(0.0, 0.0, 0.0)]), bad),
        (lambda: m.describe_tile(1)[0], bad),
        (lambda: m.describe_tile(-1)[0], bad),
        (lambda: m.compose(3)[0], bad),
        (lambda: m.compose(-1)[0], bad),
        (lambda: m.compose(gm.ODDS, 0.0)[0], bad),
        (lambda: m.compose(gm.ODDS, nan)[0], bad),
        (lambda: m.compose(gm.ODDS, limits=lim(resolution=0.0))[0], bad),
        (lambda: m.compose(gm.ODDS, limits=lim(max_y=nan))[0], bad),
        (lambda: m.compose(gm.ODDS, limits=lim(num_x_cells=0))[0], bad),
        (lambda: m.compose(gm.ODDS, limits=lim(num_x_cells=8193, num_y_cells=8192))[0], uns),
        (lambda: m.compose(gm.ODDS, 1e-6)[0], uns),                         # the tiles' extents at a micrometre: above 2^26 cells
        (lambda: m.freeze(0).status, bad),
        (lambda: m.freeze(17).status, bad),
    ]
    for i, (call, want) in enumerate(refused):
        assert call() == want, i
        rc, c2, n2 = m.download()
        assert rc == abi.OK, i
        same(c2, cells, i); same(n2, count, i)
    rc, _, pose = m.describe_tile(0)
    assert rc == abi.OK and tuple(pose) == t["pose"]                        # a refused set_poses changed nothing
    _, c3, n3 = composed(m, gm.ODDS)                                        # and a compose after the refusals is the same
    same(c3, cells); same(n3, count)


def test_the_257th_tile_and_the_gibibyte():
    one = dict(cells=np.full((1, 1), 7, dtype=np.uint16), limits=gc.limits(1, 1, max_x=0.05, max_y=0.05), pose=(0.0, 0.0, 0.0))
    m = twin_of([one] * 256)
    _, cells, count = composed(m, gm.LATEST)
    assert m.add_grid(one["cells"], one["limits"], one["pose"])[0] == abi.ERR_UNSUPPORTED
    rc, c2, n2 = m.download()
    assert rc == abi.OK
    same(c2, cells); same(n2, count)
    assert count.max() == 255
    rc, _, _, _ = gm.plan([one["limits"]] * 257, [one["pose"]] * 257)
    assert rc == abi.ERR_UNSUPPORTED


# ---------------------------------------------------------------- the pose of a tile after an optimisation
def test_pose_from_anchor():
    rng = np.random.default_rng(14)
    for _ in range(20):
        a, b = rng.uniform(-3, 3, size=3), rng.uniform(-3, 3, size=3)
        rc, p = gm.pose_from_anchor(a, b)
        want = go.pose_from_anchor(a, b)
        assert rc == abi.OK
        assert np.allclose(p[:2], want[:2], rtol=0, atol=1e-12)
        assert abs(math.remainder(p[2] - want[2], 2 * math.pi)) < 1e-12
        # the tile pose takes the anchor as frozen to the anchor as it is now
        c, s = math.cos(p[2]), math.sin(p[2])
        assert np.allclose([c * a[0] - s * a[1] + p[0], s * a[0] + c * a[1] + p[1]], b[:2], rtol=0, atol=1e-12)
    rc, p = gm.pose_from_anchor((1.0, 2.0, 0.3), (1.0, 2.0, 0.3))
    assert rc == abi.OK and np.allclose(p, 0.0, atol=1e-15)
    assert gm.pose_from_anchor((float("nan"), 0, 0), (0, 0, 0))[0] == abi.ERR_BAD_ARGUMENT


# ---------------------------------------------------------------- sub-maps as tiles (twin flavour)
@pytest.mark.parametrize("name", ["after_growth", "cropped_front"])
def test_add_submap_equals_add_grid_of_the_download(name):
    case = next(c for c in smc.edge_cases() if c["name"] == name)
    sub = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
    smc.fill(sub, case)
    a, b = gm.GlobalMap(), gm.GlobalMap()
    d = sub.describe()
    for i in range(len(d)):
        pose = (0.1 * i, -0.05, 0.2 * i)
        assert a.add_submap(sub, i, pose) == (abi.OK, i), a.last_error()
        assert b.add_grid(sub.download(i)[0], d[i], pose) == (abi.OK, i)
        assert a.describe_tile(i)[1] == b.describe_tile(i)[1]
    assert a.add_submap(sub, len(d))[0] == abi.ERR_BAD_ARGUMENT
    smc.fill(sub, case)                                                    # later insertions do not change the tiles
    sub.close()                                                            # nor does the sub-maps' destruction
    for mode, _ in MODES:
        x, y = composed(a, mode), composed(b, mode)
        assert x[0] == y[0] and x[1].any()
        same(x[1], y[1]); same(x[2], y[2])


# ---------------------------------------------------------------- a stack frozen from the composed grid
def test_stack_from_map_equals_stack_from_the_downloaded_grid():
    c = BY_NAME["two_overlapping"]
    m = twin_of(c["tiles"])
    info, cells, _ = composed(m, gm.ODDS)
    a = m.freeze(4)
    assert a.status == abi.OK, m.last_error()
    m.close()                                                              # the stack outlives the map
    b = sf.ScanStack.from_grid(cells, info, 4)
    assert b.status == abi.OK
    da, db = a.describe(), b.describe()
    assert da == db and da["device"] == 0
    for h in range(4):
        la, lb = a.download_level(h), b.download_level(h)
        assert la[1] == lb[1]
        same(la[0], lb[0], h)
    assert a.download_level(0)[0].any()
    pts = gc.scan_of(np.random.default_rng(15))
    prm = sf.default_params(linear_search_window=0.15, angular_search_window=0.2)
    ra, rb = a.match((0.02, -0.01, 0.1), pts, prm), b.match((0.02, -0.01, 0.1), pts, prm)
    assert ra[0] == abi.OK and ra == rb
