"""The global occupancy map on the GPU (include/visfs_map.h on a visfs_ba handle: k_map_tile, k_map_compose) against the one-core
host twin, byte for byte in cells, counts and info, on the cases and modes of tests/global_map_cases.py;
tests/test_global_map.py holds the twin to the NumPy checker on the same cases."""
import numpy as np
import pytest

import global_map_cases as gc
import scan_match_cases as smc
from visfs_amd import abi, backend
from visfs_amd import global_map as gm
from visfs_amd import scan_fast as sf
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu

CASES = gc.cases()
MODES = [(gm.ODDS, "odds"), (gm.LATEST, "latest"), (gm.OCCUPIED, "occupied")]


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def fill(m, tiles):
    for k, t in enumerate(tiles):
        assert m.add_grid(t["cells"], t["limits"], t["pose"]) == (abi.OK, k), m.last_error()


def composed(m, mode, resolution=0.05, limits=None):
    rc, info = m.compose(mode, resolution, limits)
    assert rc == abi.OK, m.last_error()
    rc, cells, count = m.download()
    assert rc == abi.OK, m.last_error()
    return info, cells, count


def assert_equal_maps(dev, host, mode, resolution=0.05, limits=None):
    a, b = composed(dev, mode, resolution, limits), composed(host, mode, resolution, limits)
    assert a[0] == b[0]
    same(a[1], b[1], "cells"); same(a[2], b[2], "counts")
    assert dev.last_counts() == (1, 1, 1) and host.last_counts() == (0, 0, 0)
    return a


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_twin(solver, case):
    dev, host = gm.GlobalMap(solver), gm.GlobalMap()
    fill(dev, case["tiles"]); fill(host, case["tiles"])
    for mode, _ in MODES:
        assert_equal_maps(dev, host, mode, case["resolution"], case["limits"])
    dev.close(); host.close()


def test_buffers_are_reused_across_sizes_and_poses(solver):
    """One map object through a small, a large and again a small grid, and through set_poses: nothing stale survives."""
    rng = np.random.default_rng(21)
    tiles = [gc.tile(rng, 70, 9), gc.tile(rng, 9, 9, pose=(0.2, 0.1, 0.4))]
    dev, host = gm.GlobalMap(solver), gm.GlobalMap()
    fill(dev, tiles); fill(host, tiles)
    sizes = []
    for poses in ([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0)], [(0.0, 0.0, 0.0), (3.0, 2.5, 0.9)], [(0.1, 0.0, 0.2), (0.0, 0.1, 0.0)]):
        assert dev.set_poses(0, poses) == abi.OK and host.set_poses(0, poses) == abi.OK
        assert dev.last_counts() in ((0, 0, 0), (1, 1, 1))                 # set_poses issues nothing: the counts are the last compose's
        for mode, _ in MODES:
            a = assert_equal_maps(dev, host, mode)
        sizes.append(a[1].size)
    assert sizes[0] < sizes[1] > sizes[2]
    dev.close(); host.close()


@pytest.mark.parametrize("name", ["after_growth", "cropped_front"])
def test_add_submap_on_the_device_equals_add_grid_of_the_download(solver, name):
    case = next(c for c in smc.edge_cases() if c["name"] == name)
    sub = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]), solver=solver)
    hsub = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
    smc.fill(sub, case); smc.fill(hsub, case)
    a, b, twin = gm.GlobalMap(solver), gm.GlobalMap(solver), gm.GlobalMap()
    assert a.add_submap(hsub, 0)[0] == abi.ERR_BAD_ARGUMENT                 # the sub-maps must be of the map's flavour
    assert twin.add_submap(sub, 0)[0] == abi.ERR_BAD_ARGUMENT
    d = sub.describe()
    assert d == hsub.describe() and (name != "cropped_front" or (len(d) == 2 and d[0]["finished"] == 1))
    for i in range(len(d)):
        pose = (0.1 * i, -0.05, 0.2 * i)
        assert a.add_submap(sub, i, pose) == (abi.OK, i), a.last_error()
        assert b.add_grid(sub.download(i)[0], d[i], pose) == (abi.OK, i)
        assert twin.add_submap(hsub, i, pose) == (abi.OK, i)
        assert a.describe_tile(i)[1] == b.describe_tile(i)[1]
    smc.fill(sub, case)                                                    # later insertions do not change a tile
    for mode, _ in MODES:
        x, y = composed(a, mode), composed(b, mode)
        assert x[0] == y[0] and x[1].any()
        same(x[1], y[1]); same(x[2], y[2])
        z = composed(twin, mode)
        assert z[0] == x[0]
        same(x[1], z[1]); same(x[2], z[2])
    sub.close(); hsub.close()
    x, y = composed(a, gm.ODDS), composed(b, gm.ODDS)                      # nor does the sub-maps' destruction
    same(x[1], y[1]); same(x[2], y[2])
    a.close(); b.close(); twin.close()


def test_a_compose_after_a_refusal(solver):
    rng = np.random.default_rng(22)
    t = gc.tile(rng, 66, 7, pose=(0.1, 0.0, 0.3))
    dev, host = gm.GlobalMap(solver), gm.GlobalMap()
    assert dev.download()[0] == abi.ERR_BAD_ARGUMENT and dev.freeze(3).status == abi.ERR_BAD_ARGUMENT
    assert dev.compose(gm.ODDS)[0] == abi.ERR_BAD_ARGUMENT and dev.last_counts() == (0, 0, 0)
    fill(dev, [t]); fill(host, [t])
    _, cells, count = assert_equal_maps(dev, host, gm.ODDS)
    big = dict(t["limits"], num_x_cells=8193, num_y_cells=8192)
    for call, want in ((lambda: dev.compose(7)[0], abi.ERR_BAD_ARGUMENT), (lambda: dev.compose(gm.ODDS, 0.0)[0], abi.ERR_BAD_ARGUMENT),
                       (lambda: dev.compose(gm.ODDS, limits=big)[0], abi.ERR_UNSUPPORTED),
                       (lambda: dev.add_grid(t["cells"], t["limits"], (float("nan"), 0.0, 0.0))[0], abi.ERR_BAD_ARGUMENT),
                       (lambda: dev.set_poses(1, [(0.0, 0.0, 0.0)]), abi.ERR_BAD_ARGUMENT)):
        assert call() == want
        assert dev.last_counts() == (1, 1, 1)                              # the last compose's
        rc, c2, n2 = dev.download()
        assert rc == abi.OK
        same(c2, cells); same(n2, count)
    assert_equal_maps(dev, host, gm.OCCUPIED)
    assert dev.clear() == abi.OK and host.clear() == abi.OK
    rc, c2, _ = dev.download()
    assert rc == abi.OK and c2.shape == cells.shape
    fill(dev, [t, t]); fill(host, [t, t])
    assert_equal_maps(dev, host, gm.ODDS)
    dev.close(); host.close()


def test_stack_from_map_on_the_device(solver):
    case = next(c for c in CASES if c["name"] == "two_overlapping")
    dev, host = gm.GlobalMap(solver), gm.GlobalMap()
    fill(dev, case["tiles"]); fill(host, case["tiles"])
    info, cells, _ = assert_equal_maps(dev, host, gm.ODDS)
    a, b = dev.freeze(4), host.freeze(4)
    g = sf.ScanStack.from_grid(cells, info, 4, solver=solver)
    assert (a.status, b.status, g.status) == (abi.OK, abi.OK, abi.OK), dev.last_error()
    dev.close(); host.close()                                              # the stacks outlive the maps
    assert a.describe()["device"] == 1 and b.describe()["device"] == 0 and a.describe() == g.describe()
    for h in range(4):
        la, lb, lg = a.download_level(h), b.download_level(h), g.download_level(h)
        assert la[1] == lb[1] == lg[1]
        same(la[0], lb[0], h); same(la[0], lg[0], h)
    assert a.download_level(0)[0].any()
    pts = gc.scan_of(np.random.default_rng(15))
    prm = sf.default_params(linear_search_window=0.15, angular_search_window=0.2)
    ra, rb = a.match((0.02, -0.01, 0.1), pts, prm), b.match((0.02, -0.01, 0.1), pts, prm)
    assert ra[0] == abi.OK and ra == rb
    a.close(); b.close(); g.close()
