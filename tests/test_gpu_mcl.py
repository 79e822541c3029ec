"""Monte-Carlo localisation on the GPU (include/visfs_mcl.h on a visfs_ba handle: k_mcl_rows, k_mcl_cols, k_mcl_init, k_mcl_weight,
k_mcl_sums, k_mcl_finish, k_mcl_resample) against the one-core host twin, byte for byte in the field, the particles, Q, the
ancestors and every field of the result, on the cases of tests/mcl_cases.py; tests/test_mcl.py holds the twin to the checker."""
import numpy as np
import pytest

import mcl_cases as mc
from visfs_amd import abi, backend
from visfs_amd import global_map as gm
from visfs_amd import mcl
from visfs_amd import scan_filter as sfl

pytestmark = pytest.mark.gpu

FIELD_CASES = mc.field_cases()
FILTER_CASES = mc.filter_cases()
STATE_KEYS = ("x", "y", "yaw", "w", "Q", "ancestors")
ZERO = dict(alpha1=0.0, alpha2=0.0, alpha3=0.0, alpha4=0.0)


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


@pytest.fixture(scope="module")
def rooms(solver):
    cells, lim = mc.room()
    dev, host = mcl.Field.from_grid(cells, lim, solver=solver), mcl.Field.from_grid(cells, lim)
    assert (dev.status, host.status) == (abi.OK, abi.OK)
    yield dev, host
    dev.close(); host.close()


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_state(a, b, what=""):
    for k in STATE_KEYS:
        same(a[k], b[k], (what, k))


def same_result(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k], dtype=np.float64).tobytes() == np.asarray(b[k], dtype=np.float64).tobytes(), (what, k, a[k], b[k])


def same_fields(dev, host):
    assert dict(dev.describe(), device=0) == host.describe() and dev.describe()["device"] == 1
    a, b = dev.download(), host.download()
    same(a[0], b[0], "t"); same(a[1], b[1], "q")
    assert a[2:] == b[2:]
    assert dev.last_counts() == mcl.FIELD_COUNTS == (mcl.FIELD_LAUNCHES, 1, 1) and host.last_counts() == (0, 0, 0)


def pair(rooms, N, seed):
    a, b = mcl.Filter(rooms[0], N, seed), mcl.Filter(rooms[1], N, seed)
    assert (a.status, b.status) == (abi.OK, abi.OK)
    return a, b


def step_both(a, b, delta, pts, what="", **kw):
    (ra, xa), (rb, xb) = a.update(delta, pts, mcl.default_params(**kw)), b.update(delta, pts, mcl.default_params(**kw))
    assert ra == rb == abi.OK, (a.last_error(), b.last_error())
    same_result(xa, xb, what)
    same_state(a.download(), b.download(), what)
    assert a.last_counts() == mcl.UPDATE_COUNTS == (mcl.UPDATE_LAUNCHES, 2, 1) and b.last_counts() == (0, 0, 0)
    return xa


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c["name"] for c in FIELD_CASES])
def test_field_device_equals_twin(solver, case):
    p = mcl.field_params(**case["params"])
    dev, host = mcl.Field.from_grid(case["cells"], case["limits"], p, solver=solver), mcl.Field.from_grid(case["cells"], case["limits"], p)
    assert (dev.status, host.status) == (abi.OK, abi.OK)
    same_fields(dev, host)
    dev.close(); host.close()


def test_field_from_a_device_map_that_is_then_destroyed(solver):
    rng = np.random.default_rng(4)
    a, b = mc.sprinkled(rng, 70, 30, 0.02), mc.sprinkled(rng, 35, 45, 0.02)
    dm, hm = gm.GlobalMap(solver), gm.GlobalMap()
    for m in (dm, hm):
        assert m.add_grid(a, mc.limits(70, 30), (0.0, 0.0, 0.0))[0] == abi.OK and m.add_grid(b, mc.limits(35, 45), (1.1, -0.4, 0.5))[0] == abi.OK
    assert mcl.Field.from_map(dm).status == abi.ERR_BAD_ARGUMENT                # nothing composed yet
    assert dm.compose(gm.ODDS)[0] == abi.OK and hm.compose(gm.ODDS)[0] == abi.OK
    p = mcl.field_params(max_dist=0.6)
    dev, host = mcl.Field.from_map(dm, p), mcl.Field.from_map(hm, p)
    assert (dev.status, host.status) == (abi.OK, abi.OK)
    dm.close(); hm.close()
    same_fields(dev, host)
    assert (dev.download()[0] == 0).any()
    f, g = mcl.Filter(dev, 100, 2), mcl.Filter(host, 100, 2)                    # ... and the field serves a filter afterwards
    assert f.init((1.0, 1.0, 0.2), (0.2, 0.2, 0.1)) == g.init((1.0, 1.0, 0.2), (0.2, 0.2, 0.1)) == abi.OK
    step_both(f, g, (0.1, 0.0, 0.02), mc.cloud(rng, 40))
    f.close(); g.close(); dev.close(); host.close()


def test_field_refusals_on_the_device(solver):
    cells, lim = mc.grid(8, 6, [(1, 1)]), mc.limits(8, 6)
    assert mcl.Field.from_grid(cells, lim, mcl.field_params(max_dist=-1.0), solver=solver).status == abi.ERR_BAD_ARGUMENT
    assert mcl.Field.from_grid(cells, lim, mcl.field_params(max_dist=12.8), solver=solver).status == abi.ERR_UNSUPPORTED
    assert mcl.Field.from_grid(cells, dict(lim, num_y_cells=0), solver=solver).status == abi.ERR_BAD_ARGUMENT


@pytest.mark.parametrize("case", FILTER_CASES, ids=[c["name"] for c in FILTER_CASES])
def test_filter_device_equals_twin(rooms, case):
    a, b = pair(rooms, case["N"], case["seed"])
    assert a.init(case["mean"], case["sigma"]) == b.init(case["mean"], case["sigma"]) == abi.OK
    assert a.last_counts() == mcl.INIT_COUNTS == (mcl.INIT_LAUNCHES, 1, 1)
    same_state(a.download(), b.download(), "init")
    ran = [step_both(a, b, d, pts, k, **case["params"])["resampled"] for k, (d, pts) in enumerate(zip(case["deltas"], case["clouds"]))]
    if case["N"] > 1:
        assert ran == [0, 1] * 5
    a.close(); b.close()


def test_known_answers_on_the_device(rooms):
    """The known answers of tests/test_mcl.py that steer a kernel's branches: no beams, beams outside, a zero step, the wrap, all the
    weight on one particle, and every split of the beams over the lanes."""
    rng = np.random.default_rng(13)
    N = 97
    a, b = pair(rooms, N, 13)
    far = np.array([[100.0, 0.0, 0.0], [0.0, -90.0, 0.0]])
    for f in (a, b):
        assert f.init((3.0, 3.0, 3.0), (0.3, 0.3, 0.3)) == abi.OK
    before = a.download()
    after = step_both(a, b, (0, 0, 0), np.zeros((0, 3)), "zero", **ZERO)
    for k in ("x", "y", "yaw"):
        same(a.download()[k], before[k], k)
    assert after["n_beams"] == 0 and (a.download()["yaw"] < 0).any()
    r = step_both(a, b, (0.1, 0.0, 3.0), far, "far", resample_interval=5, **ZERO)
    assert (a.download()["w"] == a.download()["w"][0]).all() and r["n_beams"] == 2
    x, y, yaw = rng.random(N) + 2.0, rng.random(N) + 2.0, rng.random(N)
    one = np.zeros(N); one[41] = 1.0
    for w in (one, rng.random(N) ** 3):
        assert a.upload(x, y, yaw, w) == b.upload(x, y, yaw, w) == abi.OK
        r = step_both(a, b, (0, 0, 0), np.zeros((0, 3)), "resample", resample_interval=1, n_eff_ratio=2.0, **ZERO)
        assert r["resampled"] == 1
    assert a.upload(x, y, yaw, one) == b.upload(x, y, yaw, one) == abi.OK
    step_both(a, b, (0, 0, 0), np.zeros((0, 3)), "one", resample_interval=1, n_eff_ratio=2.0, **ZERO)
    assert (a.download()["ancestors"] == 41).all()
    pts = mc.cloud(rng, 130)
    for lanes in (1, 2, 4, 8, 16, 32, 64, 0):
        assert a.set_lanes(lanes) == abi.OK
        step_both(a, b, (0.05, 0.01, 0.02), pts, f"lanes {lanes}")
    assert a.download()["Q"].any()
    a.close(); b.close()


def test_the_counts_do_not_depend_on_the_sizes(rooms):
    """N = 1 and N = 65536, n = 0 and n = 16384: the header's numbers every time."""
    rng = np.random.default_rng(3)
    for N, n in ((1, 0), (1, 16384), (65536, 0), (65536, 16384)):
        a = mcl.Filter(rooms[0], N, 1)
        assert a.status == abi.OK and a.last_counts() == (0, 0, 0)
        assert a.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1)) == abi.OK and a.last_counts() == mcl.INIT_COUNTS
        for _ in range(2):                                                      # one update that skips resampling and one that runs it
            rc, r = a.update((0.1, 0.0, 0.01), mc.cloud(rng, n))
            assert rc == abi.OK and r["n_beams"] == n and a.last_counts() == mcl.UPDATE_COUNTS
        assert r["resampled"] == (1 if N > 1 and n > 0 else 0)
        a.close()
    assert mcl.UPDATE_COUNTS[0] == 4 and mcl.FIELD_COUNTS[0] == 2 and mcl.INIT_COUNTS[0] == 1


def test_one_filter_through_init_updates_and_init_again(rooms):
    rng = np.random.default_rng(8)
    a, b = pair(rooms, 700, 21)
    clouds = [mc.cloud(rng, 45) for _ in range(3)]
    first = []
    for round_ in range(2):
        assert a.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1)) == b.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1)) == abi.OK
        same_state(a.download(), b.download(), "init")
        assert (a.download()["Q"] == 0).all() and (a.download()["ancestors"] == np.arange(700)).all()
        out = [step_both(a, b, (0.1, 0.01, 0.03), pts, (round_, k)) for k, pts in enumerate(clouds)]
        assert [r["update"] for r in out] == [1, 2, 3] and [r["resampled"] for r in out] == [0, 1, 0]
        first.append((out, a.download()))
    same_state(first[0][1], first[1][1])                                        # the counter went back to 0: the same draws again
    assert first[0][0] == first[1][0]
    st = a.download()
    assert a.update((float("nan"), 0, 0), clouds[0])[0] == abi.ERR_BAD_ARGUMENT and a.last_counts() == mcl.UPDATE_COUNTS
    same_state(a.download(), st)
    a.close(); b.close()


def test_the_match_cloud_of_a_device_scan_filter_feeds_a_device_filter(solver, rooms):
    rng = np.random.default_rng(17)
    scan = mc.cast(mc.ROOM_CENTRE, 360)
    scan[:, 2] = 0.1 * rng.normal(size=len(scan))
    clouds = []
    for s in (solver, None):
        sf = sfl.ScanFilter(solver=s)
        rc, recs = sf.process([scan])
        assert rc == abi.OK and recs[0]["status"] == abi.OK, sf.last_error()
        clouds.append(sf.match_cloud(0))
        sf.close()
    same(clouds[0], clouds[1])
    assert 10 < len(clouds[0]) <= len(scan)
    a, b = pair(rooms, 500, 4)
    assert a.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1)) == b.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1)) == abi.OK
    step_both(a, b, (0.0, 0.0, 0.0), clouds[0], "dev cloud")
    r = step_both(a, b, (0.0, 0.0, 0.0), clouds[1], "twin cloud")
    assert r["resampled"] == 1 and a.download()["Q"].any()
    a.close(); b.close()
