"""Laser sub-maps on the GPU (include/visfs_submap.h): the device grids against the host restatement byte for byte (a robot loop
at workload size, and every case of tests/submap_cases.py: batches of 1 to 65 insertions, growth and life-cycle events inside a
batch, the chunks of a column, the refusals), and the laser window solved against the resident matching grid against the same
window with the grid handed over from the host."""
import ctypes as C
import math

import numpy as np
import pytest

from test_submap_cases import CASES, check_known, check_not_finite, check_too_far, snapshot_of
from visfs_amd import abi, backend, synth
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu


def room_scan(T, room, n_ret, rng, n_miss=3, max_range=30.0, origin=(0.0, 0.0, 0.0)):
    """One range data in the robot frame of T: returns on the walls of an axis-aligned room (max_range caps them),
    a few misses at max_range through a doorway-like gap."""
    x0, x1, y0, y1 = room
    R, t = np.asarray(T).reshape(3, 4)[:, :3], np.asarray(T).reshape(3, 4)[:, 3]
    ang = rng.uniform(0, 2 * np.pi, n_ret)
    d = np.stack([np.cos(ang), np.sin(ang)], -1)
    with np.errstate(divide="ignore"):
        tx = np.where(d[:, 0] > 0, (x1 - t[0]) / d[:, 0], (x0 - t[0]) / d[:, 0])
        ty = np.where(d[:, 1] > 0, (y1 - t[1]) / d[:, 1], (y0 - t[1]) / d[:, 1])
    r = np.minimum(np.minimum(tx, ty) + 0.01 * rng.normal(size=n_ret), max_range)
    pw = np.stack([t[0] + r * d[:, 0], t[1] + r * d[:, 1], np.full(n_ret, t[2])], -1)
    ret = (pw - t) @ R
    ma = rng.uniform(0, 2 * np.pi, n_miss)
    mis = np.stack([max_range * np.cos(ma), max_range * np.sin(ma), np.zeros(n_miss)], -1)
    return (list(origin), ret, mis)


def pose(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return [c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, 0.0]


def compare(dev, host):
    dd, hd = dev.describe(), host.describe()
    assert dd == hd
    for i in range(len(dd)):
        cd, fd = dev.download(i)
        ch, fh = host.download(i)
        assert np.array_equal(cd, ch), i
        assert fd.tobytes() == fh.tobytes(), i
    return dd


def test_device_submaps_equal_the_host_restatement():
    """120 frames of a robot loop through a 24 m x 16 m room, 2 range data of ~500 returns + misses each: growth,
    add / finish / drop, and the frame that reads a cropped finished front."""
    s = backend.Solver(abi.default_params())
    dev = sm.Submaps(sm.default_params(), solver=s)
    host = sm.Submaps(sm.default_params())
    rng = np.random.default_rng(4)
    room = (-12.0, 12.0, -8.0, 8.0)
    saw = dict(grown=False, finished_front=False, two=False, dropped=False)
    prev = None
    for f in range(120):
        a = 2 * math.pi * f / 120
        T = pose(8.0 * math.cos(a), 5.0 * math.sin(a), a + math.pi / 2)
        rds = [room_scan(T, room, 500 + 7 * k, rng, origin=(0.05 * k, 0.0, 0.0)) for k in range(2)]
        assert dev.insert(T, rds) == abi.OK
        assert host.insert(T, rds) == abi.OK
        d = compare(dev, host)
        saw["grown"] |= any(x["num_x_cells"] > 100 and not x["finished"] for x in d)
        saw["finished_front"] |= bool(d[0]["finished"])
        saw["two"] |= len(d) == 2
        if prev is not None and prev[0]["finished"]:
            saw["dropped"] |= not d[0]["finished"]
        prev = d
    assert all(saw.values()), saw
    dev.close(); host.close(); s.close()


def test_insert_free_space_and_tsdf_on_device():
    s = backend.Solver(abi.default_params())
    a = sm.Submaps(sm.default_params(insert_free_space=1, num_range_data_limit=2), solver=s)
    b = sm.Submaps(sm.default_params(insert_free_space=0, num_range_data_limit=2), solver=s)
    rng = np.random.default_rng(9)
    for f in range(5):
        T = pose(0.3 * f, 0.1 * f, 0.2 * f)
        rds = [room_scan(T, (-5.0, 5.0, -4.0, 4.0), 200, rng)]
        assert a.insert(T, rds) == b.insert(T, rds) == abi.OK
    assert a.describe() == b.describe()
    for i in range(len(a.describe())):
        assert np.array_equal(a.download(i)[0], b.download(i)[0])
    p = sm.default_params(grid_map_type=1)
    h = C.c_void_p()
    assert sm.load().visfs_submaps_create(s.h, C.byref(p), C.byref(h)) == abi.ERR_UNSUPPORTED
    a.close(); b.close(); s.close()


def test_empty_range_data_count_toward_the_limit():
    s = backend.Solver(abi.default_params())
    dev = sm.Submaps(sm.default_params(num_range_data_limit=3), solver=s)
    host = sm.Submaps(sm.default_params(num_range_data_limit=3))
    rng = np.random.default_rng(2)
    empty = ([0.0, 0.0, 0.0], np.zeros((0, 3)), np.zeros((0, 3)))
    for f in range(8):
        T = pose(0.2 * f, 0.0, 0.1 * f)
        rds = [empty, room_scan(T, (-4.0, 4.0, -3.0, 3.0), 100, rng)] if f % 2 else [empty]
        assert dev.insert(T, rds) == host.insert(T, rds) == abi.OK
        compare(dev, host)
    d = dev.describe()
    assert sum(x["num_range_data"] for x in d) > 0
    dev.close(); host.close(); s.close()


# ---------------------------------------------------------------- the shared cases: batch, chunk, growth and life-cycle edges
CASE_IDS = [c["name"] for c in CASES]
_twin = {}


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


@pytest.fixture
def device_maps(solver):
    """Device sub-maps on the shared solver, closed after the test whether it passed or not (before the solver goes)."""
    made = []

    def make(**params):
        made.append(sm.Submaps(sm.default_params(**params), solver=solver))
        return made[-1]

    yield make
    for m in made:
        m.close()


def twin_states(case):
    """The twin's (describe, [(cells, mirror)]) after every call of the case, computed once and shared."""
    if case["name"] not in _twin:
        host = sm.Submaps(sm.default_params(**case["params"]))
        states = []
        for T, rds in case["calls"]:
            assert host.insert(T, rds) == abi.OK
            d = host.describe()
            states.append((d, [host.download(i) for i in range(len(d))]))
        host.close()
        _twin[case["name"]] = states
    return _twin[case["name"]]


def compare_state(dev, state):
    d, grids = state
    assert dev.describe() == d
    for i, (ch, fh) in enumerate(grids):
        cd, fd = dev.download(i)
        assert np.array_equal(cd, ch), i
        assert fd.tobytes() == fh.tobytes(), i


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_on_device_equals_the_twin_after_every_call(device_maps, case):
    dev = device_maps(**case["params"])
    for (T, rds), state in zip(case["calls"], twin_states(case)):
        assert dev.insert(T, rds) == abi.OK, dev.last_error()
        compare_state(dev, state)
    check_known(case, dev)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_on_device_downloaded_at_the_end_only(device_maps, case):
    """No download (and so no synchronisation) between the calls: each call stages its records with the last ones in flight."""
    dev = device_maps(**case["params"])
    for T, rds in case["calls"]:
        assert dev.insert(T, rds) == abi.OK, dev.last_error()
    compare_state(dev, twin_states(case)[-1])
    check_known(case, dev)


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_two_device_objects_interleaved_on_one_solver(device_maps, k):
    """Case k and the next one, their calls taken in turn on two objects of one solver (one stream)."""
    pair = [CASES[k], CASES[(k + 1) % len(CASES)]]
    devs = [device_maps(**c["params"]) for c in pair]
    for j in range(max(len(c["calls"]) for c in pair)):
        for c, dev in zip(pair, devs):
            if j < len(c["calls"]):
                assert dev.insert(*c["calls"][j]) == abi.OK, dev.last_error()
    for c, dev in zip(pair, devs):
        compare_state(dev, twin_states(c)[-1])
        check_known(c, dev)


def test_growth_beyond_the_cell_limit_is_refused_on_device_as_on_the_twin(device_maps):
    dev = device_maps()
    host = sm.Submaps(sm.default_params())

    def reference(T, rds):
        assert host.insert(T, rds) == abi.OK

    check_too_far(dev, lambda: compare(dev, host), reference)
    host.close()


def test_a_return_that_is_not_finite_changes_nothing_on_device(device_maps):
    dev = device_maps()
    check_not_finite(dev, lambda: snapshot_of(dev))


def _laser_window(with_visual, seed=0):
    w = synth.make_laser_window(with_visual=with_visual, n_points=500, seed=seed)
    return w


def _fill(sub, w, n_frames, rng):
    room = w["grid"]["room"]
    Ttrue = np.asarray(w["truth_Twr"]).reshape(-1, 12)
    for f in range(n_frames):
        T = Ttrue[f % len(Ttrue)].tolist()
        assert sub.insert(T, [room_scan(T, room, 400, rng), room_scan(T, room, 300, rng)]) == abi.OK


def _solve_pair(w, framework, sub, s):
    wb = abi.WindowBuffers(w)
    rc_r, rb_r = sub.solve_window(wb, s)
    cells, cost = sub.download(0)
    d = sub.describe()[0]
    w2 = dict(w)
    w2["grid"] = dict(resolution=d["resolution"], max_x=d["max_x"], max_y=d["max_y"], cost=cost)
    rc_h, rb_h = s.solve_window(abi.WindowBuffers(w2))
    return rc_r, rb_r, rc_h, rb_h, w2


@pytest.mark.parametrize("framework,with_visual", [(0, False), (0, True), (1, False), (1, True)])
def test_solve_window_reads_the_resident_grid(olib, framework, with_visual):
    prm = abi.default_params(framework=framework, iterations=10, solver=2)
    s = backend.Solver(prm)
    w = _laser_window(with_visual)
    sub = sm.Submaps(sm.default_params(num_range_data_limit=3), solver=s)
    rng = np.random.default_rng(5)
    # no sub-map yet: the window without laser edges
    rc_r, rb_r = sub.solve_window(abi.WindowBuffers(w), s)
    w0 = dict(w); w0["grid"] = None
    rc_0, rb_0 = s.solve_window(abi.WindowBuffers(w0))
    assert rc_r == rc_0 and np.array_equal(rb_r.pose_Twr_out, rb_0.pose_Twr_out) and rb_r.struct.chi2_final == rb_0.struct.chi2_final
    seen_cropped = False
    for step in range(4):                 # after 1, 2, 3, 4 frames (2 range data each, limit 3): frame 3 reads a cropped front
        _fill(sub, w, 1, rng)
        front = sub.describe()[0]
        seen_cropped |= bool(front["finished"])
        rc_r, rb_r, rc_h, rb_h, w2 = _solve_pair(w, framework, sub, s)
        assert rc_r == rc_h == abi.OK
        assert rb_r.pose_Twr_out.tobytes() == rb_h.pose_Twr_out.tobytes()
        assert rb_r.struct.chi2_final == rb_h.struct.chi2_final and rb_r.outliers() == rb_h.outliers()
        assert list(rb_r.struct.iterations_run) == list(rb_h.struct.iterations_run)
        # and the oracle, as the existing laser tests require
        wb_o = abi.WindowBuffers(w2)
        rb_o = abi.ResultBuffers(wb_o.struct.n_poses, wb_o.struct.n_refs)
        rc_o = olib.oracle_solve_window(C.byref(prm), C.byref(wb_o.struct), C.byref(rb_o.struct), 1)
        assert rc_o == abi.OK
        n = rb_o.struct.n_poses_out
        et, er = synth.pose_errors(rb_r.pose_Twr_out[:n], rb_o.pose_Twr_out[:n])
        assert et < 1e-6 and er < 1e-6, (et, er)
        assert abs(rb_r.struct.chi2_final - rb_o.struct.chi2_final) <= 1e-6 * max(1.0, rb_o.struct.chi2_final)
    assert seen_cropped
    sub.close(); s.close()
