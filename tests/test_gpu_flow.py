"""Lucas-Kanade tracking and stereo triangulation on the GPU (include/visfs_flow.h): the device path against the host twin byte for
byte, the resident slot rotation, two trackers and a BA on one handle, and the ground truth of the synthetic scenes."""
import numpy as np
import pytest

import flow_cases as fc
import flow_oracle as fo
from visfs_amd import abi, backend, synth
from visfs_amd import flow

pytestmark = pytest.mark.gpu


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _same(got, want):
    return all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("size", [(752, 480), (641, 479)])
def test_device_pyramids_equal_the_host_twin(solver, size):
    w, h = size
    first = fc.base_image(w, h)
    left, right, _, _ = fc.moved_pair(w, h)
    dev, host = flow.Flow(flow.default_params(), w, h, solver=solver), flow.Flow(flow.default_params(), w, h)
    for pair in ((first, first), (left, right)):
        dev.push_frame(*pair)
        host.push_frame(*pair)
    for slot in (flow.SLOT_PREVIOUS, flow.SLOT_CURRENT):
        for image in (flow.IMAGE_LEFT, flow.IMAGE_RIGHT):
            for level in range(4):
                assert _same(dev.download_level(slot, image, level), host.download_level(slot, image, level)), (slot, image, level)
    dev.close(); host.close()


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_device_track_and_stereo_equal_the_host_twin(solver, name):
    c = fc.case(name)
    p = flow.default_params(**c["prm"])
    dev, host = flow.Flow(p, c["width"], c["height"], solver=solver), flow.Flow(p, c["width"], c["height"])
    for pair in c["frames"]:
        dev.push_frame(*pair)
        host.push_frame(*pair)
    got, want = dev.track(c["pts"], c["guess"]), host.track(c["pts"], c["guess"])
    assert got[1].tobytes() == want[1].tobytes()
    assert _same(got, want)
    assert 0 < got[1].sum() < len(got[1])
    cam = flow.camera(Tir=[0.0, -0.6, 0.8, 0.1, -1.0, 0.0, 0.0, 0.05, 0.0, -0.8, -0.6, 0.3])
    got, want = dev.stereo(c["pts"], cam), host.stereo(c["pts"], cam)
    assert got[1].tobytes() == want[1].tobytes()
    assert _same(got, want)
    assert 0 < got[1].sum() < len(got[1])
    dev.close(); host.close()


@pytest.mark.parametrize("name", list(fc.EDGE_CASES))
def test_device_edge_case_equals_the_host_twin(solver, name):
    """fc.EDGE_CASES on the device: the slot occupancies of the wavefront's window cells, 0 / 255 images under the int32 partial sums,
    the 8-level layout, the smallest images and the iteration limits.  tests/test_flow_host.py holds the twin to the checker on the
    same inputs and the checker's counts to the case's `need`."""
    c = fc.edge_case(name)
    p = flow.default_params(**c["prm"])
    dev, host = flow.Flow(p, c["width"], c["height"], solver=solver), flow.Flow(p, c["width"], c["height"])
    for pair in c["frames"]:
        dev.push_frame(*pair)
        host.push_frame(*pair)
    if c["prm"]["max_level"] == 7:
        for slot in (flow.SLOT_PREVIOUS, flow.SLOT_CURRENT):
            for image in (flow.IMAGE_LEFT, flow.IMAGE_RIGHT):
                for level in range(8):
                    assert _same(dev.download_level(slot, image, level), host.download_level(slot, image, level)), (slot, image, level)
    for guess in (None, c["guess"]):
        got, want = dev.track(c["pts"], guess), host.track(c["pts"], guess)
        print(f"{name} track{' from a guess' if guess is not None else ''}: the twin keeps {int(want[1].sum())} of {len(want[1])}")
        assert got[1].tobytes() == want[1].tobytes()
        assert _same(got, want)
    cam = flow.camera(baseline=fc.EDGE_BASELINE)
    got, want = dev.stereo(c["pts"], cam), host.stereo(c["pts"], cam)
    assert got[1].tobytes() == want[1].tobytes()
    assert _same(got, want)
    dev.close(); host.close()


def test_slot_rotation_over_twenty_frames(solver):
    frames = fc.sequence(20)
    h, w = frames[0][0].shape
    dev, host = flow.Flow(flow.default_params(), w, h, solver=solver), flow.Flow(flow.default_params(), w, h)
    pts = fo.random_points(100, w, h, 12, seed=2)
    cam = flow.camera()
    kept = 0
    for k, pair in enumerate(frames):
        dev.push_frame(*pair)
        host.push_frame(*pair)
        if k:
            got, want = dev.track(pts), host.track(pts)
            assert _same(got, want), k
            kept += int(got[1].sum())
            for slot in (flow.SLOT_PREVIOUS, flow.SLOT_CURRENT):
                assert _same(dev.download_level(slot, flow.IMAGE_LEFT, 2), host.download_level(slot, flow.IMAGE_LEFT, 2)), k
        assert _same(dev.stereo(pts, cam), host.stereo(pts, cam)), k
    assert kept > 0
    dev.close(); host.close()


def test_two_trackers_on_one_handle_do_not_disturb_each_other(solver):
    w, h = 752, 480
    first = fc.base_image(w, h)
    left, right, _, _ = fc.moved_pair(w, h)
    pts = fc.truth_points(w, h, n=120)
    a = flow.Flow(flow.default_params(), w, h, solver=solver)
    a.push_frame(first, first)
    a.push_frame(left, right)
    before = a.track(pts)
    b = flow.Flow(flow.default_params(max_level=2), w, h, solver=solver)        # other frames, other parameters, same stream
    b.push_frame(right, left)
    b.push_frame(first, right)
    other = b.track(pts)
    assert _same(a.track(pts), before)
    for level in range(4):
        host = flow.Flow(flow.default_params(), w, h)
        host.push_frame(first, first)
        host.push_frame(left, right)
        assert _same(a.download_level(flow.SLOT_CURRENT, flow.IMAGE_RIGHT, level), host.download_level(flow.SLOT_CURRENT, flow.IMAGE_RIGHT, level))
        host.close()
    hb = flow.Flow(flow.default_params(max_level=2), w, h)
    hb.push_frame(right, left)
    hb.push_frame(first, right)
    assert _same(other, hb.track(pts))
    a.close(); b.close(); hb.close()


def test_ba_between_flow_calls_returns_the_same_bytes(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    w, h = 752, 480
    left, right, _, _ = fc.moved_pair(w, h)
    f = flow.Flow(flow.default_params(), w, h, solver=solver)
    f.push_frame(fc.base_image(w, h), fc.base_image(w, h))
    f.push_frame(left, right)
    pts = fc.truth_points(w, h, n=150)
    t0 = f.track(pts)
    rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
    s0 = f.stereo(pts, flow.camera())
    assert rc1 == rc0
    assert rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
    assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()
    assert _same(f.track(pts), t0) and _same(f.stereo(pts, flow.camera()), s0)
    f.close()


def test_ground_truth_track_on_the_device(solver):
    """As tests/test_flow_host.py::test_ground_truth_track: 1.5 px, at most 10 % dropped (the checker alone: 0 %)."""
    w, h = 752, 480
    f = flow.Flow(flow.default_params(), w, h, solver=solver)
    f.push_frame(fc.base_image(w, h), fc.base_image(w, h))
    left, right, _, _ = fc.moved_pair(w, h)
    f.push_frame(left, right)
    fc.check_track_truth(f.track)
    f.close()


@pytest.mark.parametrize("kind", ["plane", "slant", "step"])
def test_ground_truth_stereo_on_the_device(solver, kind):
    """As tests/test_flow_host.py::test_ground_truth_stereo: 0.5 px, the depth that 0.5 px of disparity makes, at most 10 % dropped."""
    w, h = 752, 480
    left, right, d = fc.still_pair(w, h, kind)
    f = flow.Flow(flow.default_params(), w, h, solver=solver)
    f.push_frame(left, right)
    cam = flow.camera()
    fc.check_stereo_truth(lambda p: f.stereo(p, cam), kind, d.fb)
    f.close()


def test_dropped_points_and_the_gate_on_the_device(solver):
    w, h = 752, 480
    a, b, centre = fc.constant_patch_pair(w, h)
    f = flow.Flow(flow.default_params(), w, h, solver=solver)
    f.push_frame(a, a)
    f.push_frame(b, b)
    outside = np.array([[-40.0, 100.0], [w + 25.0, 100.0], [100.0, -35.5], [100.0, h + 30.0]], dtype=np.float32)
    to, st, err = f.track(np.concatenate([outside, centre]))
    assert st.tolist() == [0] * 5
    # the round-trip gate: what the checker rejects by distance alone
    a, b, pts = fc.replaced_region_pair(w, h)
    o = fo.Tracker(fo.Params(), w, h)
    o.push_frame(a, a)
    o.push_frame(b, b)
    to_o, st_o, err_o, det = o.track(pts, detail=True)
    by_distance = (det["forward"] == 1) & (det["reverse"] == 1) & ~(det["dist"] <= np.float32(1.5))
    assert by_distance.sum() >= 1
    f.push_frame(a, a)
    f.push_frame(b, b)
    to, st, err = f.track(pts)
    assert (st[by_distance] == 0).all()
    assert st.tobytes() == st_o.tobytes() and to.tobytes() == to_o.tobytes() and err.tobytes() == err_o.tobytes()
    f.close()


def test_more_points_than_the_initial_capacity(solver):
    w, h = 320, 240
    frames = fc.sequence(2)
    dev, host = flow.Flow(flow.default_params(), w, h, solver=solver), flow.Flow(flow.default_params(), w, h)
    for pair in frames:
        dev.push_frame(*pair)
        host.push_frame(*pair)
    pts = fo.random_points(1500, w, h, 5, seed=9)
    assert _same(dev.track(pts), host.track(pts))
    assert _same(dev.track(pts[:10]), host.track(pts[:10]))
    dev.close(); host.close()
