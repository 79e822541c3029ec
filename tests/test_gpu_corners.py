"""Corner extraction on the GPU (include/visfs_corners.h): the device path against the host twin byte for byte (corners, response
map, mask, draw decisions, candidate count, maximum), the resident slot rotation, two trackers and a BA on one handle, and the full
step push_frame -> track -> corners behind the mask -> stereo."""
import numpy as np
import pytest

import corners_cases as cc
import corners_oracle as co
import flow_cases as fc
from visfs_amd import abi, backend, corners, flow, synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _pair(img, solver, **flow_kw):
    h, w = img.shape
    dev, host = flow.Flow(flow.default_params(**flow_kw), w, h, solver=solver), flow.Flow(flow.default_params(**flow_kw), w, h)
    dev.push_frame(img, img)
    host.push_frame(img, img)
    return dev, host


def _same_call(dev, host, discs=None, **kw):
    got, want = corners.corners(dev, discs=discs, **kw), corners.corners(host, discs=discs, **kw)
    n = 0 if discs is None else len(discs)
    a, b = corners.download(dev, n), corners.download(host, n)
    for key in ("eig", "mask", "disc_drawn", "max_val"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_candidates"] == b["n_candidates"]
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    return got, a


@pytest.mark.parametrize("size", cc.SIZES)
def test_base_image_equals_the_host_twin(solver, size):
    w, h = size
    dev, host = _pair(fc.base_image(w, h), solver)
    counts = set()
    for md in cc.MIN_DISTANCES:
        for mc in cc.MAX_CORNERS:
            got, st = _same_call(dev, host, max_corners=mc, min_distance=md)
            counts.add(len(got) == mc)
            assert st["n_candidates"] > cc.DEVICE_TILE
    assert counts == {True, False}
    dev.close(); host.close()


@pytest.mark.parametrize("name", list(cc.EDGE))
def test_edge_case_equals_the_host_twin(solver, name):
    """cc.EDGE on the device: both image borders inside one workgroup of the response kernel, and the selection's other paths.
    tests/test_corners_host.py holds the twin to the checker on the same inputs and states what the checker returns."""
    w, h, kw = cc.EDGE[name]
    dev, host = _pair(cc.edge_image(w, h), solver, **cc.EDGE_FLOW_PARAMS)
    got, st = _same_call(dev, host, **kw)
    want = cc.edge_checked(name)
    assert got.tobytes() == want["xy"].tobytes() and st["n_candidates"] == want["n_candidates"]
    assert st["eig"].tobytes() == want["eig"].tobytes()
    dev.close(); host.close()


def test_ties_equal_the_host_twin(solver):
    dev, host = _pair(cc.tiled_image(), solver)
    for md in (10.0, 0.0):
        got, _ = _same_call(dev, host, max_corners=300, min_distance=md)
        assert len(got) == 300
    dev.close(); host.close()


def test_many_candidates_equal_the_host_twin(solver):
    dev, host = _pair(fc.base_image(752, 480), solver)
    got, st = _same_call(dev, host, max_corners=4096, quality_level=1e-6, min_distance=0.0)
    assert len(got) == 4096 and st["n_candidates"] > 4 * cc.DEVICE_TILE
    dev.close(); host.close()
    dev, host = _pair(cc.noise_image(), solver)
    for md, mc in ((7.0, 4096), (3.0, 300), (0.0, 4096)):
        got, st = _same_call(dev, host, max_corners=mc, min_distance=md)
        assert st["n_candidates"] == 23888 and len(got) > 0
    dev.close(); host.close()


def test_mask_scenario_equals_the_host_twin(solver):
    w, h = 752, 480
    dev, host = _pair(fc.base_image(w, h), solver)
    discs = cc.mask_scenario(w, h)
    for mc, n in ((204, 66), (20, 20)):
        got, st = _same_call(dev, host, discs=discs, max_corners=mc, min_distance=40.0)
        assert len(got) == n and int(st["disc_drawn"].sum()) == 109 and st["n_candidates"] == 2202
    first = corners.corners(host, max_corners=150, min_distance=40.0)
    fed = [(float(x), float(y), 40) for x, y in first]
    _, st = _same_call(dev, host, discs=fed, max_corners=150, min_distance=40.0)
    assert int(st["disc_drawn"].sum()) == 148
    for name, (discs, drawn) in sorted(cc.special_discs(w, h).items()):
        _, st = _same_call(dev, host, discs=discs, max_corners=300, min_distance=40.0)
        assert st["disc_drawn"].tolist() == drawn, name
    # a call without discs after calls with them: no mask is left behind
    _, st = _same_call(dev, host, max_corners=300, min_distance=40.0)
    assert (st["mask"] == 255).all()
    dev.close(); host.close()


def test_degenerate_inputs_and_argument_checks(solver):
    dev, host = _pair(cc.flat_image(), solver)
    got, st = _same_call(dev, host, max_corners=300, min_distance=40.0)
    assert len(got) == 0 and st["n_candidates"] == 0 and st["max_val"] == 0
    dev.close(); host.close()
    dev, host = _pair(fc.base_image(320, 240), solver)
    got, st = _same_call(dev, host, discs=cc.full_cover_discs(320, 240), max_corners=300, min_distance=40.0)
    assert len(got) == 0 and (st["mask"] == 0).all() and st["max_val"].tobytes() == np.float32(0).tobytes()
    assert corners.corners_status(dev, slot=corners.SLOT_PREVIOUS)[0] == abi.ERR_NOT_LOADED
    assert corners.corners_status(dev, max_corners=0)[0] == abi.ERR_BAD_ARGUMENT
    assert corners.corners_status(dev, max_corners=4097, capacity=5000)[0] == abi.ERR_UNSUPPORTED
    assert corners.corners_status(dev, max_corners=300, capacity=299)[0] == abi.ERR_BAD_ARGUMENT
    assert corners.corners_status(dev, discs=[(float("nan"), 3.0, 5)])[0] == abi.ERR_BAD_ARGUMENT
    assert corners.corners_status(dev, discs=[(3.0, 3.0, -1)])[0] == abi.ERR_BAD_ARGUMENT
    dev.close(); host.close()
    fresh = flow.Flow(flow.default_params(), 320, 240, solver=solver)
    assert corners.corners_status(fresh)[0] == abi.ERR_NOT_LOADED
    with pytest.raises(backend.BackendError):
        corners.download(fresh)
    fresh.close()


def test_ground_truth_squares_on_the_device(solver):
    """As tests/test_corners_host.py::test_ground_truth_squares: within 1 px both ways."""
    img, truth = cc.squares_image()
    dev, host = _pair(img, solver)
    got, _ = _same_call(dev, host, max_corners=300, min_distance=10.0)
    d = np.sqrt(((got.astype(np.float64)[:, None, :] - truth[None]) ** 2).sum(-1))
    print(f"squares on the device: {len(got)} corners for {len(truth)}; max {d.min(1).max():.3f} / {d.min(0).max():.3f} px")
    assert len(got) == 160 and d.min(1).max() <= 1.0 and d.min(0).max() <= 1.0
    dev.close(); host.close()


def test_slots_after_a_rotation_over_several_frames(solver):
    frames = fc.sequence(6)
    h, w = frames[0][0].shape
    dev, host = flow.Flow(flow.default_params(), w, h, solver=solver), flow.Flow(flow.default_params(), w, h)
    for k, pair in enumerate(frames):
        dev.push_frame(*pair)
        host.push_frame(*pair)
        for slot in ((corners.SLOT_CURRENT, corners.SLOT_PREVIOUS) if k else (corners.SLOT_CURRENT,)):
            for image in (corners.IMAGE_LEFT, corners.IMAGE_RIGHT):
                got, _ = _same_call(dev, host, slot=slot, image=image, max_corners=300, min_distance=20.0)
                src = frames[k if slot == corners.SLOT_CURRENT else k - 1][image]
                if k in (0, 5):
                    assert got.tobytes() == co.good_features(src, 300, 0.01, 20.0)["xy"].tobytes()
    dev.close(); host.close()


def test_two_trackers_on_one_handle_do_not_disturb_each_other(solver):
    w, h = 752, 480
    a_img, b_img = fc.base_image(w, h), cc.noise_image(w, h)
    a = flow.Flow(flow.default_params(), w, h, solver=solver)
    b = flow.Flow(flow.default_params(max_level=2), w, h, solver=solver)
    a.push_frame(a_img, a_img)
    b.push_frame(b_img, a_img)
    discs = cc.mask_scenario(w, h)
    before = corners.corners(a, discs=discs, max_corners=204)
    other = corners.corners(b, max_corners=300, min_distance=7.0)
    st_a = corners.download(a, len(discs))
    assert corners.corners(a, discs=discs, max_corners=204).tobytes() == before.tobytes()
    host_a, host_b = flow.Flow(flow.default_params(), w, h), flow.Flow(flow.default_params(max_level=2), w, h)
    host_a.push_frame(a_img, a_img)
    host_b.push_frame(b_img, a_img)
    assert before.tobytes() == corners.corners(host_a, discs=discs, max_corners=204).tobytes()
    want_a = corners.download(host_a, len(discs))
    assert st_a["mask"].tobytes() == want_a["mask"].tobytes() and st_a["eig"].tobytes() == want_a["eig"].tobytes()
    assert other.tobytes() == corners.corners(host_b, max_corners=300, min_distance=7.0).tobytes()
    for f in (a, b, host_a, host_b):
        f.close()


def test_ba_and_flow_calls_between_corner_calls_return_the_same_bytes(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    w, h = 752, 480
    left, right, _, _ = fc.moved_pair(w, h)
    f = flow.Flow(flow.default_params(), w, h, solver=solver)
    f.push_frame(fc.base_image(w, h), fc.base_image(w, h))
    f.push_frame(left, right)
    pts = fc.truth_points(w, h, n=150)
    t0, s0 = f.track(pts), f.stereo(pts, flow.camera())               # before the first corner call of the object
    c0 = corners.corners(f, max_corners=300, min_distance=40.0)
    rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
    t1 = f.track(pts)
    c1 = corners.corners(f, max_corners=300, min_distance=40.0)
    s1 = f.stereo(pts, flow.camera())
    assert rc1 == rc0
    assert rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
    assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()
    assert c0.tobytes() == c1.tobytes() and len(c0) > 100
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t0, t1)) and all(x.tobytes() == y.tobytes() for x, y in zip(s0, s1))
    f.close()


def _step(f, frames, max_corners, min_distance, cam):
    """Tracker::imageProcess's pixel path over a sequence: per frame (words after the top-up, new corners, stereo survivors)."""
    h, w = frames[0][0].shape
    pts = np.zeros((0, 2), dtype=np.float32)
    log, outs = [], []
    for k, pair in enumerate(frames):
        f.push_frame(*pair)
        if k:
            to, st, _ = f.track(pts)
            ok = (st == 1) & (to[:, 0] >= 0) & (to[:, 0] < w) & (to[:, 1] >= 0) & (to[:, 1] < h)
            pts = to[ok]
        new = np.zeros((0, 2), dtype=np.float32)
        if len(pts) < max_corners:
            discs = [(float(x), float(y), int(min_distance)) for x, y in pts]
            new = corners.corners(f, discs=discs, max_corners=max_corners - len(pts), min_distance=min_distance)
            pts = np.concatenate([pts, new]).astype(np.float32)
        rt, st, xyz = f.stereo(pts, cam)
        log.append((len(pts), len(new), int(st.sum())))
        outs.append((pts.copy(), new, rt, st, xyz))
    return log, outs


def test_full_step_over_a_sequence_equals_the_host_twin(solver):
    """push_frame -> track -> corners behind the mask of the tracked points -> stereo over 20 frames.  The word count stays at
    max_corners where the image offers that many corners, and otherwise at what the checker alone adds behind the same mask."""
    frames = fc.sequence(20)
    h, w = frames[0][0].shape
    cam = flow.camera()
    for mc, md in ((60, 12.0), (300, 20.0)):
        dev, host = flow.Flow(flow.default_params(), w, h, solver=solver), flow.Flow(flow.default_params(), w, h)
        got_log, got = _step(dev, frames, mc, md, cam)
        want_log, want = _step(host, frames, mc, md, cam)
        assert got_log == want_log
        for a, b in zip(got, want):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        print(f"full step max_corners {mc}, min_distance {md}: (words, new, stereo) per frame {got_log}")
        assert sum(n for _, n, _ in got_log[1:]) > 0                      # lost words were replaced
        for k, (words, new, _) in enumerate(got_log):
            if words < mc:                                               # the checker alone finds no more behind this mask
                pts, new_xy = got[k][0], got[k][1]
                tracked = pts[:len(pts) - len(new_xy)]
                discs = [(float(x), float(y), int(md)) for x, y in tracked]
                ref = co.good_features(frames[k][0], mc - len(tracked), 0.01, md, discs)
                assert ref["exhausted"] and ref["xy"].tobytes() == new_xy.tobytes(), k
        if mc == 60:
            assert all(words == mc for words, _, _ in got_log)
        dev.close(); host.close()
