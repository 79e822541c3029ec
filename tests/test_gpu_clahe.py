"""The equalised frame push on the GPU (include/visfs_clahe.h): the device path against the host twin byte for byte (final
histograms, look-up tables, the equalised level 0, every pyramid level and derivative) on the cases of tests/clahe_cases.py and on
one 752 x 480 pair, track and corners behind it, a plain push_frame afterwards, and two objects plus a BA solve on one handle."""
import numpy as np
import pytest

import clahe_cases as cc
import flow_cases as fc
from visfs_amd import abi, backend, clahe, corners, flow, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _same_state(dev, host, levels):
    for image in (clahe.IMAGE_LEFT, clahe.IMAGE_RIGHT):
        a, b = clahe.download(dev, image), clahe.download(host, image)
        assert a["hist"].tobytes() == b["hist"].tobytes(), image
        assert a["lut"].tobytes() == b["lut"].tobytes(), image
        for level in range(levels):
            pa, pb = dev.download_level(flow.SLOT_CURRENT, image, level), host.download_level(flow.SLOT_CURRENT, image, level)
            assert pa[0].tobytes() == pb[0].tobytes(), (image, level)
            assert pa[1].tobytes() == pb[1].tobytes(), (image, level)


@pytest.mark.parametrize("name", cc.NAMES + cc.EDGE_NAMES)
def test_case_equals_the_host_twin(solver, name):
    c = cc.case(name)
    prm = flow.default_params(**c["flow"])
    dev, host = flow.Flow(prm, c["w"], c["h"], solver=solver), flow.Flow(prm, c["w"], c["h"])
    for f in (dev, host):
        clahe.push_frame(f, clahe.default_params(**c["params"]), c["left"], c["right"])
    _same_state(dev, host, c["flow"]["max_level"] + 1)
    # the checker's bytes as well: the host tests pin the twin to them, this pins the device without the detour
    for image in (0, 1):
        assert dev.download_level(flow.SLOT_CURRENT, image, 0)[0].tobytes() == cc.expected(name, image)["dst"].tobytes()
    dev.close(); host.close()


def test_full_size_track_and_corners_equal_the_host_twin(solver):
    w, h = 752, 480
    first = cc.big_pair(w, h)
    left, right, _, _ = fc.moved_pair(w, h)
    dev, host = flow.Flow(flow.default_params(), w, h, solver=solver), flow.Flow(flow.default_params(), w, h)
    pts = fc.truth_points(w, h, n=150)
    out = []
    for f in (dev, host):
        clahe.push_frame(f, clahe.default_params(), fc.base_image(w, h), first[1])
        clahe.push_frame(f, clahe.default_params(), left, right)
        out.append((f.track(pts), f.stereo(pts, flow.camera()), corners.corners(f, max_corners=300, min_distance=20.0)))
    _same_state(dev, host, 4)
    (ta, sa, ca), (tb, sb, cb) = out
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ta + sa, tb + sb))
    assert ca.tobytes() == cb.tobytes() and len(ca) > 100
    assert int(ta[1].sum()) > 100
    dev.close(); host.close()


def test_plain_push_frame_afterwards_is_untouched(solver):
    c = cc.case("texture_70x52_c3_t8x8")
    prm = flow.default_params(**cc.FLOW_PARAMS)
    used, fresh = flow.Flow(prm, c["w"], c["h"], solver=solver), flow.Flow(prm, c["w"], c["h"], solver=solver)
    clahe.push_frame(used, clahe.default_params(), c["left"], c["right"])
    clahe.push_frame(used, clahe.default_params(tiles_x=4, tiles_y=2), c["right"], c["left"])
    for f in (used, fresh):
        f.push_frame(c["left"], c["right"])
    for image in (0, 1):
        for level in range(2):
            a, b = used.download_level(flow.SLOT_CURRENT, image, level), fresh.download_level(flow.SLOT_CURRENT, image, level)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert used.download_level(flow.SLOT_CURRENT, image, 0)[0].tobytes() == (c["left"], c["right"])[image].tobytes()
    used.close(); fresh.close()


def test_argument_checks_on_the_device(solver):
    c = cc.case("texture_64x48_c3_t8x8")
    f = flow.Flow(flow.default_params(**cc.FLOW_PARAMS), 64, 48, solver=solver)
    with pytest.raises(backend.BackendError):
        clahe.download(f)
    assert clahe.push_frame_status(f, None, c["left"], c["right"]) == abi.ERR_BAD_ARGUMENT
    assert clahe.push_frame_status(f, clahe.default_params(clip_limit=-1.0), c["left"], c["right"]) == abi.ERR_BAD_ARGUMENT
    assert clahe.push_frame_status(f, clahe.default_params(tiles_x=33), c["left"], c["right"]) == abi.ERR_UNSUPPORTED
    assert clahe.push_frame_status(f, clahe.default_params(tiles_x=32, tiles_y=32), c["left"], c["right"]) == abi.OK
    host = flow.Flow(flow.default_params(**cc.FLOW_PARAMS), 64, 48)
    clahe.push_frame(host, clahe.default_params(tiles_x=32, tiles_y=32), c["left"], c["right"])
    _same_state(f, host, 2)
    f.close(); host.close()


def test_two_objects_and_a_ba_solve_on_one_handle(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))                   # before any equalised push exists on the handle
    assert rc0 == abi.OK
    ca, cb = cc.case("noise_256x128_c3_t8x8"), cc.case("low_contrast_70x52_c3_t8x8")
    prm = flow.default_params(**cc.FLOW_PARAMS)
    a, b = flow.Flow(prm, ca["w"], ca["h"], solver=solver), flow.Flow(prm, cb["w"], cb["h"], solver=solver)
    clahe.push_frame(a, clahe.default_params(**ca["params"]), ca["left"], ca["right"])
    clahe.push_frame(b, clahe.default_params(**cb["params"]), cb["left"], cb["right"])
    st_a = clahe.download(a, 0)                                              # the state of a after b has run
    px_a = a.download_level(flow.SLOT_CURRENT, 0, 0)[0]
    rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
    assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()
    want = cc.expected(ca["name"], 0)
    assert st_a["lut"].tobytes() == want["lut"].tobytes() and st_a["hist"].tobytes() == want["hist"].tobytes()
    assert px_a.tobytes() == want["dst"].tobytes()
    assert b.download_level(flow.SLOT_CURRENT, 1, 0)[0].tobytes() == cc.expected(cb["name"], 1)["dst"].tobytes()
    clahe.push_frame(a, clahe.default_params(**ca["params"]), ca["left"], ca["right"])
    assert a.download_level(flow.SLOT_CURRENT, 0, 0)[0].tobytes() == px_a.tobytes()
    a.close(); b.close()
