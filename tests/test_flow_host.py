"""Lucas-Kanade tracking and stereo triangulation (include/visfs_flow.h) on the host twin: against the NumPy checker of
flow_oracle.py byte for byte, and against the ground truth of the synthetic scenes within the reference's own gates."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as fc
import flow_oracle as fo
from visfs_amd import abi, backend
from visfs_amd import flow


def _twin(width, height, **kw):
    return flow.Flow(flow.default_params(**kw), width, height)


def _checker(width, height, **kw):
    return fo.Tracker(fo.Params(**kw), width, height)


def test_exports_and_defaults():
    lib = flow.load()
    assert lib.visfs_flow_abi_version() == flow.ABI_VERSION == 1
    p = flow.default_params()
    q = fo.Params()
    assert (p.win_size, p.max_level, p.iterations, p.flow_back) == (21, 3, 30, 1) == (q.win_size, q.max_level, q.iterations, q.flow_back)
    for name in ("eps", "min_eig_threshold", "back_gate_track", "back_gate_stereo", "min_depth", "max_depth"):
        assert np.float32(getattr(p, name)) == getattr(q, name), name
    assert (np.float32(p.back_gate_track), np.float32(p.back_gate_stereo)) == (1.5, 0.5)


@pytest.mark.parametrize("size", [(752, 480), (641, 479)])
def test_pyramids_and_derivatives_equal_the_checker(size):
    w, h = size
    first = fc.base_image(w, h)
    left, right, _, _ = fc.moved_pair(w, h)
    f, o = _twin(w, h), _checker(w, h)
    for pair in ((first, first), (left, right)):
        f.push_frame(*pair)
        o.push_frame(*pair)
    for slot, pyr in ((flow.SLOT_PREVIOUS, o.prev), (flow.SLOT_CURRENT, o.cur)):
        for image in (flow.IMAGE_LEFT, flow.IMAGE_RIGHT):
            for level in range(4):
                px, der = f.download_level(slot, image, level)
                assert px.shape == pyr[image][level][0].shape == f.level_size(level)[::-1]
                assert px.tobytes() == pyr[image][level][0].tobytes(), (slot, image, level)
                assert der.tobytes() == pyr[image][level][1].tobytes(), (slot, image, level)
    f.close()


def test_push_frame_honours_the_row_stride():
    w, h = 641, 479
    left, right, _, _ = fc.moved_pair(w, h)
    wide = np.zeros((2, h, w + 23), dtype=np.uint8)
    wide[0, :, :w] = left
    wide[1, :, :w] = right
    a, b = _twin(w, h), _twin(w, h)
    a.push_frame(left, right)
    b.push_frame(wide[0, :, :w], wide[1, :, :w])
    for image in (0, 1):
        for level in range(4):
            pa, da = a.download_level(flow.SLOT_CURRENT, image, level)
            pb, db = b.download_level(flow.SLOT_CURRENT, image, level)
            assert pa.tobytes() == pb.tobytes() and da.tobytes() == db.tobytes()
    a.close(); b.close()


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_track_and_stereo_equal_the_checker(name):
    c = fc.case(name)
    f, o = _twin(c["width"], c["height"], **c["prm"]), _checker(c["width"], c["height"], **c["prm"])
    for pair in c["frames"]:
        f.push_frame(*pair)
        o.push_frame(*pair)
    to, st, err = f.track(c["pts"], c["guess"])
    to_o, st_o, err_o = o.track(c["pts"], c["guess"])
    assert st.tobytes() == st_o.tobytes()
    assert to.tobytes() == to_o.tobytes()
    assert err.tobytes() == err_o.tobytes()
    assert 0 < st.sum() < len(st)                      # both outcomes occur (points beyond the border are among the inputs)
    rt, st2, xyz = f.stereo(c["pts"], flow.camera())
    rt_o, st2_o, xyz_o = o.stereo(c["pts"], fo.Camera())
    assert st2.tobytes() == st2_o.tobytes()
    assert rt.tobytes() == rt_o.tobytes()
    assert xyz.tobytes() == xyz_o.tobytes()
    assert np.isnan(xyz[st2 == 0]).all() and 0 < st2.sum() < len(st2)
    f.close()


@pytest.mark.parametrize("name", list(fc.EDGE_CASES))
def test_edge_case_equals_the_checker(name):
    """The window sizes, pyramid depths, image sizes and iteration limits of fc.EDGE_CASES: track without and with a guess, and
    stereo.  What the checker alone keeps and drops is printed and held to the case's `need`, so that no case compares two empty
    outcomes; smallest_5x5_win_3 keeps nothing and smallest_23x23_win_21 keeps nothing in stereo: bytes only there."""
    c = fc.edge_case(name)
    f, o = _twin(c["width"], c["height"], **c["prm"]), _checker(c["width"], c["height"], **c["prm"])
    for pair in c["frames"]:
        f.push_frame(*pair)
        o.push_frame(*pair)
    for guess, what in ((None, "track"), (c["guess"], "track from a guess")):
        to, st, err = f.track(c["pts"], guess)
        with np.errstate(invalid="ignore"):            # the checker's round-trip distance of the row that is inf
            to_o, st_o, err_o = o.track(c["pts"], guess)
        fc.check_not_vacuous(name, st_o, what)
        assert st.tobytes() == st_o.tobytes(), what
        assert to.tobytes() == to_o.tobytes(), what
        assert err.tobytes() == err_o.tobytes(), what
    rt, st2, xyz = f.stereo(c["pts"], flow.camera(baseline=fc.EDGE_BASELINE))
    with np.errstate(invalid="ignore"):
        rt_o, st2_o, xyz_o = o.stereo(c["pts"], fo.Camera(baseline=fc.EDGE_BASELINE))
    print(f"{name} stereo: the checker keeps {int(st2_o.sum())} of {len(st2_o)}, {int(np.isfinite(xyz_o[:, 0]).sum())} with a depth")
    assert st2.tobytes() == st2_o.tobytes()
    assert rt.tobytes() == rt_o.tobytes()
    assert xyz.tobytes() == xyz_o.tobytes()
    assert np.isnan(xyz[st2 == 0]).all()
    f.close()


def test_edge_pyramid_of_eight_levels_equals_the_checker():
    c = fc.edge_case("levels_8_top_5x5")
    f, o = _twin(c["width"], c["height"], **c["prm"]), _checker(c["width"], c["height"], **c["prm"])
    f.push_frame(*c["frames"][1])
    o.push_frame(*c["frames"][1])
    assert f.level_size(7) == (5, 5)
    for image in (flow.IMAGE_LEFT, flow.IMAGE_RIGHT):
        for level in range(8):
            px, der = f.download_level(flow.SLOT_CURRENT, image, level)
            assert px.tobytes() == o.cur[image][level][0].tobytes(), (image, level)
            assert der.tobytes() == o.cur[image][level][1].tobytes(), (image, level)
    f.close()


def test_triangulation_known_answers():
    """projectDisparityTo3D: zero and negative disparity give NaN; c = cx_right - cx only when both are positive; depth must lie in
    (0.2, 10.0]."""
    p = flow.default_params()
    nan3 = [True] * 3

    def tri(cam, lx, rx, ly=100.0):
        return flow.hook_triangulate(p, cam, [[lx, ly]], [[rx, ly]])[0]

    ident = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    cam = flow.camera(fx=320.0, fy=320.0, cx=300.0, cy=200.0, cx_right=300.0, baseline=0.125, Tir=ident)
    assert list(np.isnan(tri(cam, 400.0, 400.0))) == nan3                       # zero disparity
    assert list(np.isnan(tri(cam, 400.0, 404.0))) == nan3                       # negative disparity
    assert tri(cam, 400.0, 396.0).tolist() == [3.125, -3.125, 10.0]             # W = 0.125 / 4; depth 10.0 passes (z <= max_depth)
    assert list(np.isnan(tri(cam, 400.0, np.nextafter(np.float32(396.0), np.float32(400.0))))) == nan3     # just beyond 10 m
    # the c rule
    cam_c = flow.camera(fx=320.0, fy=320.0, cx=300.0, cy=200.0, cx_right=304.0, baseline=0.125, Tir=ident)
    assert tri(cam_c, 400.0, 388.0).tolist() == [0.78125, -0.78125, 2.5]        # W = 0.125 / (12 + 4)
    cam_0 = flow.camera(fx=320.0, fy=320.0, cx=0.0, cy=200.0, cx_right=304.0, baseline=0.125, Tir=ident)
    assert tri(cam_0, 400.0, 384.0).tolist() == [3.125, -0.78125, 2.5]          # cx not positive: c = 0, W = 0.125 / 16
    assert list(np.isnan(tri(flow.camera(baseline=0.0, Tir=ident), 400.0, 390.0))) == nan3
    # the lower gate is strict: z == 0.2f is dropped, the next float up is kept
    fx = float(np.float32(0.2) * np.float32(512.0))
    cam_n = flow.camera(fx=fx, fy=fx, cx=300.0, cy=200.0, cx_right=300.0, baseline=0.125, Tir=ident)
    assert list(np.isnan(tri(cam_n, 400.0, 336.0))) == nan3                     # W = 2^-9, z = 0.2f
    fx_up = float(np.nextafter(np.float32(fx), np.float32(1e9)))
    cam_u = flow.camera(fx=fx_up, fy=fx_up, cx=300.0, cy=200.0, cx_right=300.0, baseline=0.125, Tir=ident)
    assert tri(cam_u, 400.0, 336.0)[2] == np.nextafter(np.float32(0.2), np.float32(1.0))
    # no gates when min_depth < 0 and max_depth <= 0
    q = flow.default_params(min_depth=-1.0, max_depth=0.0)
    assert flow.hook_triangulate(q, cam, [[400.0, 100.0]], [[399.0, 100.0]])[0].tolist() == [12.5, -12.5, 40.0]
    # the image -> robot transform, and the checker on a spread of pairs
    rng = np.random.default_rng(0)
    left = rng.uniform(0, 700, (200, 2)).astype(np.float32)
    right = left.copy()
    right[:, 0] -= rng.uniform(-2, 40, 200).astype(np.float32)
    Tir = [0.0, -0.6, 0.8, 0.1, -1.0, 0.0, 0.0, 0.05, 0.0, -0.8, -0.6, 0.3]
    xyz = flow.hook_triangulate(p, flow.camera(Tir=Tir), left, right)
    xyz_o = fo.triangulate(left, right, np.ones(200, np.uint8), fo.Camera(Tir=Tir), fo.Params())
    assert xyz.tobytes() == xyz_o.tobytes() and 0 < np.isnan(xyz[:, 0]).sum() < 200


def test_ground_truth_track():
    """Every kept point within 1.5 px of where the motion puts it; at most 10 % dropped.  The NumPy checker alone keeps 300 of 300
    (0 % dropped) on these inputs, error max 0.118 px, median 0.036 px."""
    w, h = 752, 480
    f = _twin(w, h)
    f.push_frame(fc.base_image(w, h), fc.base_image(w, h))
    left, right, _, _ = fc.moved_pair(w, h)
    f.push_frame(left, right)
    fc.check_track_truth(f.track)
    f.close()


@pytest.mark.parametrize("kind", ["plane", "slant", "step"])
def test_ground_truth_stereo(kind):
    """Every kept point within 0.5 px of the true right position and its depth within what 0.5 px of disparity makes there; at most
    10 % of the points whose window is clear of the depth step dropped.  The NumPy checker alone keeps all of them (plane 300 of
    300, slant 300 of 300, step 285 of 285), error max 0.019 / 0.038 / 0.023 px."""
    w, h = 752, 480
    left, right, d = fc.still_pair(w, h, kind)
    f = _twin(w, h)
    f.push_frame(left, right)
    cam = flow.camera()
    fc.check_stereo_truth(lambda p: f.stereo(p, cam), kind, d.fb)
    f.close()


def test_points_outside_and_on_a_constant_patch_are_dropped():
    w, h = 752, 480
    a, b, centre = fc.constant_patch_pair(w, h)
    f = _twin(w, h)
    f.push_frame(a, a)
    f.push_frame(b, b)
    outside = np.array([[-40.0, 100.0], [w + 25.0, 100.0], [100.0, -35.5], [100.0, h + 30.0]], dtype=np.float32)
    to, st, err = f.track(outside)
    assert st.tolist() == [0, 0, 0, 0] and err.tolist() == [0.0] * 4
    to, st, err = f.track(centre)
    assert st.tolist() == [0] and err[0] < 1e-4
    rt, st, xyz = f.stereo(np.concatenate([outside, centre]), flow.camera())
    assert st.tolist() == [0] * 5 and np.isnan(xyz).all()
    f.close()


def test_round_trip_gate_rejects_by_distance_alone():
    """A region of the second frame holds a foreign texture.  The checker names the points whose forward and reverse pass both
    succeed and whose round trip misses the start by more than the gate; the library must drop exactly what the checker drops."""
    w, h = 752, 480
    a, b, pts = fc.replaced_region_pair(w, h)
    o = _checker(w, h)
    o.push_frame(a, a)
    o.push_frame(b, b)
    to_o, st_o, err_o, det = o.track(pts, detail=True)
    by_distance = (det["forward"] == 1) & (det["reverse"] == 1) & ~(det["dist"] <= np.float32(1.5))
    assert by_distance.sum() >= 1 and st_o.sum() >= 1
    f = _twin(w, h)
    f.push_frame(a, a)
    f.push_frame(b, b)
    to, st, err = f.track(pts)
    assert (st[by_distance] == 0).all()
    assert st.tobytes() == st_o.tobytes() and to.tobytes() == to_o.tobytes() and err.tobytes() == err_o.tobytes()
    # without the reverse pass the same points are kept
    g = _twin(w, h, flow_back=0)
    g.push_frame(a, a)
    g.push_frame(b, b)
    assert (g.track(pts)[1][by_distance] == 1).all()
    f.close(); g.close()


def test_slot_rotation_over_a_sequence():
    frames = fc.sequence(6)
    h, w = frames[0][0].shape
    f, o = _twin(w, h), _checker(w, h)
    pts = fo.random_points(60, w, h, 12, seed=2)
    for k, pair in enumerate(frames):
        f.push_frame(*pair)
        o.push_frame(*pair)
        if k == 0:
            continue
        got, want = f.track(pts), o.track(pts)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), k
        got, want = f.stereo(pts, flow.camera()), o.stereo(pts, fo.Camera())
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), k
    f.close()


def test_argument_checks():
    lib = flow.load()
    h = C.c_void_p()
    for kw, rc in ((dict(win_size=23), abi.ERR_UNSUPPORTED), (dict(max_level=8), abi.ERR_UNSUPPORTED), (dict(iterations=-1), abi.ERR_BAD_ARGUMENT),
                   (dict(eps=float("nan")), abi.ERR_BAD_ARGUMENT), (dict(win_size=2), abi.ERR_UNSUPPORTED)):
        p = flow.default_params(**kw)
        assert lib.visfs_flow_create_host(C.byref(p), 752, 480, C.byref(h)) == rc, kw
    p = flow.default_params()
    assert lib.visfs_flow_create_host(C.byref(p), 120, 100, C.byref(h)) == abi.ERR_BAD_ARGUMENT      # top level 15 x 13 < window
    p = flow.default_params(win_size=3, max_level=0)
    assert lib.visfs_flow_create_host(C.byref(p), 4, 4, C.byref(h)) == abi.ERR_BAD_ARGUMENT          # smaller than win_size + 2
    _twin(5, 5, win_size=3, max_level=0).close()                                                      # exactly win_size + 2: created
    _twin(752, 480, win_size=4).close()                                                               # an even window: created
    f = _twin(320, 240)
    with pytest.raises(backend.BackendError):
        f.stereo([[10.0, 10.0]], flow.camera())                                                       # no frame yet
    img = np.zeros((240, 320), dtype=np.uint8)
    f.push_frame(img, img)
    with pytest.raises(backend.BackendError):
        f.track([[10.0, 10.0]])                                                                       # one frame only
    f.push_frame(img, img)
    to, st, err = f.track(np.zeros((0, 2), dtype=np.float32))
    assert len(to) == len(st) == len(err) == 0
    f.close()
