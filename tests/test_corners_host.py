"""Corner extraction (include/visfs_corners.h) on the host twin: against the NumPy checker of corners_oracle.py byte for byte, and
against the ground truth of planted squares.  Every test first asserts on the checker's output alone that its input takes the
branches it is there for; the counts in the docstrings are what the checker gives."""
import numpy as np
import pytest

import corners_cases as cc
import corners_oracle as co
import flow_cases as fc
from visfs_amd import abi, backend, corners, flow


def _twin(img, **flow_kw):
    h, w = img.shape
    f = flow.Flow(flow.default_params(**flow_kw), w, h)
    f.push_frame(img, img)
    return f


def _compare(f, want, discs=None, **params):
    """The host twin's call and every piece of its state against the checker's dict."""
    got = corners.corners(f, discs=discs, **params)
    n_discs = 0 if discs is None else len(discs)
    st = corners.download(f, n_discs)
    assert st["eig"].tobytes() == want["eig"].tobytes()
    assert st["mask"].tobytes() == want["mask"].tobytes()
    assert st["disc_drawn"].tobytes() == want["disc_drawn"].tobytes()
    assert st["max_val"].tobytes() == want["max_val"].tobytes()
    assert st["n_candidates"] == want["n_candidates"]
    assert len(got) == len(want["xy"])
    assert got.tobytes() == want["xy"].tobytes()
    return got


def test_exports_and_defaults():
    lib = corners.load()
    assert lib.visfs_corners_abi_version() == corners.ABI_VERSION == 1
    assert flow.load().visfs_flow_abi_version() == 1
    for name in corners.EXPORTS:
        assert hasattr(lib, name) and not name.startswith("visfs_ba_")
    p = corners.default_params()
    assert (p.max_corners, p.quality_level, p.min_distance) == (300, 0.01, 40.0)


def test_halfwidth_known_answers():
    """The filled circle of cv::circle is not the Euclidean disc."""
    hw = corners.halfwidth(40)
    assert hw[:6].tolist() == [40, 39, 39, 39, 39, 39] and hw[-6:].tolist() == [19, 17, 15, 12, 8, 0]
    assert corners.halfwidth(20)[[0, 10, 14, 15, 19, 20]].tolist() == [20, 17, 14, 13, 6, 0]
    assert corners.halfwidth(0).tolist() == [0]
    for r in (1, 2, 3, 7, 20, 40, 333):
        assert corners.halfwidth(r).tobytes() == co.halfwidth(r).tobytes(), r
    with pytest.raises(backend.BackendError):
        corners.halfwidth(-1)


# the checker's counts: (candidates at quality 0.01, corners returned at min_distance 40 / 20 / 7 with max_corners 300)
EXPECTED = {(752, 480): (11678, 159, 300, 300), (641, 479): (9910, 136, 300, 300), (320, 240): (2492, 38, 133, 300)}


@pytest.mark.parametrize("size", cc.SIZES)
def test_base_image_equals_the_checker(size):
    """base_image at quality 0.01: 11 678 / 9 910 / 2 492 candidates; min_distance 40 / 20 / 7 return 159 / 300 / 300, 136 / 300 / 300
    and 38 / 133 / 300 corners, so the list runs out in some cases and max_corners cuts in others; min_distance 0 takes the first
    max_corners of the order."""
    w, h = size
    f = _twin(fc.base_image(w, h))
    exhausted = set()
    for md in cc.MIN_DISTANCES:
        for mc in cc.MAX_CORNERS:
            want = cc.checked(w, h, mc, md)
            exhausted.add(bool(want["exhausted"]))
            assert want["n_candidates"] == EXPECTED[size][0]
            if mc == 300 and md >= 1:
                assert len(want["xy"]) == EXPECTED[size][1 + cc.MIN_DISTANCES.index(md)]
            if md == 0:
                assert len(want["xy"]) == mc
            got = _compare(f, want, max_corners=mc, min_distance=md)
            if md >= 1 and len(got) > 1:
                d = got[:, None, :].astype(np.float64) - got[None].astype(np.float64)
                d2 = (d ** 2).sum(-1) + np.eye(len(got)) * 1e9
                assert d2.min() >= md * md
    assert exhausted == {True, False}
    f.close()


def test_ties_are_ordered_by_raster_index_descending():
    """The tiled patch: 63 805 non-zero thresholded responses with only 3 606 distinct values; 300 corners at min_distance 10."""
    img = cc.tiled_image()
    want = co.good_features(img, 300, 0.01, 10.0)
    t = np.float32(np.float64(want["max_val"]) * 0.01)
    nz = want["eig"][want["eig"] > t]
    assert len(nz) == 63805 and len(np.unique(nz)) == 3606
    v = want["order_values"]
    assert (v[1:] == v[:-1]).sum() > 100                       # equal neighbours in the order: the index decided
    assert len(want["xy"]) == 300
    f = _twin(img)
    _compare(f, want, max_corners=300, min_distance=10.0)
    want0 = co.good_features(img, 300, 0.01, 0.0)
    _compare(f, want0, max_corners=300, min_distance=0.0)
    # within a run of equal values the raster index falls
    idx = (want0["xy"][:, 1].astype(np.int64) * img.shape[1] + want0["xy"][:, 0].astype(np.int64))
    same = v[1:300] == v[:299]
    assert same.any() and (idx[1:][same] < idx[:-1][same]).all()
    f.close()


def test_many_candidates():
    """quality 1e-6, min_distance 0, max_corners 4096 on base_image; uniform noise (23 888 candidates at quality 0.01): both need
    several of the device's tiles."""
    img = fc.base_image(752, 480)
    want = co.good_features(img, 4096, 1e-6, 0.0)
    assert want["n_candidates"] > 4 * cc.DEVICE_TILE and len(want["xy"]) == 4096
    f = _twin(img)
    _compare(f, want, max_corners=4096, quality_level=1e-6, min_distance=0.0)
    f.close()
    img = cc.noise_image()
    f = _twin(img)
    for md, mc in ((7.0, 4096), (3.0, 300), (0.0, 4096)):
        want = co.good_features(img, mc, 0.01, md)
        assert want["n_candidates"] == 23888 and want["n_candidates"] > 4 * cc.DEVICE_TILE
        _compare(f, want, max_corners=mc, min_distance=md)
    f.close()


@pytest.mark.parametrize("name", list(cc.EDGE))
def test_edge_case_equals_the_checker(name):
    """Images narrower and lower than the device's 32 x 8 response tile, exactly one tile, one pixel past it and the smallest a flow
    object accepts; every candidate wanted, one corner wanted, and thresholds no response passes.  The checker gives 4 / 5 / 6
    corners at 31 x 7 / 32 x 8 / 33 x 9 (none at 5 x 5, whose interior is 3 x 3), 384 at 200 x 100 and 1 of 64 candidates at 64 x 48."""
    w, h, kw = cc.EDGE[name]
    want = cc.edge_checked(name)
    print(f"{name}: the checker has {want['n_candidates']} candidates and returns {len(want['xy'])}")
    if name in cc.SMALL_TILE_CASES:
        assert len(want["xy"]) >= 4
    if name.startswith("every_candidate"):
        assert len(want["xy"]) == want["n_candidates"] == 384
    if name.startswith("one_corner"):
        assert len(want["xy"]) == 1 and want["n_candidates"] > 1 and not want["exhausted"]
    if name.startswith("quality"):
        assert want["n_candidates"] == 0 and len(want["xy"]) == 0 and want["max_val"] > 0
    f = _twin(cc.edge_image(w, h), **cc.EDGE_FLOW_PARAMS)
    _compare(f, want, **kw)
    f.close()


def test_mask_scenario():
    """116 discs of which 109 are drawn, 19 % of the image left free, 2 202 candidates; 66 new corners at max_corners 204 (list
    exhausted), 20 at 20."""
    w, h = 752, 480
    img = fc.base_image(w, h)
    discs = cc.mask_scenario(w, h)
    f = _twin(img)
    for mc, n in ((204, 66), (20, 20)):
        want = co.good_features(img, mc, 0.01, 40.0, discs)
        assert len(discs) == 116 and int(want["disc_drawn"].sum()) == 109
        assert want["disc_drawn"][90:96].sum() < 6               # drifted points inside an earlier disc
        assert abs((want["mask"] != 0).mean() - 0.19) < 0.005
        assert want["n_candidates"] == 2202 and len(want["xy"]) == n
        got = _compare(f, want, discs=discs, max_corners=mc, min_distance=40.0)
        assert (want["mask"][got[:, 1].astype(int), got[:, 0].astype(int)] == 255).all()
    f.close()


def test_corners_fed_back_as_discs():
    """Of 150 corners extracted at min_distance 40 and fed back as discs of radius 40, 148 are drawn: the filled circle reaches a
    little further than the Euclidean distance test along the axes."""
    w, h = 752, 480
    img = fc.base_image(w, h)
    first = cc.checked(w, h, 150, 40.0)["xy"]
    discs = [(float(x), float(y), 40) for x, y in first]
    want = co.good_features(img, 150, 0.01, 40.0, discs)
    assert len(first) == 150 and int(want["disc_drawn"].sum()) == 148
    f = _twin(img)
    _compare(f, want, discs=discs, max_corners=150, min_distance=40.0)
    f.close()


@pytest.mark.parametrize("name", sorted(cc.special_discs()))
def test_special_discs(name):
    w, h = 752, 480
    img = fc.base_image(w, h)
    discs, drawn = cc.special_discs(w, h)[name]
    want = co.good_features(img, 300, 0.01, 40.0, discs)
    assert want["disc_drawn"].tolist() == drawn
    f = _twin(img)
    _compare(f, want, discs=discs, max_corners=300, min_distance=40.0)
    f.close()


def test_degenerate_images_and_masks():
    flat = cc.flat_image()
    want = co.good_features(flat, 300, 0.01, 40.0)
    assert len(want["xy"]) == 0 and want["n_candidates"] == 0 and want["max_val"] == 0
    f = _twin(flat)
    _compare(f, want, max_corners=300, min_distance=40.0)
    f.close()
    img = fc.base_image(320, 240)
    discs = cc.full_cover_discs(320, 240)
    want = co.good_features(img, 300, 0.01, 40.0, discs)
    assert (want["mask"] == 0).all() and len(want["xy"]) == 0 and want["max_val"] == 0 and want["max_val"].tobytes() == np.float32(0).tobytes()
    f = _twin(img)
    _compare(f, want, discs=discs, max_corners=300, min_distance=40.0)
    f.close()


def test_argument_checks():
    img = fc.base_image(320, 240)
    f = flow.Flow(flow.default_params(), 320, 240)
    assert corners.corners_status(f)[0] == abi.ERR_NOT_LOADED
    with pytest.raises(backend.BackendError):
        corners.download(f)
    f.push_frame(img, img)
    assert corners.corners_status(f, slot=corners.SLOT_PREVIOUS)[0] == abi.ERR_NOT_LOADED
    bad, unsupported = abi.ERR_BAD_ARGUMENT, abi.ERR_UNSUPPORTED
    assert corners.corners_status(f, max_corners=0)[0] == bad
    assert corners.corners_status(f, max_corners=4097, capacity=5000)[0] == unsupported
    assert corners.corners_status(f, max_corners=300, capacity=299)[0] == bad
    for q in (0.0, -0.5, float("nan"), float("inf")):
        assert corners.corners_status(f, quality_level=q)[0] == bad
    for md in (-1.0, float("nan"), float("inf")):
        assert corners.corners_status(f, min_distance=md)[0] == bad
    assert corners.corners_status(f, slot=2)[0] == bad and corners.corners_status(f, image=2)[0] == bad
    assert corners.corners_status(f, discs=[(float("nan"), 3.0, 5)])[0] == bad
    assert corners.corners_status(f, discs=[(3.0, float("inf"), 5)])[0] == bad
    assert corners.corners_status(f, discs=[(3.0, 3.0, -1)])[0] == bad
    assert corners.corners_status(f, discs=[(3.0, 3.0, corners.MAX_RADIUS + 1)])[0] == unsupported
    rc, xy = corners.corners_status(f, max_corners=4096, capacity=4096, min_distance=3.0)
    assert rc == abi.OK and len(xy) > 0
    f.push_frame(img, img)
    assert corners.corners_status(f, slot=corners.SLOT_PREVIOUS, image=corners.IMAGE_RIGHT)[0] == abi.OK
    f.close()


def test_previous_slot_and_right_image():
    a, b = fc.base_image(320, 240), fc.moved_pair(320, 240)[0]
    c = fc.moved_pair(320, 240)[1]
    f = flow.Flow(flow.default_params(), 320, 240)
    f.push_frame(a, c)
    f.push_frame(b, a)
    for slot, image, img in ((corners.SLOT_PREVIOUS, 0, a), (corners.SLOT_PREVIOUS, 1, c), (corners.SLOT_CURRENT, 0, b), (corners.SLOT_CURRENT, 1, a)):
        want = co.good_features(img, 300, 0.01, 20.0)
        got = corners.corners(f, slot=slot, image=image, min_distance=20.0)
        assert got.tobytes() == want["xy"].tobytes() and len(got) > 50
    f.close()


def test_ground_truth_squares():
    """160 corners for 160 true ones; every returned corner within 1 px of a true corner and every true corner found within 1 px
    (the checker alone: 0.707 px both ways, the closest an integer pixel can be to a corner between pixels)."""
    img, truth = cc.squares_image()
    assert len(truth) == 160
    f = _twin(img)
    got = corners.corners(f, max_corners=300, min_distance=10.0).astype(np.float64)
    d = np.sqrt(((got[:, None, :] - truth[None]) ** 2).sum(-1))
    print(f"squares: {len(got)} corners for {len(truth)}; corner -> truth max {d.min(1).max():.3f} px, truth -> corner max {d.min(0).max():.3f} px")
    assert d.min(1).max() <= 1.0 and d.min(0).max() <= 1.0
    want = co.good_features(img, 300, 0.01, 10.0)
    assert len(want["xy"]) == 160
    _compare(f, want, max_corners=300, min_distance=10.0)
    f.close()


def test_download_sizes_disc_drawn_from_the_last_call():
    """The hook copies as many draw decisions as the last call had discs: the binding asks the library for that count, so a caller
    that does not know it (or states another) cannot be handed a short buffer."""
    w, h = 752, 480
    f = _twin(fc.base_image(w, h))
    discs = cc.mask_scenario(w, h)
    corners.corners(f, discs=discs, max_corners=204)
    st = corners.download(f)
    assert len(st["disc_drawn"]) == len(discs) == 116 and int(st["disc_drawn"].sum()) == 109
    with pytest.raises(ValueError):
        corners.download(f, 0)
    corners.corners(f, max_corners=20)
    assert len(corners.download(f)["disc_drawn"]) == 0 and len(corners.download(f, 0)["disc_drawn"]) == 0
    f.close()
