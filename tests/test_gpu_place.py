"""Visual place recognition on the GPU (include/visfs_place.h): the device path against the host twin byte for byte on every input of
place_cases.py (descriptors, valid flags, bins, store contents, every byte of the result block), what a call issues, and the
objects beside the others of one handle.  tests/test_place_host.py holds the twin to the NumPy checker on the same inputs."""
import numpy as np
import pytest

import place_cases as pc
from visfs_amd import abi, backend, corners, flow, place, synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _pair(solver, w, h, frames):
    dev, host = flow.Flow(flow.default_params(**pc.FLOW), w, h, solver=solver), flow.Flow(flow.default_params(**pc.FLOW), w, h)
    for left, right in frames:
        dev.push_frame(left, right)
        host.push_frame(left, right)
    return dev, host


def _same_sets(a, b):
    got, want = a.download(), b.download()
    for key in ("xy", "desc", "valid", "bin"):
        assert got[key].tobytes() == want[key].tobytes(), key
    return got


def _same_slot(da, db, k):
    got, want = da.download(k), db.download(k)
    assert got["key"] == want["key"]
    for key in ("desc", "valid", "ids", "xyz"):
        assert got[key].tobytes() == want[key].tobytes(), key


def _same_query(ddb, dset, hdb, hset, **params):
    rc, r = ddb.query_raw(dset, **params)
    assert rc == abi.OK, ddb.last_error()
    assert ddb.last_counts() == (1, place.QUERY_LAUNCHES, 1, 1) == (1, 2, 1, 1)
    rc, want = hdb.query_raw(hset, **params)
    assert rc == abi.OK
    assert bytes(memoryview(r)) == bytes(memoryview(want)), params
    return place.unpack(r)


@pytest.mark.parametrize("size", pc.DESCRIBE_SIZES)
def test_describe_equals_the_host_twin(solver, size):
    w, h = size
    img = pc.describe_image(w, h)
    dev, host = _pair(solver, w, h, [(img, img)])
    a, b = place.DescriptorSet(dev, 512), place.DescriptorSet(host, 512)
    for n in pc.DESCRIBE_COUNTS:
        xy = pc.describe_points(w, h, n)
        a.describe(xy); b.describe(xy)
        assert a.last_counts() == (1, 1, 0, 0)
        got = _same_sets(a, b)
        want = pc.describe_checked(w, h, n)
        assert got["desc"].tobytes() == want["desc"].tobytes() and got["bin"].tobytes() == want["bin"].tobytes()
    for n in (65, 3):                                   # a shorter call after a longer one, back to back with no wait between
        a.describe(pc.describe_points(w, h, n)); b.describe(pc.describe_points(w, h, n))
    _same_sets(a, b)
    a.close(); b.close(); dev.close(); host.close()


def test_describe_from_every_slot_and_image(solver):
    w, h = 160, 120
    base = pc.describe_image(w, h)
    imgs = [base, np.ascontiguousarray(base[::-1]), np.ascontiguousarray(base[:, ::-1]), np.ascontiguousarray(base[::-1, ::-1])]
    dev, host = _pair(solver, w, h, [(imgs[0], imgs[1]), (imgs[2], imgs[3])])
    xy = pc.describe_points(w, h, 65)
    a, b = place.DescriptorSet(dev, 65), place.DescriptorSet(host, 65)
    seen = set()
    for slot in (place.SLOT_PREVIOUS, place.SLOT_CURRENT):
        for image in (place.IMAGE_LEFT, place.IMAGE_RIGHT):
            a.describe(xy, slot, image); b.describe(xy, slot, image)
            seen.add(_same_sets(a, b)["desc"].tobytes())
    assert len(seen) == 4
    a.close(); b.close(); dev.close(); host.close()


@pytest.mark.parametrize("name", list(pc.QUERY_CASES))
def test_query_equals_the_host_twin(solver, name):
    case = pc.query_case(name)
    dev, host = _pair(solver, 160, 120, [])
    a, b = place.DescriptorSet(dev, 512), place.DescriptorSet(host, 512)
    n = max(len(case["slots"]), 1)
    da, db = place.KeyFrameStore(solver, n), place.KeyFrameStore(None, n)
    for k, sl in enumerate(case["slots"]):
        for s, store in ((a, da), (b, db)):
            s.upload(np.zeros((len(sl["desc"]), 2), np.float32), sl["desc"], sl["valid"])
            assert store.add(s, sl["ids"], sl["xyz"], sl["key"]) == k
    for k in sorted({0, len(case["slots"]) // 2, len(case["slots"]) - 1}):
        _same_slot(da, db, k)
    q = case["qset"]
    a.upload(q["xy"], q["desc"], q["valid"]); b.upload(q["xy"], q["desc"], q["valid"])
    for v, want in zip(case["variants"], pc.query_checked(name)):
        got = _same_query(da, a, db, b, **v)
        assert got["raw"] == want, v
    da.close(); db.close(); a.close(); b.close(); dev.close(); host.close()


def test_a_revisited_scene_on_the_device(solver):
    """Describe, add and query end to end on resident images: eight scenes, two revisits (tests/test_place_host.py states the counts)."""
    pts = pc.scene_points()
    dev, host = _pair(solver, pc.SCENE_W, pc.SCENE_H, [])
    a, b = place.DescriptorSet(dev, 200), place.DescriptorSet(host, 200)
    da, db = place.KeyFrameStore(solver, 8), place.KeyFrameStore(None, 8)
    ids = (1000 + np.arange(200)).astype(np.int32)
    xyz = np.random.default_rng(3).normal(0, 2, (200, 3)).astype(np.float32)
    for k, seed in enumerate(pc.PLACE_SEEDS):
        for f, s, store in ((dev, a, da), (host, b, db)):
            f.push_frame(pc.scene(seed), pc.scene(seed))
            s.describe(pts)
            assert store.add(s, ids, xyz, seed) == k
        _same_slot(da, db, k)
    for revisited, view in pc.PLACE_QUERIES:
        img, moved = pc.moved_scene(pc.PLACE_SEEDS[revisited], view["t"], view["rot"], view["zoom"])
        for f, s in ((dev, a), (host, b)):
            f.push_frame(img, img)
            s.describe(moved)
        _same_sets(a, b)
        got = _same_query(da, a, db, b)
        assert [c["slot"] for c in got["candidates"]] == [revisited]
        assert got["candidates"][0]["count"] >= 3 * max(np.delete(got["count"], revisited).max(), 1)
    da.close(); db.close(); a.close(); b.close(); dev.close(); host.close()


def test_flavours_do_not_mix(solver):
    img = pc.describe_image(160, 120)
    dev, host = _pair(solver, 160, 120, [(img, img)])
    a, b = place.DescriptorSet(dev, 8), place.DescriptorSet(host, 8)
    da, db = place.KeyFrameStore(solver, 2), place.KeyFrameStore(None, 2)
    xy = pc.describe_points(160, 120, 8)
    a.describe(xy); b.describe(xy)
    ids, xyz = np.arange(8, dtype=np.int32), np.zeros((8, 3), np.float32)
    assert da.add_status(b, ids, xyz)[0] == abi.ERR_BAD_ARGUMENT and "flavours" in da.last_error()
    assert db.add_status(a, ids, xyz)[0] == abi.ERR_BAD_ARGUMENT
    assert da.add(a, ids, xyz) == 0 and db.add(b, ids, xyz) == 0
    assert da.query_raw(b)[0] == abi.ERR_BAD_ARGUMENT and db.query_raw(a)[0] == abi.ERR_BAD_ARGUMENT
    other = backend.Solver(abi.default_params(iterations=10, solver=2))
    dc = place.KeyFrameStore(other, 2)
    assert dc.add_status(a, ids, xyz)[0] == abi.ERR_BAD_ARGUMENT and "handles" in dc.last_error()
    dc.close(); other.close()
    da.close(); db.close(); a.close(); b.close(); dev.close(); host.close()


def test_beside_the_other_objects_of_a_handle(solver):
    """Two sets and two stores on one handle, a describe behind visfs_flow_corners on the same frame (the corners are what they were
    without it), and a bundle adjustment between two queries (both give the same block)."""
    w, h = pc.SCENE_W, pc.SCENE_H
    img0, img1 = pc.scene(20), pc.scene(21)
    dev, host = _pair(solver, w, h, [(img0, img1)])
    kw = dict(max_corners=200, min_distance=10.0)
    alone = corners.corners(dev, **kw)
    sets = [(place.DescriptorSet(dev, 256), place.DescriptorSet(host, 256)) for _ in range(2)]
    stores = [(place.KeyFrameStore(solver, 4), place.KeyFrameStore(None, 4)) for _ in range(2)]
    xy = corners.corners(dev, **kw)
    assert xy.tobytes() == alone.tobytes() == corners.corners(host, **kw).tobytes() and len(xy) > 100
    ids, xyz = np.arange(len(xy), dtype=np.int32), np.ones((len(xy), 3), np.float32)
    for image, ((a, b), (da, db)) in enumerate(zip(sets, stores)):
        a.describe(xy, place.SLOT_CURRENT, image); b.describe(xy, place.SLOT_CURRENT, image)
        assert da.add(a, ids, xyz, image) == 0 and db.add(b, ids, xyz, image) == 0
    assert corners.corners(dev, **kw).tobytes() == alone.tobytes()
    for (a, b), (da, db) in zip(sets, stores):
        _same_sets(a, b)
        _same_slot(da, db, 0)
    (a0, b0), (a1, b1) = sets
    (da0, db0), (da1, db1) = stores
    assert _same_sets(a0, b0)["desc"].tobytes() != _same_sets(a1, b1)["desc"].tobytes()
    first = _same_query(da0, a0, db0, b0, min_matches=1)            # a frame against itself: every valid corner, at distance 0
    assert first["candidates"][0]["count"] == int(a0.download()["valid"].sum()) and (first["candidates"][0]["rows"]["distance"] == 0).all()
    rc, rb = solver.solve_window(abi.WindowBuffers(synth.make_window("C1")))
    assert rc == abi.OK
    assert _same_query(da0, a0, db0, b0, min_matches=1)["raw"] == first["raw"]
    crossed = _same_query(da1, a0, db1, b0, min_matches=0)          # the left image's set against the store of the right image's
    assert crossed["n_slots"] == 1 and crossed["count"][0] < first["candidates"][0]["count"]
    for pair in sets + stores:
        for o in pair:
            o.close()
    dev.close(); host.close()
