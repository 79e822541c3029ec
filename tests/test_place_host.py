"""Visual place recognition (include/visfs_place.h) on the host twin: against the NumPy checker of place_oracle.py byte for byte
(pattern, descriptors, valid flags, bins, store contents, every byte of the result block), the refusals, and what the descriptor is
for: the same point found again in a turned, zoomed and shifted view, and a revisited scene told from seven others.  The figures in
the docstrings are what the checker gives."""
import ctypes as C

import numpy as np
import pytest

import place_cases as pc
import place_oracle as po
from visfs_amd import abi, backend, flow, place


def _twin(img):
    h, w = img.shape
    f = flow.Flow(flow.default_params(**pc.FLOW), w, h)
    f.push_frame(img, img)
    return f


def _same_set(got, want, xy):
    assert got["xy"].tobytes() == np.asarray(xy, dtype=np.float32).tobytes()
    for key in ("desc", "valid", "bin"):
        assert got[key].tobytes() == want[key].tobytes(), key


def test_exports_and_defaults():
    lib = place.load()
    assert lib.visfs_place_abi_version() == place.ABI_VERSION == 1
    for name in place.EXPORTS:
        assert hasattr(lib, name)
    p = place.default_params()
    assert (p.first_slot, p.last_slot, p.max_distance, p.ratio_num, p.ratio_den, p.min_matches, p.cross_check) == (0, 1024, 64, 4, 5, 40, 1)
    assert C.sizeof(place.Result) == po.RESULT_DTYPE.itemsize and C.sizeof(place.Row) == po.ROW_DTYPE.itemsize == 36
    assert {k: getattr(p, k) for k in po.DEFAULTS} == po.DEFAULTS


def test_pattern_equals_the_checker_and_keeps_its_promises():
    """No test compares a point with itself, in any bin, and no rotated coordinate leaves [-13, 13]: with the 5 x 5 box that is
    the reach of 15 pixels the validity margin allows."""
    want = po.pattern()
    assert place.pattern().tobytes() == want.tobytes()
    assert np.abs(want.astype(int)).max() == 13
    assert not np.any(np.all(want[:, 0::2] == want[:, 1::2], axis=-1))
    base = np.array(po.base_points())
    assert want[0].tolist() == base.tolist() and len({tuple(p) for p in base.tolist()}) > 300
    # the literals are what they say they are
    k = np.arange(32)
    assert po.COS == np.rint(16384 * np.cos(2 * np.pi * k / 32)).astype(int).tolist()
    assert po.SIN == np.rint(16384 * np.sin(2 * np.pi * k / 32)).astype(int).tolist()


@pytest.mark.parametrize("size", pc.DESCRIBE_SIZES)
def test_describe_equals_the_checker(size):
    w, h = size
    f = _twin(pc.describe_image(w, h))
    s = place.DescriptorSet(f, 512)
    for n in pc.DESCRIBE_COUNTS:
        xy = pc.describe_points(w, h, n)
        s.describe(xy)
        assert s.last_counts() == (0, 0, 0, 0)
        _same_set(s.download(), pc.describe_checked(w, h, n), xy)
    s.close(); f.close()


@pytest.mark.parametrize("size", pc.DESCRIBE_SIZES)
def test_describe_inputs_take_their_branches(size):
    """On the checker alone: valid and invalid one pixel apart, the half-even rule, the constant patch (bin 0, no bit set, valid) and
    the point-symmetric patch (both moments 0, so every bin scores 0 and bin 0 wins the tie, yet bits are set)."""
    w, h = size
    img, xy = pc.describe_image(w, h), pc.special_points(w, h)
    got = po.describe(img, xy)
    valid = {tuple(p): int(v) for p, v in zip(xy.tolist(), got["valid"])}
    my, mx = h // 2, w // 2
    assert [valid[(x, my)] for x in (14, 15, w - 16, w - 15)] == [0, 1, 1, 0]
    assert [valid[(mx, y)] for y in (14, 15, h - 16, h - 15)] == [0, 1, 1, 0]
    assert valid[(15, 15)] == valid[(w - 16, h - 16)] == 1 and valid[(14, 15)] == valid[(w - 16, h - 15)] == 0
    assert valid[(14.5, my)] == 0 and valid[(15.5, my)] == 1                   # 14.5 -> 14, 15.5 -> 16
    assert valid[(w - 15.5, my)] == (1 if w % 2 == 0 else 0)                   # 144.5 -> 144 = w - 16, 145.5 -> 146 = w - 15
    assert valid[(mx, h - 15.5)] == (1 if h % 2 == 0 else 0)
    assert got["valid"][np.any(~np.isfinite(xy), axis=1)].sum() == 0 and (~np.isfinite(xy)).any(axis=1).sum() == 5
    assert got["desc"][got["valid"] == 0].sum() == 0 and got["bin"][got["valid"] == 0].sum() == 0
    assert got["valid"][0] == 1 and got["bin"][0] == 0 and got["desc"][0].sum() == 0               # constant
    assert po.moments(img, *pc.SYMMETRIC_AT) == (0, 0)
    assert got["valid"][1] == 1 and got["bin"][1] == 0 and got["desc"][1].sum() > 0                # symmetric
    assert len(set(got["bin"][got["valid"] == 1].tolist())) > 8
    # (mx + 0.5, my + 0.5) and (mx + 1.5, my + 1.5) round to one centre or to two, depending on the parity of mx
    a, b = po.centre(mx + 0.5, my + 0.5, w, h), po.centre(mx + 1.5, my + 1.5, w, h)
    assert (a[0] % 2, b[0] % 2) == (0, 0)


def test_describe_from_every_slot_and_image():
    w, h = 160, 120
    imgs = [pc.describe_image(w, h), np.ascontiguousarray(pc.describe_image(w, h)[::-1]), np.ascontiguousarray(pc.describe_image(w, h)[:, ::-1]),
            np.ascontiguousarray(pc.describe_image(w, h)[::-1, ::-1])]
    f = flow.Flow(flow.default_params(**pc.FLOW), w, h)
    f.push_frame(imgs[0], imgs[1])
    f.push_frame(imgs[2], imgs[3])
    xy = pc.describe_points(w, h, 65)
    s = place.DescriptorSet(f, 65)
    seen = set()
    for slot, image, img in ((place.SLOT_PREVIOUS, 0, imgs[0]), (place.SLOT_PREVIOUS, 1, imgs[1]), (place.SLOT_CURRENT, 0, imgs[2]),
                             (place.SLOT_CURRENT, 1, imgs[3])):
        s.describe(xy, slot, image)
        got = s.download()
        _same_set(got, po.describe(img, xy), xy)
        seen.add(got["desc"].tobytes())
    assert len(seen) == 4
    s.close(); f.close()


def test_refusals():
    img = pc.describe_image(160, 120)
    f = flow.Flow(flow.default_params(**pc.FLOW), 160, 120)
    lib = place.load()
    h = C.c_void_p()
    assert lib.visfs_place_set_create(f.h, 0, C.byref(h)) == abi.ERR_BAD_ARGUMENT
    assert lib.visfs_place_set_create(f.h, 513, C.byref(h)) == abi.ERR_UNSUPPORTED
    assert lib.visfs_place_db_create(None, 0, C.byref(h)) == abi.ERR_BAD_ARGUMENT
    assert lib.visfs_place_db_create(None, 1025, C.byref(h)) == abi.ERR_UNSUPPORTED
    s = place.DescriptorSet(f, 8)
    xy = pc.describe_points(160, 120, 9)
    assert s.describe_status(xy[:4]) == abi.ERR_NOT_LOADED and "no frame" in s.last_error()
    with pytest.raises(backend.BackendError):
        s.download()
    db = place.KeyFrameStore(None, 2)
    assert db.add_status(s, np.zeros(4, np.int32), np.zeros((4, 3), np.float32))[0] == abi.ERR_NOT_LOADED
    assert db.query_raw(s)[0] == abi.ERR_NOT_LOADED
    f.push_frame(img, img)
    assert s.describe_status(xy[:4], place.SLOT_PREVIOUS) == abi.ERR_NOT_LOADED
    assert s.describe_status(xy) == abi.ERR_BAD_ARGUMENT and "capacity" in s.last_error()
    assert s.describe_status(xy[:4], 2, 0) == abi.ERR_BAD_ARGUMENT and s.describe_status(xy[:4], 1, 2) == abi.ERR_BAD_ARGUMENT
    s.describe(xy[:4])
    ids, xyz = np.arange(4, dtype=np.int32), np.ones((4, 3), np.float32)
    assert db.add(s, ids, xyz, 5) == 0 and db.add(s, ids, xyz, 6) == 1 and db.size() == 2
    assert db.add_status(s, ids, xyz)[0] == abi.ERR_UNSUPPORTED and "full" in db.last_error()
    for bad in (dict(first_slot=-1), dict(first_slot=2, last_slot=1), dict(max_distance=-1), dict(max_distance=257), dict(ratio_num=0),
                dict(ratio_den=0), dict(ratio_den=1025), dict(min_matches=-1), dict(min_matches=513)):
        assert db.query_raw(s, **bad)[0] == abi.ERR_BAD_ARGUMENT, bad
    with pytest.raises(backend.BackendError):
        db.download(2)
    db.reset()
    assert db.size() == 0 and db.query(s, min_matches=0)["n_slots"] == 0
    assert db.add(s, ids, xyz, 7) == 0 and db.download(0)["key"] == 7
    small = flow.Flow(flow.default_params(max_level=0, win_size=3), 30, 40)
    small.push_frame(np.zeros((40, 30), np.uint8), np.zeros((40, 30), np.uint8))
    t = place.DescriptorSet(small, 4)
    assert t.describe_status(xy[:1]) == abi.ERR_BAD_ARGUMENT and "31 x 31" in t.last_error()
    t.close(); small.close(); db.close(); s.close(); f.close()


def _load(case, f):
    """The case's query set and store on host twins."""
    q = case["qset"]
    s = place.DescriptorSet(f, 512)
    db = place.KeyFrameStore(None, max(len(case["slots"]), 1))
    for k, sl in enumerate(case["slots"]):
        s.upload(np.zeros((len(sl["desc"]), 2), np.float32), sl["desc"], sl["valid"])
        assert db.add(s, sl["ids"], sl["xyz"], sl["key"]) == k
    s.upload(q["xy"], q["desc"], q["valid"])
    return s, db


@pytest.mark.parametrize("name", list(pc.QUERY_CASES))
def test_query_equals_the_checker(name):
    case = pc.query_case(name)
    f = flow.Flow(flow.default_params(**pc.FLOW), 160, 120)
    s, db = _load(case, f)
    for k in sorted({0, len(case["slots"]) // 2, len(case["slots"]) - 1}):
        got, sl = db.download(k), case["slots"][k]
        assert got["key"] == sl["key"]
        for key in ("desc", "valid", "ids", "xyz"):
            assert got[key].tobytes() == np.ascontiguousarray(sl[key]).tobytes(), key
    for v, want in zip(case["variants"], pc.query_checked(name)):
        rc, r = db.query_raw(s, **v)
        assert rc == abi.OK and db.last_counts() == (0, 0, 0, 0)
        assert bytes(memoryview(r)) == want, v
    db.close(); s.close(); f.close()


def _result(name, variant):
    return np.frombuffer(pc.query_checked(name)[variant], dtype=po.RESULT_DTYPE)[0]


def test_query_inputs_take_their_branches():
    """On the checker alone, what each made-to-order case is there for."""
    for n in (63, 64, 65, 1024):                                   # more than eight equal counts: ordered by slot, behind the two better
        r = _result(f"slots_{n}", 0)
        assert r["n_slots"] == n and r["n_candidates"] == 8
        assert r["candidate"]["count"].tolist() == [10, 7] + [6] * 6
        assert r["candidate"]["slot"].tolist() == [n - 1, n // 2] + [s for s in range(0, n, 5) if s not in (n - 1, n // 2)][:6]
        assert r["candidate"]["key"].tolist() == [(1 << 40) + 7 * s for s in r["candidate"]["slot"].tolist()]
        assert (np.diff(r["row"][0]["query_index"][:10]) > 0).all()
        left_out = _result(f"slots_{n}", 4)                        # the range leaves out the best slot
        assert left_out["first_slot"] == 1 and left_out["n_slots"] == n - 2 and left_out["candidate"]["slot"][0] == n // 2
        one = _result(f"slots_{n}", 5)
        assert one["n_slots"] == 1 and one["candidate"]["slot"][0] == n // 2 and one["n_candidates"] == 1
        assert _result(f"slots_{n}", 6)["n_slots"] == 0 and _result(f"slots_{n}", 2)["n_candidates"] == 2
    assert _result("slots_1", 0)["candidate"]["count"][0] == 10 and _result("slots_2", 0)["candidate"]["slot"].tolist()[:2] == [1, 0]
    r = _result("entries_0_1_512", 0)                              # 0, 1 and 512 entries; one entry: d2 = 257
    assert r["count"][:3].tolist() == [0, 1, 482] and r["row"][1][0]["query_index"] == 5 and r["row"][1][0]["distance"] == 3
    assert r["candidate"]["slot"].tolist()[:2] == [2, 1]
    assert _result("entries_0_1_512", 1)["count"][:3].tolist() == [0, 1, 482]      # the other queries lie further than max_distance from the lone entry
    assert _result("entries_0_1_512", 2)["count"][2] == 0 and _result("entries_0_1_512", 3)["count"][2] == 482      # distance 10 exactly
    r = _result("no_valid_query", 0)
    assert r["count"][:2].tolist() == [0, 0] and r["n_candidates"] == 2 and _result("no_valid_query", 1)["n_candidates"] == 0
    assert _result("empty_set", 0)["n_candidates"] == 1
    for v in range(2):                                             # duplicates: d1 = d2 fails any ratio up to 1; the plain slot matches
        assert _result("duplicates", v)["count"][:3].tolist() == [0, 0, 16]
    assert _result("duplicates", 2)["count"][:3].tolist() == [16, 0, 16]          # 4 < 4 * 1024 passes, 0 < 0 never does
    assert _result("duplicates", 2)["row"][1]["db_index"][:16].tolist() == list(range(16))     # the lower of two equal entries
    r = _result("equal_queries", 0)
    assert r["count"][0] == 2 and r["row"][0]["query_index"][:2].tolist() == [2, 4]
    r = _result("equal_queries", 1)
    assert r["count"][0] == 3 and r["row"][0]["query_index"][:3].tolist() == [2, 4, 9] and r["row"][0]["db_index"][:3].tolist() == [0, 3, 0]
    assert [_result("distance_bounds", v)["count"][0] for v in range(4)] == [8, 12, 12, 24]


# ------------------------------------------------------------------------------------------------ what the descriptor is for
def _truth_stats(a, b):
    """Entry i of b is the same scene point as query i of a.  (share of valid pairs whose nearest entry is the true one, accepted,
    wrongly accepted, valid pairs)"""
    both = (a["valid"] == 1) & (b["valid"] == 1)
    D = po.distances(a["desc"], b["desc"]) * 1024 + np.arange(len(b["desc"]))[None, :]
    D[:, b["valid"] == 0] = 1 << 40
    nearest = (D.argmin(1) == np.arange(len(D)))[both].mean()
    m = po.match_slot(a["desc"], a["valid"], b["desc"], b["valid"], po.DEFAULTS)
    return nearest, len(m), sum(1 for i, j, _ in m if i != j), int(both.sum())


def test_descriptor_finds_the_point_again_in_a_moved_view():
    """Texture 11, 200 points, the views of pc.VIEWS (rot 0, 0.1, 0.5, 1.3, 3.0 rad).  The checker gives nearest-correct shares of
    1.000, 0.945, 0.922, 0.962 and 0.950, accepted 200 of 200, 181 of 200, 161 of 192, 168 of 185 and 175 of 200 valid pairs, and no
    wrongly accepted match at any angle; required: a share of at least 0.85 at every angle and wrongly
    accepted matches of at most 5 % of the accepted.  The twin's descriptors are the checker's."""
    base = po.describe(pc.scene(11), pc.scene_points())
    assert base["valid"].all()
    for view in pc.VIEWS:
        img, pts = pc.moved_scene(11, view["t"], view["rot"], view["zoom"])
        moved = po.describe(img, pts)
        nearest, accepted, wrong, pairs = _truth_stats(moved, base)
        print(f"rot {view['rot']}: nearest-correct {nearest:.3f}, accepted {accepted} of {pairs}, wrongly accepted {wrong}")
        assert pairs >= 150
        assert nearest >= 0.85
        assert wrong <= 0.05 * accepted
    f = _twin(np.ascontiguousarray(img))
    s = place.DescriptorSet(f, 200)
    s.describe(pts)
    _same_set(s.download(), moved, pts)
    s.close(); f.close()


def test_a_revisited_scene_is_told_from_seven_others():
    """Eight slots from textures 20 to 27 at the same 200 points; the queries are slot 3's scene turned by 0.7 rad and slot 6's by
    2.5 rad (zoom 1.03, shift (6, -4)).  Required: the revisited slot first with at least three times the runner-up's count, and with
    the default min_matches the only candidate.  The checker counts 172 against at most 20 elsewhere, and 160 against at most 19;
    the default min_matches of 40 lies between them."""
    pts = pc.scene_points()
    f = flow.Flow(flow.default_params(**pc.FLOW), pc.SCENE_W, pc.SCENE_H)
    s = place.DescriptorSet(f, 200)
    db = place.KeyFrameStore(None, 8)
    slots = []
    for k, seed in enumerate(pc.PLACE_SEEDS):
        f.push_frame(pc.scene(seed), pc.scene(seed))
        s.describe(pts)
        sl = pc.as_slot(s.download(), key=seed)
        assert db.add(s, sl["ids"], sl["xyz"], seed) == k
        slots.append(sl)
    for revisited, view in pc.PLACE_QUERIES:
        img, moved = pc.moved_scene(pc.PLACE_SEEDS[revisited], view["t"], view["rot"], view["zoom"])
        f.push_frame(img, img)
        s.describe(moved)
        q = s.download()
        rc, r = db.query_raw(s)
        assert rc == abi.OK
        assert bytes(memoryview(r)) == po.query(dict(xy=moved, desc=q["desc"], valid=q["valid"]), slots).tobytes()
        got = place.unpack(r)
        counts = got["count"].tolist()
        others = sorted(c for k, c in enumerate(counts) if k != revisited)
        print(f"slot {revisited} at rot {view['rot']}: {counts[revisited]} against at most {others[-1]}")
        assert counts[revisited] >= 3 * max(others[-1], 1)
        assert [c["slot"] for c in got["candidates"]] == [revisited] and got["candidates"][0]["key"] == pc.PLACE_SEEDS[revisited]
        rows = got["candidates"][0]["rows"]
        assert (rows["id"] == 1000 + rows["db_index"]).all() and (rows["to_xy"] == moved[rows["query_index"]]).all()
        assert (rows["query_index"] == rows["db_index"]).mean() >= 0.95          # the rows pair a point with itself
        assert place.default_params().min_matches > others[-1] and place.default_params().min_matches < counts[revisited]
    db.close(); s.close(); f.close()


# ------------------------------------------------------------------------------------------------ the chain down to a pose
CHAIN_ROT_TOL, CHAIN_TRANS_TOL = 3 * 0.00125, 3 * 0.0063      # three times the largest difference over the seeds 1, 2, 3 (rad, m)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_rows_of_a_query_give_the_pose_of_the_true_correspondences(seed):
    """A stereo_pair wall at 5 m, 320 x 240: the twin's visfs_flow_stereo gives the 200 words their 3-D points, the key-frame is stored,
    and the scene comes back under Motion(t=(6, -4), rot=0.7, zoom=1).  visfs_pnp_solve on the rows of the top candidate is held to
    visfs_pnp_solve on the true correspondences of the same 200 points.  Measured over the three seeds: 178, 169 and 175 rows, pose
    differences of 1.24e-3, 1.1e-5 and 4.6e-6 rad and of 6.3e-3, 5.5e-5 and 2.4e-5 m (seed 1 carries one wrong match); the tolerance
    is three times the largest, as section 9t sets its arc tolerance."""
    import flow_oracle as fo
    from visfs_amd import pnp
    w, h = pc.SCENE_W, pc.SCENE_H
    left, right, _ = fo.stereo_pair("plane", width=w, height=h, seed=seed)
    pts = pc.scene_points()
    f = flow.Flow(flow.default_params(**pc.FLOW), w, h)
    f.push_frame(left, right)
    _, _, xyz = f.stereo(pts, flow.camera(cx=0.5 * (w - 1), cy=0.5 * (h - 1), cx_right=0.5 * (w - 1)))
    assert np.isfinite(xyz).all(axis=1).sum() >= 190
    s = place.DescriptorSet(f, 200)
    db = place.KeyFrameStore(None, 2)
    s.describe(pts)
    ids = np.arange(200, dtype=np.int32)
    assert db.add(s, ids, xyz, seed) == 0
    m = fo.Motion(w, h, (6.0, -4.0), 0.7, 1.0)
    X, Y = fo.grid(w, h)
    back = m.inverse(np.stack([X, Y], -1))
    img = fo.Texture(seed).image(back[..., 0], back[..., 1])
    moved = m.forward(pts).astype(np.float32)
    f.push_frame(img, img)
    s.describe(moved)
    got = db.query(s)
    q = s.download()
    want = po.query(dict(xy=moved, desc=q["desc"], valid=q["valid"]), [dict(desc=db.download(0)["desc"], valid=db.download(0)["valid"], ids=ids, xyz=xyz, key=seed)])
    assert got["raw"] == want.tobytes()
    assert [c["slot"] for c in got["candidates"]] == [0]
    rows = got["candidates"][0]["rows"]
    solver, cam = pnp.Pnp(512), pnp.camera(cx=0.5 * (w - 1), cy=0.5 * (h - 1))
    a = solver.solve(pnp.default_params(), cam, rows["from_xyz"], rows["to_xy"])
    b = solver.solve(pnp.default_params(), cam, xyz, moved)
    assert a["T"][3, 3] == b["T"][3, 3] == 1.0
    rot = float(np.arccos(np.clip(0.5 * (np.trace(a["T"][:3, :3].T @ b["T"][:3, :3]) - 1.0), -1.0, 1.0)))
    trans = float(np.linalg.norm(a["T"][:3, 3] - b["T"][:3, 3]))
    print(f"seed {seed}: {len(rows)} rows, {rot:.3g} rad, {trans:.3g} m")
    assert rot <= CHAIN_ROT_TOL and trans <= CHAIN_TRANS_TOL
    solver.close(); db.close(); s.close(); f.close()
