"""The verified place query (include/visfs_place_verify.h) on the host twin: against the staged calls byte for byte
(visfs_place_query, then visfs_pnp_solve per candidate), against the checker of place_verify_oracle.py (picks, kept rows and inlier
lists exactly, poses within POSE_BOUND), the refusals, the closure edge against a scene's true planar pose, and what the guided stage
is for on the chain scene of section 9w.  The figures in the docstrings are what the checker and the twin give."""
import ctypes as C

import numpy as np
import pytest

import flow_oracle as fo
import place_cases as pc
import place_oracle as po
import place_verify_cases as vc
import place_verify_oracle as pvo
from visfs_amd import abi, backend, flow, place, pnp, pose_graph
from visfs_amd import place_verify as pv

POSE_BOUND = 1.5e-11      # pose and covariance entries against the checker: what tests/pnp_cases.py measured between twin and checker


_load, _params = vc.load, vc.params


def _call(v, s, case, variant):
    rc, r, w = v.query_verify_raw(s, _params(variant), case["query_xyz"] if variant["xyz"] else None, **variant["place"])
    assert rc == abi.OK, v.last_error()
    return r, w


@pytest.fixture(scope="module")
def host_flow():
    f = flow.Flow(flow.default_params(**pc.FLOW), 160, 120)
    yield f
    f.close()


def test_exports_and_defaults():
    lib = pv.load()
    assert lib.visfs_place_verify_abi_version() == pv.ABI_VERSION == 1
    for name in pv.EXPORTS:
        assert hasattr(lib, name)
    p = pv.default_params()
    d = pnp.default_params()
    assert bytes(memoryview(p.pnp)) == bytes(memoryview(d))
    assert (p.guided, p.guided_radius, p.guided_max_distance) == (1, 6.0, 64) and p.guided_radius == 3 * d.reproj_error
    assert p.guided_max_distance == place.default_params().max_distance
    assert {k: getattr(p, k) for k in pvo.DEFAULTS} == pvo.DEFAULTS
    assert C.sizeof(pv.Stage1) == 8 + 2 * 2048 + 8 * 52 and C.sizeof(pv.Stage2) == 8 + 512 * 36 + 8 + 2048 + 8 * 52
    assert C.sizeof(pv.Result) == 8 + 8 * (C.sizeof(pv.Stage1) + C.sizeof(pv.Stage2))


def test_the_window_is_closed_and_evaluated_in_double():
    """A query exactly on the circle is inside (3-4-5), one float32 step of the radius below it is outside; radius 0 takes the query
    that coincides with the projection and no other; what is not finite is in no window.  The checker's window agrees on random pairs."""
    assert pv.in_window(100.0, 50.0, 103.0, 54.0, 5.0) and pvo.in_window(100.0, 50.0, 103.0, 54.0, 5.0)
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    assert not pv.in_window(100.0, 50.0, 103.0, 54.0, below) and not pvo.in_window(100.0, 50.0, 103.0, 54.0, below)
    assert pv.in_window(17.25, 9.5, 17.25, 9.5, 0.0) and not pv.in_window(17.25 + 1e-9, 9.5, 17.25, 9.5, 0.0)
    assert not pv.in_window(np.nan, 9.5, 17.25, 9.5, 6.0) and not pv.in_window(1.0, 1.0, np.inf, 1.0, 6.0)
    rng = np.random.default_rng(0)
    for _ in range(2000):
        pu, pv_, r = rng.uniform(0, 700), rng.uniform(0, 400), np.float32(rng.uniform(0, 8))
        ang = rng.uniform(0, 2 * np.pi)
        qx, qy = np.float32(pu + float(r) * np.cos(ang) * rng.choice([0.999999, 1.0, 1.000001])), np.float32(pv_ + float(r) * np.sin(ang))
        assert pv.in_window(pu, pv_, qx, qy, r) == bool(pvo.in_window(pu, pv_, qx, qy, r))


def _staged_stage1(solver, r, c, variant, case):
    """The Stage1 block of candidate c from visfs_pnp_solve on the rows of the place block."""
    rows = np.frombuffer(bytes(memoryview(r.row[c])), dtype=place.ROW_DTYPE)[:r.candidate[c].count]
    to = case["query_xyz"][rows["query_index"]] if variant["xyz"] else None
    out = solver.solve(_params(variant).pnp, pnp.camera(*vc.K, Tir=vc.TIR), rows["from_xyz"], rows["to_xy"], to)
    b = pv.Stage1()
    b.n_matches, b.n_inliers = len(out["matches"]), len(out["inliers"])
    b.matches[:b.n_matches] = out["matches"].tolist()
    b.inliers[:b.n_inliers] = out["inliers"].tolist()
    b.T[:] = out["T"].reshape(16).tolist()
    b.cov[:] = out["cov"].reshape(36).tolist()
    return b, solver.download()


HOOK_KEYS = vc.HOOK_KEYS


@pytest.mark.parametrize("name", list(vc.CASES))
def test_twin_equals_the_staged_calls(host_flow, name):
    """The place block is visfs_place_query's, stage 1 of every candidate is visfs_pnp_solve's on its rows with the shared seed (every
    byte, the hooks included), candidates from n_candidates on are zero, and guided = 0 leaves every stage-2 byte zero."""
    case = vc.case(name)
    s, db = _load(case, host_flow)
    v = pv.Verifier(db)
    solver = pnp.Pnp(512)
    for variant in case["variants"]:
        r, w = _call(v, s, case, variant)
        assert v.last_counts() == (0, 0, 0, 0)
        rc, want = db.query_raw(s, **variant["place"])
        assert rc == abi.OK and bytes(memoryview(r)) == bytes(memoryview(want)), variant
        for c in range(r.n_candidates):
            b, st = _staged_stage1(solver, r, c, variant, case)
            assert bytes(memoryview(w.candidate[c].stage1)) == bytes(memoryview(b)), (variant, c)
            got = v.download_pnp(c, 1)
            assert (got["m"], got["winner"]) == (st["m"], st["winner"])
            for key in HOOK_KEYS:
                assert got[key].tobytes() == st[key].tobytes(), (variant, c, key)
            if not variant["verify"].get("guided", 1):
                assert bytes(memoryview(w.candidate[c].stage2)) == bytes(C.sizeof(pv.Stage2))
        for c in range(r.n_candidates, 8):
            assert bytes(memoryview(w.candidate[c])) == bytes(C.sizeof(pv.Candidate)), c
            assert v.download_pnp(c, 1)["m"] == 0 and v.download_pnp(c, 2)["n_passes"] == 0
    solver.close(); v.close(); db.close(); s.close()


def _check_against_checker(v, s, case, variant):
    """One call of the twin held to the checker; returns (place block unpacked, verify block unpacked, per-candidate checker notes)."""
    r, w = _call(v, s, case, variant)
    got_p, got = place.unpack(r), pv.unpack(w, r.n_candidates)
    prm = vc.pnp_dict(variant)
    vp = dict(pvo.DEFAULTS); vp.update(variant["verify"])
    qxyz = case["query_xyz"] if variant["xyz"] else None
    want_place = po.query(case["qset"], case["slots"], **variant["place"])
    assert got_p["raw"] == want_place.tobytes()
    notes, final = [], []
    dm = 0.0
    for c, cand in enumerate(got_p["candidates"]):
        a, b = got["candidates"][c]["stage1"], got["candidates"][c]["stage2"]
        ref = pvo.stage1(prm, vc.K, vc.TIR, cand["rows"], qxyz)
        assert a["matches"].tolist() == ref["matches"].tolist() and a["inliers"].tolist() == ref["inliers"].tolist(), (variant, c)
        dm = max(dm, float(np.abs(a["T"] - ref["T"]).max()), float(np.abs(a["cov"] - ref["cov"]).max()))
        ran = bool(vp["guided"]) and len(ref["inliers"]) > 0
        assert b["ran"] == int(ran), (variant, c)
        pick, keep = v.download_guided(c)
        note = dict(stage1=len(a["inliers"]), ran=ran, rows=0, stage2=0)
        if ran:
            st = v.download_pnp(c, 1)
            R, t = pvo.rt_of(st["pass_tq"][-1])                       # the twin's stage-1 model
            slot = case["slots"][cand["slot"]]
            wp, wk, wrows = pvo.guided(R, t, vc.K, slot, case["qset"], vp["guided_radius"], vp["guided_max_distance"])
            assert pick.tolist() == wp.tolist() and keep.tolist() == wk.tolist(), (variant, c)
            assert b["rows"].tobytes() == wrows.tobytes(), (variant, c)
            ref2 = pvo.stage2(prm, vc.K, vc.TIR, R, t, wrows, qxyz)
            assert b["inliers"].tolist() == list(ref2["inliers"]), (variant, c)
            assert ref2["margin"] > 1e-4
            dm = max(dm, float(np.abs(b["T"] - ref2["T"]).max()), float(np.abs(b["cov"] - ref2["cov"]).max()))
            st2 = v.download_pnp(c, 2)
            assert st2["n_hypotheses"] == 0 and st2["winner"] == -1 and st2["m"] == len(wrows) and st2["n_passes"] == len(ref2["passes"])
            for k, (_, _, _, _, lst) in enumerate(ref2["passes"]):
                assert st2["pass_inliers"][k][:st2["pass_count"][k]].tolist() == lst
            note.update(rows=len(wrows), stage2=len(b["inliers"]), pick=wp, keep=wk)
        else:
            assert (pick == -1).all() and (keep == -1).all()
            assert not b["T"].any() and not b["cov"].any() and len(b["rows"]) == 0
        final.append(note["stage2"] if ran else note["stage1"])
        notes.append(note)
    assert got["best"] == pvo.best(final, prm["min_inliers"])
    return got_p, got, notes, dm


_PARITY = {}


def _parity(host_flow, name):
    """Every variant of a case held to the checker once; the largest pose and covariance difference."""
    if name not in _PARITY:
        case = vc.case(name)
        s, db = _load(case, host_flow)
        v = pv.Verifier(db)
        _PARITY[name] = max(_check_against_checker(v, s, case, variant)[3] for variant in case["variants"])
        v.close(); db.close(); s.close()
    return _PARITY[name]


@pytest.mark.parametrize("name", list(vc.CASES))
def test_twin_equals_the_checker_in_picks_rows_and_lists(host_flow, name):
    """Exact: the place block, the stage-1 match and inlier lists, every pick and keep, the guided rows, the stage-2 inlier list of
    every refinement pass, which stages ran, and best."""
    _parity(host_flow, name)


@pytest.mark.parametrize("name", list(vc.CASES))
def test_twin_poses_equal_the_checker_within_the_bound(host_flow, name):
    """Transforms and covariances of both stages against the checker, whose refit is Gauss-Newton run to convergence.  Measured:
    kept_rows 6.7e-12, rows_512 1.7e-12, nan_points 4.2e-14, ten_equal 4.2e-15, collinear 0 (no pose), geometry 1.3e-11 (its stage 1;
    stage 2, whose refits end in the convergence polish of section 9x, measures 5.6e-16 there)."""
    worst = _parity(host_flow, name)
    print(f"place verify parity {name}: poses and covariances {worst:.3e} (bound {POSE_BOUND:.1e})")
    assert worst <= POSE_BOUND


def test_cases_take_their_branches(host_flow):
    """What each made-to-order case is there for, on the twin's output (which the two tests above hold to the checker)."""
    def run(name, k):
        case = vc.case(name)
        s, db = _load(case, host_flow)
        v = pv.Verifier(db)
        out = _check_against_checker(v, s, case, case["variants"][k])
        v.close(); db.close(); s.close()
        return case, out

    case, (p, w, notes, _) = run("kept_rows", 0)                     # 65, 64, 63, min_inliers and min_inliers - 1 kept rows
    assert [c["count"] for c in p["candidates"]] == [65, 64, 63, 12, 11]
    assert [n["stage1"] for n in notes] == [65, 64, 63, 12, 0] and [n["ran"] for n in notes] == [True] * 4 + [False] and w["best"] == 0
    case, (p, w, notes, _) = run("rows_512", 0)
    assert p["candidates"][0]["count"] == 512 and 400 < notes[0]["stage1"] < 512 and notes[0]["rows"] >= notes[0]["stage1"]
    case, (p, w, notes, _) = run("nan_points", 0)                    # kept rows fewer than the count, a match index that is not the identity
    m = w["candidates"][0]["stage1"]["matches"]
    assert p["candidates"][0]["count"] == 80 and len(m) == 71 and m.tolist() != list(range(71))
    case, (p, w, notes, _) = run("ten_equal", 0)                     # more than eight equal counts
    assert [c["slot"] for c in p["candidates"]] == list(range(8)) and w["best"] == 0 and all(n["stage2"] == 30 for n in notes)
    assert len(run("ten_equal", 1)[1][0]["candidates"]) == 0 and run("ten_equal", 1)[1][1]["best"] == -1
    assert [c["slot"] for c in run("ten_equal", 2)[1][0]["candidates"]] == [3]
    case, (p, w, notes, _) = run("collinear", 0)                     # no valid hypothesis: no pose, stage 2 does not run
    assert p["candidates"][0]["count"] == 40 and notes[0] == dict(stage1=0, ran=False, rows=0, stage2=0) and w["best"] == -1
    case, (p, w, notes, _) = run("geometry", 0)
    order, n = case["order"], notes[0]
    rows1, rows2 = p["candidates"][0]["rows"], w["candidates"][0]["stage2"]["rows"]
    assert len(rows1) == 46 and len(rows2) == 60                      # the ratio test dropped 14 true pairs; the window finds them
    assert (n["pick"][60:63] == -1).all()                             # behind the camera
    assert n["pick"][5] == n["pick"][63] >= 0 and (n["keep"][order[5]] & 1023) == 5      # equal D from two entries: the lower j
    assert (n["pick"][8] & 1023) == min(order[8], 60) and n["keep"][max(order[8], 60)] == -1      # equal D to two queries: the lower i
    for a in range(10, 20):
        assert (n["keep"][order[a]] & 1023) == a                      # equal descriptors told apart by the window
    assert n["stage2"] >= n["stage1"]
    assert run("geometry", 3)[1][2][0]["rows"] == 0                   # radius 0: no query coincides with a projection
    assert 12 <= run("geometry", 4)[1][2][0]["rows"] < 60             # 0.5 px: inside the pixel noise
    n5 = run("geometry", 5)[1][2][0]                                  # max_distance 0: stage 2 runs, finds nothing, leaves no pose
    assert n5["ran"] and n5["rows"] == 0 and n5["stage2"] == 0 and run("geometry", 5)[1][1]["best"] == -1
    assert run("geometry", 6)[1][2][0]["rows"] == 60                  # max_distance 256: no more than at 64, the pairs stay one to one
    n7 = run("geometry", 7)[1][2][0]                                  # refine_iterations 0: the reference's quirk
    assert n7 == dict(stage1=0, ran=False, rows=0, stage2=0)
    n8 = run("geometry", 8)[1][2][0]                                  # a guided set below min_inliers
    assert n8["ran"] and 0 < n8["rows"] < 30 and n8["stage2"] == 0


def test_refusals(host_flow):
    case = vc.case("collinear")
    s, db = _load(case, host_flow)
    v = pv.Verifier(db)
    good = _params(vc.V_DEFAULT)

    def status(place_params=None, **kw):
        p = _params(vc.V_DEFAULT)
        for k, val in kw.items():
            obj, _, field = k.rpartition("__")
            setattr(getattr(p, obj) if obj else p, field, val)
        return v.query_verify_raw(s, p, None, **(place_params or {}))[0]

    assert status() == abi.OK
    for bad in (dict(first_slot=-1), dict(first_slot=2, last_slot=1), dict(max_distance=257), dict(ratio_num=0), dict(min_matches=513)):
        assert status(bad) == abi.ERR_BAD_ARGUMENT, bad
    assert status(pnp__iterations=0) == abi.ERR_BAD_ARGUMENT and status(pnp__iterations=4097) == abi.ERR_UNSUPPORTED
    assert status(pnp__refine_iterations=-1) == abi.ERR_BAD_ARGUMENT and status(pnp__refine_iterations=33) == abi.ERR_UNSUPPORTED
    assert status(pnp__reproj_error=-1.0) == abi.ERR_BAD_ARGUMENT and status(pnp__refine_sigma=float("nan")) == abi.ERR_BAD_ARGUMENT
    assert status(camera__fx=0.0) == abi.ERR_BAD_ARGUMENT and status(camera__cy=float("inf")) == abi.ERR_BAD_ARGUMENT
    for r in (-1.0, float("nan"), float("inf")):
        assert status(guided_radius=r) == abi.ERR_BAD_ARGUMENT and "guided_radius" in v.last_error()
    assert status(guided_max_distance=-1) == abi.ERR_BAD_ARGUMENT and status(guided_max_distance=257) == abi.ERR_BAD_ARGUMENT
    assert status(guided_max_distance=256) == abi.OK and status(guided_radius=0.0) == abi.OK
    fresh = place.DescriptorSet(host_flow, 8)
    assert v.query_verify_raw(fresh, good)[0] == abi.ERR_NOT_LOADED
    lib = pv.load()
    assert lib.visfs_place_query_verify(v.h, s.h, None, C.byref(good), None, None, None) == abi.ERR_BAD_ARGUMENT
    h = C.c_void_p()
    assert lib.visfs_place_verifier_create(None, C.byref(h)) == abi.ERR_BAD_ARGUMENT
    w = pv.Verifier(db)
    with pytest.raises(backend.BackendError):
        w.download_pnp(0, 1)                                          # no call yet
    assert lib.visfs_place_verify_download_pnp(v.h, 8, 1, *[None] * 13) == abi.ERR_BAD_ARGUMENT
    assert lib.visfs_place_verify_download_pnp(v.h, 0, 3, *[None] * 13) == abi.ERR_BAD_ARGUMENT
    w.close(); fresh.close(); v.close(); db.close(); s.close()


def test_the_plain_calls_are_what_they_were(host_flow):
    """visfs_place_query and visfs_pnp_solve on the same inputs before and after a verify call: the same bytes, the same counts."""
    case = vc.case("geometry")
    s, db = _load(case, host_flow)
    solver = pnp.Pnp(512)
    cam = pnp.camera(*vc.K, Tir=vc.TIR)
    rc, before = db.query_raw(s, min_matches=1)
    counts = db.last_counts()
    rows = place.unpack(before)["candidates"][0]["rows"]
    a = solver.solve(pnp.default_params(), cam, rows["from_xyz"], rows["to_xy"])
    v = pv.Verifier(db)
    _call(v, s, case, case["variants"][0])
    assert db.last_counts() == counts
    rc, after = db.query_raw(s, min_matches=1)
    assert bytes(memoryview(after)) == bytes(memoryview(before)) and db.last_counts() == counts
    b = solver.solve(pnp.default_params(), cam, rows["from_xyz"], rows["to_xy"])
    for key in ("T", "cov", "matches", "inliers"):
        assert a[key].tobytes() == b[key].tobytes()
    v.close(); solver.close(); db.close(); s.close()


# ------------------------------------------------------------------------------------------------ the closure edge
PLANAR_TRUTH = (0.40, -0.25, 0.30)        # the query's robot pose in the key-frame's robot frame: x, y (m), yaw (rad)


def _planar_case():
    """A pnp_cases scene whose motion is the planar pose above, as a one-slot verify case with 150 words."""
    x, y, yaw = PLANAR_TRUTH
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:2, 3] = [x, y]
    rng = np.random.default_rng(77)
    n = 150
    Ti = np.eye(4); Ti[:3] = np.array(vc.TIR).reshape(3, 4)
    uv = np.stack([rng.uniform(8, 744, n), rng.uniform(8, 472, n)], axis=1)
    z = rng.uniform(1.5, 9.0, n)
    cam = np.stack([(uv[:, 0] - vc.K[2]) / vc.K[0] * z, (uv[:, 1] - vc.K[3]) / vc.K[1] * z, z, np.ones(n)], axis=1)
    now = cam @ Ti.T                              # the words in the query's robot frame
    before = now @ T.T                            # ... and in the key-frame's
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    slot = dict(desc=desc, valid=np.ones(n, np.uint8), ids=np.arange(n, dtype=np.int32), xyz=before[:, :3].astype(np.float32), key=1)
    qset = dict(desc=desc.copy(), valid=np.ones(n, np.uint8), xy=(uv + rng.normal(0, 0.3, (n, 2))).astype(np.float32))
    return dict(qset=qset, slots=[slot], query_xyz=(now[:, :3] + rng.normal(0, 0.01, (n, 3))).astype(np.float32), truth=T)


def test_closure_edge_is_the_pose_of_the_query_in_the_key_frame(host_flow):
    """The direction of T is fixed here, not by reading: a key-frame i, a query j whose true pose in the frame of i is (0.40, -0.25,
    0.30 rad), 150 words with 0.3 px of pixel noise.  z of the edge is held to that pose within the 0.05 m and 0.01 rad test_pnp_host.py
    allows a pose of these scenes (measured: 3.9e-4 m, 6.4e-5 rad); the inverse direction would be (-0.31, 0.36, -0.30)."""
    case = _planar_case()
    s, db = _load(case, host_flow)
    v = pv.Verifier(db)
    r, w = _call(v, s, case, dict(vc.V_DEFAULT, xyz=True))
    got = pv.unpack(w, r.n_candidates)
    assert got["best"] == 0
    b = got["candidates"][0]["stage2"]
    z, info, oop = pv.closure_edge(b["T"], b["cov"])
    print(f"closure edge: z {z}, truth {PLANAR_TRUTH}, out of plane {oop}")
    assert np.hypot(z[0] - PLANAR_TRUTH[0], z[1] - PLANAR_TRUTH[1]) < 0.05 and abs(z[2] - PLANAR_TRUTH[2]) < 0.01
    assert np.abs(oop).max() < 0.05
    wz, winfo, woop = pvo.closure_edge(b["T"], b["cov"])
    assert np.allclose(z, wz, rtol=0, atol=1e-15) and np.allclose(oop, woop, rtol=0, atol=1e-15)
    assert np.allclose(info, winfo, rtol=1e-12, atol=0) and (info == info.T).all()
    # the information is what the pose graph takes: an odometry chain of two vertices, drifted, pulled back by the edge
    edges = [(0, 1, z, info)]
    rc, plan = pose_graph.plan([1, 0], edges)
    assert rc == abi.OK and plan["rows"] == 1
    g = pose_graph.PoseGraph(None, 8, 8)
    rc, out = g.optimize([[0, 0, 0], [0.6, -0.1, 0.2]], [1, 0], edges)
    assert rc == abi.OK, g.last_error()
    assert np.abs(out["poses"][1] - z).max() < 1e-6
    g.close(); v.close(); db.close(); s.close()


def test_closure_edge_refusals():
    T, cov = np.eye(4), np.diag([1e-4, 1e-4, 1e-4, 1e-5, 1e-5, 1e-5])
    assert pv.closure_edge_status(T, cov)[0] == abi.OK
    assert pv.closure_edge_status(None, cov)[0] == abi.ERR_BAD_ARGUMENT and pv.closure_edge_status(T, None)[0] == abi.ERR_BAD_ARGUMENT
    lib = pv.load()
    a, b, o = np.eye(4).reshape(16), cov.reshape(36).copy(), np.zeros(9)
    pd = C.POINTER(C.c_double)
    for k in range(2, 5):
        args = [x.ctypes.data_as(pd) for x in (a, b, o, o, o)]
        args[k] = None
        assert lib.visfs_place_closure_edge(*args) == abi.ERR_BAD_ARGUMENT
    bad = T.copy(); bad[1, 2] = np.nan
    assert pv.closure_edge_status(bad, cov)[0] == abi.ERR_BAD_ARGUMENT
    bad = cov.copy(); bad[5, 0] = np.inf
    assert pv.closure_edge_status(T, bad)[0] == abi.ERR_BAD_ARGUMENT
    assert pv.closure_edge_status(np.zeros((4, 4)), np.eye(6))[0] == abi.ERR_BAD_ARGUMENT          # the sentinel: no pose
    for bad in (np.zeros((6, 6)), np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -1.0]), np.diag([1.0, 0.0, 1.0, 1.0, 1.0, 1.0])):
        assert pv.closure_edge_status(T, bad)[0] == abi.ERR_BAD_ARGUMENT                           # not positive definite
    semi = np.eye(6); semi[0, 1] = semi[1, 0] = 1.0
    assert pv.closure_edge_status(T, semi)[0] == abi.ERR_BAD_ARGUMENT
    rc, z, info, oop = pv.closure_edge_status(np.eye(4), np.eye(6))                                # the identity covariance of a sentinel is accepted as a block
    assert rc == abi.OK and (info == np.eye(3)).all() and not z.any() and not oop.any()


# ------------------------------------------------------------------------------------------------ what the guided stage is for
CHAIN_SEEDS = (1, 2, 3)
# measured on the twin over the seeds 1, 2, 3 against the scene's truth (see the docstring below); three times the largest
CHAIN_ROT_TOL, CHAIN_TRANS_TOL = 3 * 1.24e-3, 3 * 6.29e-3


chain_scene, chain_camera = vc.chain_scene, vc.chain_camera


def _pose_difference(a, b):
    rot = float(np.arccos(np.clip(0.5 * (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0), -1.0, 1.0)))
    return rot, float(np.linalg.norm(a[:3, 3] - b[:3, 3]))


@pytest.mark.parametrize("seed", CHAIN_SEEDS)
def test_guided_rows_on_the_chain_scene(seed):
    """Truth: query i and entry i are the same scene point.  At the default radius (6 px) and distance (64) the checker gives
    seed 1: stage 1 178 rows (1 wrong) and 178 inliers, stage 2 188 rows (1 wrong, 0.5 %) and 188 inliers;
    seed 2: 169 rows (0 wrong), 169 inliers, then 185 rows (0 wrong) and 185 inliers;
    seed 3: 175 rows (0 wrong), 175 inliers, then 188 rows (1 wrong, 0.5 %) and 187 inliers.
    Required: at most 5 % of the guided rows wrong (the bound section 9w holds accepted matches to), and, since the checker shows a gain
    on every seed, no fewer stage-2 inliers than stage-1 inliers.  The scene has no pose of its own to compare with (the image motion is
    a rotation and a shift in the image), so, as section 9w does, the pose visfs_pnp_solve gives on the 200 true pairs stands for the
    truth, and each stage is compared with it.  Measured on the twin: stage 1 1.24e-3, 1.09e-5, 4.61e-6 rad and 6.29e-3, 5.54e-5,
    2.41e-5 m; stage 2 1.24e-3, 2.89e-6, 3.37e-6 rad and 6.28e-3, 1.43e-5, 1.68e-5 m (seed 1 carries one wrong row through both
    stages); the tolerance is three times the largest."""
    f, s, db, moved, xyz = chain_scene(seed)
    v = pv.Verifier(db)
    vp = pv.default_params(camera=chain_camera())
    p, w = v.query_verify(s, vp)
    assert [c["slot"] for c in p["candidates"]] == [0] and w["best"] == 0
    a, b = w["candidates"][0]["stage1"], w["candidates"][0]["stage2"]
    rows1, rows2 = p["candidates"][0]["rows"], b["rows"]
    # the checker on the twin's stage-1 model
    q = s.download()
    st = v.download_pnp(0, 1)
    R, t = pvo.rt_of(st["pass_tq"][-1])
    slot = dict(desc=db.download(0)["desc"], valid=db.download(0)["valid"], ids=np.arange(200, dtype=np.int32), xyz=xyz)
    _, _, wrows = pvo.guided(R, t, (vp.camera.fx, vp.camera.fy, vp.camera.cx, vp.camera.cy), slot, dict(desc=q["desc"], valid=q["valid"], xy=moved),
                             6.0, 64)
    assert rows2.tobytes() == wrows.tobytes()
    wrong1, wrong2 = int((rows1["query_index"] != rows1["db_index"]).sum()), int((wrows["query_index"] != wrows["db_index"]).sum())
    solver = pnp.Pnp(512)
    truth = solver.solve(pnp.default_params(), chain_camera(), xyz, moved)["T"]
    d1, d2 = _pose_difference(a["T"], truth), _pose_difference(b["T"], truth)
    print(f"seed {seed}: stage 1 {len(rows1)} rows ({wrong1} wrong) {len(a['inliers'])} inliers, stage 2 {len(wrows)} rows ({wrong2} wrong) "
          f"{len(b['inliers'])} inliers; to the pose of the true pairs: stage 1 {d1[0]:.3g} rad {d1[1]:.3g} m, stage 2 {d2[0]:.3g} rad {d2[1]:.3g} m")
    assert wrong2 <= 0.05 * len(wrows)
    assert len(b["inliers"]) >= len(a["inliers"]) and len(wrows) >= len(rows1)
    assert truth[3, 3] == 1.0
    for rot, trans in (d1, d2):
        assert rot <= CHAIN_ROT_TOL and trans <= CHAIN_TRANS_TOL
    solver.close(); v.close(); db.close(); s.close(); f.close()
