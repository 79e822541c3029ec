"""Monte-Carlo localisation (include/visfs_mcl.h) on the CPU: the one-core host twin against the checker of
tests/mcl_oracle.py, byte for byte in the field (t, q, v_occ, T) and in the filter (x, y, yaw, w, Q, ancestors and every field of the
result), on the cases of tests/mcl_cases.py; known answers, refusals, sincos_any against libm, and that the filter localises.
tests/test_gpu_mcl.py holds the device to the twin."""
import functools
import math

import numpy as np
import pytest

import mcl_cases as mc
import mcl_oracle as mo
from visfs_amd import abi
from visfs_amd import global_map as gm
from visfs_amd import mcl

FIELD_CASES = mc.field_cases()
FIELD_BY_NAME = {c["name"]: c for c in FIELD_CASES}
FILTER_CASES = mc.filter_cases()
STATE_KEYS = ("x", "y", "yaw", "w", "Q", "ancestors")
RESULT_KEYS = ("status", "resampled", "best", "n_beams", "update", "mean", "covariance", "n_eff", "W", "best_pose", "best_weight")


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_result(got, want, what=""):
    for k in RESULT_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            a, b = a.astype(np.float64), b.astype(np.float64)
            assert a.tobytes() == b.tobytes(), (what, k, got[k], want[k])
        else:
            assert np.array_equal(a, b), (what, k, got[k], want[k])


def same_state(got, want, what=""):
    for k in STATE_KEYS:
        same(got[k], np.asarray(want[k]), (what, k))


@functools.lru_cache(maxsize=None)
def field_reference(name):
    c = FIELD_BY_NAME[name]
    out = mo.field(c["cells"], c["limits"]["resolution"], **c["params"])
    out[0].setflags(write=False); out[1].setflags(write=False)
    return out


def twin_field(case):
    f = mcl.Field.from_grid(case["cells"], case["limits"], mcl.field_params(**case["params"]))
    assert f.status == abi.OK
    return f


@functools.lru_cache(maxsize=None)
def room_twin():
    cells, lim = mc.room()
    f = mcl.Field.from_grid(cells, lim)
    assert f.status == abi.OK
    return f


def oracle_filter(N, seed):
    t, q, _, T, _ = mc.room_field()
    _, lim = mc.room()
    return mo.Filter(t, q, T, lim["resolution"], lim["max_x"], lim["max_y"], N, seed)


# ---------------------------------------------------------------- the field: known answers of the checker, then twin = checker
def test_field_known_answers_of_the_checker():
    t, q, v_occ, T, R = field_reference("no_obstacle")
    assert (R, T) == (10, 100) and (t == T).all()
    assert field_reference("one_by_one")[0].tolist() == [[0]]
    t, _, _, T, _ = field_reference("corner")
    assert all(t[y, x] == min(T, x * x + y * y) for y in range(20) for x in range(30)) and t[0, 10] == 100 and t[6, 8] == 100 and t[6, 7] == 85
    t, _, _, T, _ = field_reference("middle")
    assert all(t[y, x] == min(T, (x - 15) ** 2 + (y - 10) ** 2) for y in range(21) for x in range(31))
    t = field_reference("two_equidistant")[0]
    assert t[4, 10] == 36 and t[4, 9] == 25 and t[4, 11] == 25 and t[0, 10] == 52
    t, _, _, T, R = field_reference("radius_one")
    assert (R, T) == (1, 3) and t[4, 5] == 0 and t[4, 4] == 1 and t[3, 4] == 2 and t[4, 3] == 3 and t[2, 5] == 3 and t[7, 0] == 1
    t, _, _, T, R = field_reference("radius_beyond_grid")
    assert (R, T) == (40, 1600) and all(t[y, x] == (x - 2) ** 2 + (y - 3) ** 2 for y in range(7) for x in range(9))
    t, q, _, T, R = field_reference("square_is_integer")
    assert (R, T) == (10, 100) and t[3, 13] == 100 and t[3, 12] == 81 and t[9, 11] == 100 and t[29, 39] == 100 and len(q) == 101
    assert field_reference("square_is_no_integer")[3:] == (44, 6)
    t, _, v_occ, T, _ = field_reference("v_occ_and_the_next")
    assert 1.0 - mo.value_cost(v_occ) >= 0.65 > 1.0 - mo.value_cost(v_occ + 1)
    assert t[2, 3] == 0 and t[2, 8] == 25 and t[2, 11] == 64
    t = field_reference("unknown_beside")[0]
    assert t[1, 4] == 0 and t[1, 5] == 1 and t[1, 6] == 4
    q = field_reference("no_obstacle")[1]
    assert q[0] == mo.llround((0.5 + 0.5 / 12.0) ** 3 * 2.0 ** 40) and all(q[i] > q[i + 1] for i in range(len(q) - 1))


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c["name"] for c in FIELD_CASES])
def test_field_twin_equals_checker(case):
    t, q, v_occ, T, R = field_reference(case["name"])
    f = twin_field(case)
    gt, gq, gv, gT = f.download()
    same(gt, t, "t"); same(gq, q, "q")
    assert (gv, gT) == (v_occ, T)
    d = f.describe()
    assert (d["R"], d["T"], d["v_occ"], d["device"]) == (R, T, v_occ, 0)
    assert {k: d[k] for k in gm.LIMIT_KEYS} == case["limits"]
    assert f.last_counts() == (0, 0, 0)
    f.close()


def test_field_from_a_composed_two_tile_map_equals_the_field_of_its_download():
    rng = np.random.default_rng(4)
    m = gm.GlobalMap()
    a, b = mc.sprinkled(rng, 40, 30, 0.02), mc.sprinkled(rng, 35, 45, 0.02)
    assert m.add_grid(a, mc.limits(40, 30), (0.0, 0.0, 0.0))[0] == abi.OK
    assert m.add_grid(b, mc.limits(35, 45), (1.1, -0.4, 0.5))[0] == abi.OK
    assert mcl.Field.from_map(m).status == abi.ERR_BAD_ARGUMENT                 # nothing composed yet
    rc, info = m.compose(gm.ODDS)
    assert rc == abi.OK
    _, cells, _ = m.download()
    lim = {k: info[k] for k in gm.LIMIT_KEYS}
    p = mcl.field_params(max_dist=0.6)
    fa, fb = mcl.Field.from_map(m, p), mcl.Field.from_grid(cells, lim, p)
    assert (fa.status, fb.status) == (abi.OK, abi.OK)
    m.close()                                                                    # the field outlives the map
    assert fa.describe() == fb.describe()
    ta, tb = fa.download(), fb.download()
    same(ta[0], tb[0]); same(ta[1], tb[1])
    assert ta[2:] == tb[2:] and (ta[0] == 0).any() and (ta[0] == ta[3]).any()
    t = mo.field(cells, lim["resolution"], max_dist=0.6)[0]
    same(ta[0], t)
    fa.close(); fb.close()


def test_field_refusals():
    cells, lim = mc.grid(8, 6, [(1, 1)]), mc.limits(8, 6)
    for kw in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(z_hit=-1.0), dict(z_rand=0.0), dict(sigma_hit=float("inf")), dict(range_max=0.0),
               dict(occupied_probability=1.5), dict(occupied_probability=0.0), dict(z_hit=7.0)):    # 7^3 2^40 > 2^48
        assert mcl.Field.from_grid(cells, lim, mcl.field_params(**kw)).status == abi.ERR_BAD_ARGUMENT, kw
    assert mcl.Field.from_grid(cells, lim, mcl.field_params(max_dist=12.8)).status == abi.ERR_UNSUPPORTED    # R = 256
    assert mcl.Field.from_grid(cells, lim, mcl.field_params(max_dist=12.79)).status == abi.OK               # R = 255
    for bad in (dict(lim, resolution=0.0), dict(lim, num_x_cells=0), dict(lim, max_x=float("nan"))):
        assert mcl.Field.from_grid(cells, bad).status == abi.ERR_BAD_ARGUMENT
    assert mcl.load().visfs_mcl_abi_version() == mcl.ABI_VERSION == 1


# ---------------------------------------------------------------- sincos_any against libm
SINCOS_MEASURED_ULPS = 2.0      # the largest error of this sweep against math.sin and math.cos, for both


def test_sincos_any_against_libm():
    a = np.concatenate([np.linspace(-4.0, 4.0, 20001)] + [k * (math.pi / 2) + np.linspace(-1e-3, 1e-3, 401) for k in range(-3, 4)] +
                       [k * (math.pi / 2) + np.array([-1e-9, -1e-12, 0.0, 1e-12, 1e-9]) for k in range(-3, 4)])
    a = a[np.abs(a) <= 4.0 + 1e-9]
    s, c = mcl.hook_sincos(a)
    os_, oc = mo.sincos_any(a)
    same(s, os_); same(c, oc)                                                   # the twin's and the checker's are the same function
    worst = 0.0
    for x, sv, cv in zip(a.tolist(), s.tolist(), c.tolist()):
        for got, want in ((sv, math.sin(x)), (cv, math.cos(x))):
            worst = max(worst, abs(got - want) / math.ulp(want) if want != 0.0 else abs(got) / 5e-324)
    print(f"sincos_any: largest error {worst:.3f} ulp over {len(a)} angles")
    assert worst <= 4.0 * SINCOS_MEASURED_ULPS, worst


# ---------------------------------------------------------------- the filter: known answers
def twin_filter(N, seed):
    f = mcl.Filter(room_twin(), N, seed)
    assert f.status == abi.OK
    return f


ZERO = dict(alpha1=0.0, alpha2=0.0, alpha3=0.0, alpha4=0.0)


def test_one_particle_whose_beams_all_end_on_obstacles():
    pts = mc.cast(mc.ROOM_CENTRE, 40)
    assert len(pts) == 40
    q = mc.room_field()[1]
    for f in (twin_filter(1, 3), oracle_filter(1, 3)):
        assert f.init(mc.ROOM_CENTRE, (0, 0, 0)) in (None, abi.OK)
        r = f.update((0, 0, 0), pts, **ZERO) if isinstance(f, mo.Filter) else f.update((0, 0, 0), pts, mcl.default_params(**ZERO))[1]
        st = f.state() if isinstance(f, mo.Filter) else f.download()
        assert st["Q"][0] == 40 * int(q[0])
        assert r["W"] == 1.0 + (40 * int(q[0])) / 2.0 ** 40 and st["w"][0] == 1.0 and r["n_eff"] == 1.0 and r["resampled"] == 0
        assert (st["x"][0], st["y"][0], st["yaw"][0]) == mc.ROOM_CENTRE and r["mean"][:2] == list(mc.ROOM_CENTRE[:2])


def both(N, seed):
    return twin_filter(N, seed), oracle_filter(N, seed)


def step(f, delta, pts, **kw):
    """(result, state) of one update on the twin or on the checker."""
    if isinstance(f, mo.Filter):
        return f.update(delta, pts, **kw), f.state()
    rc, r = f.update(delta, pts, mcl.default_params(**kw))
    assert rc == abi.OK, f.last_error()
    return r, f.download()


def test_beams_outside_the_grid_and_no_beams_leave_the_weights():
    far = np.array([[100.0, 0.0, 0.0], [0.0, -90.0, 0.0], [-70.0, 70.0, 0.0]])
    T, q = mc.room_field()[3], mc.room_field()[1]
    for f in both(50, 9):
        f.init(mc.ROOM_CENTRE, (0.2, 0.2, 0.1))
        before = {k: np.array(v) for k, v in (f.state() if isinstance(f, mo.Filter) else f.download()).items()}
        r, st = step(f, (0.1, 0.0, 0.05), far, resample_interval=5)
        assert (st["Q"] == 3 * int(q[T])).all() and r["W"] == 1.0 + 3 * int(q[T]) / 2.0 ** 40 and (st["w"] == st["w"][0]).all()
        assert abs(st["w"][0] - 1.0 / 50) < 1e-17 and not (st["x"] == before["x"]).any()
        w = np.array(st["w"])
        r, st2 = step(f, (0.1, 0.0, 0.05), np.zeros((0, 3)), resample_interval=5)
        assert (st2["Q"] == 0).all() and r["W"] == mo.tree_sum(w) and r["n_beams"] == 0
        same(st2["w"], w / r["W"])
        assert not (st2["x"] == st["x"]).any()                                 # the motion is still applied


def test_zero_alphas_and_a_zero_delta_leave_the_state_bytes():
    for f in both(65, 10):
        f.init((3.0, 3.0, 3.0), (0.3, 0.3, 0.3))
        a = {k: np.array(v) for k, v in (f.state() if isinstance(f, mo.Filter) else f.download()).items()}
        assert (a["yaw"] < 0).any() and (a["yaw"] > 3.0).any()                 # the initial yaws wrapped
        _, b = step(f, (0.0, 0.0, 0.0), np.zeros((0, 3)), resample_interval=3, **ZERO)
        for k in ("x", "y", "yaw"):
            same(b[k], a[k], k)


def test_a_forward_delta_moves_every_particle_along_its_own_yaw():
    for f in both(64, 11):
        f.init(mc.ROOM_CENTRE, (0.1, 0.1, 1.0))
        a = {k: np.array(v) for k, v in (f.state() if isinstance(f, mo.Filter) else f.download()).items()}
        _, b = step(f, (0.25, 0.0, 0.0), np.zeros((0, 3)), resample_interval=3, **ZERO)
        same(b["yaw"], a["yaw"])
        assert np.abs(b["x"] - (a["x"] + 0.25 * np.cos(a["yaw"]))).max() < 1e-15 and np.abs(b["y"] - (a["y"] + 0.25 * np.sin(a["yaw"]))).max() < 1e-15


def test_a_yaw_near_pi_wraps_to_the_negative_side():
    for f in both(1, 12):
        f.init((3.0, 3.0, math.pi - 1e-3), (0, 0, 0))
        _, b = step(f, (0.0, 0.0, 0.01), np.zeros((0, 3)), **ZERO)
        assert b["yaw"][0] == (math.pi - 1e-3) + 0.01 - mo.TWO_PI and -math.pi < b["yaw"][0] < -3.13


def set_state(f, x, y, yaw, w):
    if isinstance(f, mo.Filter):
        f.x, f.y, f.yaw, f.w = (np.array(v, dtype=np.float64) for v in (x, y, yaw, w))
    else:
        assert f.upload(x, y, yaw, w) == abi.OK, f.last_error()


def test_resampling_known_answers():
    N = 97
    rng = np.random.default_rng(13)
    x, y, yaw = rng.random(N) + 2.0, rng.random(N) + 2.0, rng.random(N)
    one = np.zeros(N); one[41] = 1.0
    rand = rng.random(N) ** 3
    rand[5] = 0.0
    for f in both(N, 13):
        for w, check in ((np.full(N, 1.0 / N), "identity"), (one, "one"), (rand, "random")):
            set_state(f, x, y, yaw, w)
            r, st = step(f, (0, 0, 0), np.zeros((0, 3)), resample_interval=1, n_eff_ratio=2.0, **ZERO)
            assert r["resampled"] == 1 and (st["w"] == 1.0 / N).all()
            anc = st["ancestors"]
            same(st["x"], x[anc])
            if check == "identity":
                assert (anc == np.arange(N)).all()
            elif check == "one":
                assert (anc == 41).all()
            else:
                k = [int(math.floor(v * 2.0 ** 40)) for v in (w / mo.tree_sum(w)).tolist()]
                mult = np.bincount(anc, minlength=N)
                assert mult.sum() == N and mult[5] == 0 and (np.diff(anc) >= 0).all()
                assert all(abs(int(mult[j]) * sum(k) - N * k[j]) <= sum(k) for j in range(N))     # within 1 of N k_j / K, in integers
        set_state(f, x, y, yaw, rand)
        r, st = step(f, (0, 0, 0), np.zeros((0, 3)), resample_interval=1, n_eff_ratio=0.0, **ZERO)    # n_eff is never below 0
        assert r["resampled"] == 0 and (st["ancestors"] == np.arange(N)).all() and abs(r["n_eff"] - rand.sum() ** 2 / (rand ** 2).sum()) < 1e-9


# ---------------------------------------------------------------- the filter: twin = checker over ten updates
@pytest.mark.parametrize("case", FILTER_CASES, ids=[c["name"] for c in FILTER_CASES])
def test_filter_twin_equals_checker(case):
    f, o = both(case["N"], case["seed"])
    assert f.init(case["mean"], case["sigma"]) == abi.OK
    o.init(case["mean"], case["sigma"])
    same_state(f.download(), o.state(), "init")
    ran = []
    for k, (d, pts) in enumerate(zip(case["deltas"], case["clouds"])):
        (ra, sa), (rb, sb) = step(f, d, pts, **case["params"]), step(o, d, pts, **case["params"])
        same_result(ra, rb, k); same_state(sa, sb, k)
        assert f.last_counts() == (0, 0, 0) and f.last_result() == (abi.OK, ra)
        ran.append(ra["resampled"])
    if case["N"] > 1:
        assert ran == [0, 1] * 5                                                # run and skipped by turns
    if case["params"]["max_beams"]:
        assert ra["n_beams"] == len(case["clouds"][-1][::-(-60 // case["params"]["max_beams"])]) <= case["params"]["max_beams"]
    f.close()


def test_filter_refusals_leave_the_state():
    f = twin_filter(10, 1)
    assert f.init(mc.ROOM_CENTRE, (0.1, 0.1, 0.1)) == abi.OK
    pts = mc.cloud(np.random.default_rng(1), 5)
    rc, r = f.update((0.1, 0, 0), pts)
    assert rc == abi.OK
    st = f.download()
    bad_pts = pts.copy(); bad_pts[2, 0] = float("nan")
    for delta, p, prm in (((float("nan"), 0, 0), pts, {}), ((0.1, 0, 0), bad_pts, {}), ((0.1, 0, 0), pts, dict(alpha1=-1.0)),
                          ((0.1, 0, 0), pts, dict(resample_interval=0)), ((0.1, 0, 0), pts, dict(max_beams=-1)),
                          ((0.1, 0.0, 6.0), pts, {}), ((0.1, 0.0, 7.0), pts, ZERO),            # the yaw step with its noise, and alone
                          ((1.0, 0, 2.0), pts, dict(alpha1=1.0))):              # |rot1 + rot2| + 6 (sigma + sigma) > 2 pi
        assert f.update(delta, p, mcl.default_params(**prm))[0] == abi.ERR_BAD_ARGUMENT, (delta, prm)
        same_state(f.download(), st)
        assert f.last_result() == (abi.OK, r)
    assert f.update((0.1, 0, 0), np.zeros((mcl.MAX_BEAMS + 1, 3)))[0] == abi.ERR_BAD_ARGUMENT
    assert f.init((0, 0, 0), (0.1, -0.1, 0.1)) == abi.ERR_BAD_ARGUMENT and f.init((0, 0, 0), (0.1, 0.1, 2.0)) == abi.ERR_BAD_ARGUMENT
    assert f.upload(st["x"], st["y"], st["yaw"], np.zeros(10)) == abi.ERR_BAD_ARGUMENT
    same_state(f.download(), st)
    for n in (0, mcl.MAX_PARTICLES + 1):
        assert mcl.Filter(room_twin(), n).status == abi.ERR_BAD_ARGUMENT
    assert f.set_lanes(3) == abi.ERR_BAD_ARGUMENT and f.set_lanes(64) == abi.OK
    assert f.update((0.1, 0, 0), pts)[0] == abi.OK and f.download()["Q"].any()
    f.close()


# ---------------------------------------------------------------- it localises
# The checker's final pose error on the scene over the seeds 1 .. 5 (metres, radians), measured on the CPU; the test holds the
# checker, and so the twin that equals it, to three times the worst of them.
MEASURED_ERRORS = [(0.0589, 0.0188), (0.0638, 0.0166), (0.0557, 0.0165), (0.0626, 0.0198), (0.0671, 0.0170)]
LOCALISE_BOUND = (3.0 * max(e[0] for e in MEASURED_ERRORS), 3.0 * max(e[1] for e in MEASURED_ERRORS))


def localise(f):
    s = mc.localisation_scene()
    start = tuple(a + b for a, b in zip(s["poses"][0], s["offset"]))
    f.init(start, s["sigma"])
    out = []
    for d, pts in zip(s["odometry"], s["scans"]):
        out.append(step(f, d, pts)[0])
    return out


def test_it_localises():
    s = mc.localisation_scene()
    f, o = both(s["N"], 1)
    ra, rb = localise(f), localise(o)
    for k, (a, b) in enumerate(zip(ra, rb)):
        same_result(a, b, k)
    same_state(f.download(), o.state())
    et, er = mc.pose_error(rb[-1]["mean"], s["poses"][-1])
    trace = [r["covariance"][0] + r["covariance"][4] + r["covariance"][8] for r in rb]
    print(f"localisation: final error {et:.4f} m, {er:.4f} rad; n_eff {rb[0]['n_eff']:.1f}; trace {trace[0]:.4f} -> {trace[-1]:.4f}")
    assert rb[0]["n_eff"] < s["N"]                                              # the first scan tells the particles apart
    assert trace[-1] < trace[0]
    assert et <= LOCALISE_BOUND[0] and er <= LOCALISE_BOUND[1], (et, er)
    f.close()
