"""The scan refinement's one-core host twin (include/visfs_scan_refine.h on host sub-maps and host stacks) against the independent
NumPy checker of tests/scan_refine_oracle.py, its known answer, its accuracy on a smooth field, and its argument checks.  The GPU
tests hold the device to this twin byte for byte."""
import ctypes as C
import math

import numpy as np
import pytest

import scan_refine_cases as rc
import scan_refine_oracle as orc
from visfs_amd import abi
from visfs_amd import scan_fast as sf
from visfs_amd import scan_group as sg
from visfs_amd import scan_refine as sr
from visfs_amd import submap as sm

CASES = rc.cases()
# The largest deviation of the twin from the checker over CASES, measured on the CPU, was 3.4e-16: the
# polynomial against libm and the summation order, a few units in the last place per step.  The bound is 100 times that.
BOUND = 3.4e-14


def deviation(r, o):
    """The largest difference of pose (absolute), costs and information (relative to max(1, magnitude))."""
    d = max(abs(r["x"] - o["x"]), abs(r["y"] - o["y"]), abs(r["yaw"] - o["yaw"]))
    for k in ("initial_cost", "final_cost"):
        d = max(d, abs(r[k] - o[k]) / max(1.0, abs(o[k])))
    return d, float(np.abs(r["information"] - o["information"]).max() / max(1.0, np.abs(o["information"]).max()))


def check_monotone(r, trace):
    assert r["final_cost"] <= r["initial_cost"]
    accepted = trace[trace[:, 2] == 1.0][:, 0]
    assert np.all(np.diff(np.concatenate([[r["initial_cost"]], accepted])) <= 0)
    if len(accepted):
        assert accepted[-1] == r["final_cost"]


def checker(case, limits, cells, initial=None, **kw):
    prm = dict(case["prm"]); prm.update(kw)
    weights = {k: prm.pop(k) for k in list(prm) if k.endswith("_weight")}
    a = initial if initial is not None else case["initial"]
    return orc.refine(orc.Problem(orc.cost_of_cells(cells), limits, case["points"], a, case["target"], **weights), a, **prm)


def test_abi_and_defaults():
    lib = sr.load()
    assert lib.visfs_scan_refine_abi_version() == sr.ABI_VERSION == 1
    p = sr.default_params()
    assert (p.occupied_space_weight, p.translation_weight, p.rotation_weight, p.function_tolerance, p.max_iterations) == (1.0, 10.0, 40.0, 1e-6, 20)
    assert C.sizeof(sr.Result) == 6 * 4 + 14 * 8


def test_value_to_cost_conversion():
    """The checker's value -> cost table is Grid2D's, as the window solve's laser factor reads it (float)."""
    cost, _ = sm.hook_value_tables()
    assert np.array_equal(cost.astype(np.float32).astype(np.float64), orc.TABLE)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_against_checker(case):
    op = rc.Opened(case)
    status, r = op.refine()
    assert status == abi.OK and r["status"] == abi.OK and r["refined"] == 1, op.last_error()
    trace = op.trace()
    o = checker(case, *op.grid())
    ot = np.array(o["trace"], dtype=np.float64).reshape(-1, 6)
    assert (r["iterations"], r["trials"], r["termination"]) == (o["iterations"], o["trials"], o["termination"])
    assert len(trace) == r["trials"] and np.array_equal(trace[:, 2], ot[:, 2])                   # the accept / reject sequence
    pose_cost, info = deviation(r, o)
    print(f"{case['name']}: deviation {pose_cost:.3e} (information {info:.3e})")
    assert pose_cost <= BOUND and info <= BOUND
    check_monotone(r, trace)
    op.close()


def test_live_sub_map_and_its_frozen_stack_agree():
    """A host sub-map and the stack frozen from it hold the same costs: the same bytes."""
    case = next(c for c in CASES if c["name"] == "cropped_front_live")
    live = rc.Opened(case)
    frozen = rc.Opened(dict(case, on="stack"), subs=live.sub)
    (s1, r1), (s2, r2) = live.refine(), frozen.refine()
    assert s1 == s2 == abi.OK
    rc.same_refinement(r1, r2, live.trace(), frozen.trace())
    frozen.close(); live.close()


def test_known_answer_of_the_priors_alone():
    """occupied_space_weight = 0: the cost is a quadratic whose minimum is the target translation and the initial yaw."""
    case = CASES[0]
    op = rc.Opened(case)
    target, yaw = (0.41, 0.07), 0.33
    status, r = op.refine(initial=(target[0] + 0.03, target[1] - 0.02, yaw), target=target, occupied_space_weight=0.0)
    assert status == abi.OK and r["refined"] == 1
    assert abs(r["x"] - target[0]) <= 1e-12 and abs(r["y"] - target[1]) <= 1e-12 and abs(r["yaw"] - yaw) <= 1e-12
    assert r["final_cost"] <= 1e-20 and r["initial_cost"] == pytest.approx(100.0 * (0.03 ** 2 + 0.02 ** 2), rel=1e-12)
    check_monotone(r, op.trace())
    # the rotation residual is measured from the start's own yaw, so a start 0.006 rad further keeps that yaw
    status, r = op.refine(initial=(target[0] + 0.03, target[1] - 0.02, yaw + 0.006), target=target, occupied_space_weight=0.0)
    assert abs(r["x"] - target[0]) <= 1e-12 and abs(r["y"] - target[1]) <= 1e-12 and abs(r["yaw"] - (yaw + 0.006)) <= 1e-12
    np.testing.assert_allclose(r["information"], np.diag([100.0, 100.0, 1600.0]), rtol=0, atol=0)
    op.close()


@pytest.fixture(scope="module")
def field():
    limits, cells = rc.smooth_field()
    st = sf.ScanStack.from_grid(cells, limits, 1)
    assert st.status == abi.OK
    yield st, limits, orc.cost_of_cells(cells)
    st.close()


@pytest.mark.parametrize("n", rc.FIELD_COUNTS)
def test_accuracy_on_a_smooth_field(field, n):
    """Exact wall hits on a field that falls off smoothly from the walls of a rectangle that is not cell-aligned: from 20 starts
    within a cell and 0.01 rad, the result lies within 0.05 cell and 5e-4 rad of the truth.  Measured: the twin and the checker
    both reach 0.0120 cell and 3.3e-5 rad at worst over the 60 runs (n = 7: 0.0120 cell; 64: 0.0097; 360: 0.0034), below a quarter
    of the bound."""
    st, limits, cost = field
    pts = rc.wall_scan(rc.FIELD_TRUTH, n)
    worst = [0.0, 0.0, 0.0, 0.0]
    for start in rc.field_starts():
        status, r = st.refine(start, start[:2], pts, **rc.FIELD_PRM)
        assert status == abi.OK and r["refined"] == 1
        o = orc.refine(orc.Problem(cost, limits, pts, start, start[:2], 1.0, 0.0, 0.0), start, function_tolerance=0.0)
        for k, q in enumerate((r, o)):
            worst[2 * k] = max(worst[2 * k], abs(q["x"] - rc.FIELD_TRUTH[0]) / rc.RES, abs(q["y"] - rc.FIELD_TRUTH[1]) / rc.RES)
            worst[2 * k + 1] = max(worst[2 * k + 1], abs(q["yaw"] - rc.FIELD_TRUTH[2]))
        check_monotone(r, sr.stack_trace(st))
    print(f"n = {n}: twin {worst[0]:.4f} cell, {worst[1]:.2e} rad; checker {worst[2]:.4f} cell, {worst[3]:.2e} rad")
    assert worst[2] <= 0.05 / 4 and worst[3] <= 5e-4 / 4                  # the checker itself, else the bound says nothing
    assert worst[0] <= 0.05 and worst[1] <= 5e-4


def test_nothing_to_refine():
    """n == 0 and no sub-map yet: refined = 0, the start back, no trials."""
    case = CASES[0]
    op = rc.Opened(case)
    status, r = op.refine()
    assert status == abi.OK and len(op.trace()) == r["trials"] > 0
    status, r = op.refine(points=np.zeros((0, 3)))
    assert status == abi.OK and (r["refined"], r["iterations"], r["trials"]) == (0, 0, 0) and (r["x"], r["y"], r["yaw"]) == tuple(case["initial"])
    assert len(op.trace()) == 0
    op.close()
    empty = sm.Submaps(sm.default_params())
    status, r = empty.refine(case["initial"], case["target"], case["points"])
    assert status == abi.OK and r["refined"] == 0 and (r["x"], r["y"], r["yaw"]) == tuple(case["initial"])
    assert len(sr.submaps_trace(empty)) == 0
    empty.close()


BAD = [
    ("nan_pose", dict(initial=(math.nan, 0.0, 0.0)), abi.ERR_BAD_ARGUMENT),
    ("inf_target", dict(target=(0.0, math.inf)), abi.ERR_BAD_ARGUMENT),
    ("nan_point", dict(points=np.array([[0.0, math.nan, 0.0]])), abi.ERR_BAD_ARGUMENT),
    ("negative_weight", dict(occupied_space_weight=-1.0), abi.ERR_BAD_ARGUMENT),
    ("nan_weight", dict(translation_weight=math.nan), abi.ERR_BAD_ARGUMENT),
    ("inf_weight", dict(rotation_weight=math.inf), abi.ERR_BAD_ARGUMENT),
    ("negative_tolerance", dict(function_tolerance=-1e-9), abi.ERR_BAD_ARGUMENT),
    ("no_iterations", dict(max_iterations=0), abi.ERR_BAD_ARGUMENT),
    ("too_many_iterations", dict(max_iterations=51), abi.ERR_BAD_ARGUMENT),
    ("too_many_points", dict(points=np.zeros((sr.MAX_POINTS + 1, 3))), abi.ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("on", ["stack", "live"])
def test_refused_arguments_leave_the_hook_data(on):
    case = dict(CASES[0], on=on)
    op = rc.Opened(case)
    status, r = op.refine()
    assert status == abi.OK
    before = op.trace()
    for name, kw, code in BAD:
        status, _ = op.refine(**kw)
        assert status == code and op.last_error() != "", name
        after = op.trace()
        assert after.shape == before.shape and after.tobytes() == before.tobytes(), name
    if on == "live":
        status, _ = op.sub.refine(case["initial"], case["target"], case["points"], index=5)
        assert status == abi.ERR_BAD_ARGUMENT and op.trace().tobytes() == before.tobytes()
    # the limit itself is accepted
    status, r = op.refine(points=np.tile(case["points"], (83, 1))[:sr.MAX_POINTS], max_iterations=2)
    assert status == abi.OK and r["refined"] == 1 and r["iterations"] <= 2
    op.close()


# ---------------------------------------------------------------- the group: host twins
@pytest.fixture(scope="module")
def stacks():
    """Host stacks of the base scene (twice the same object is allowed) and of the cropped front."""
    base = rc.Opened(dict(CASES[0], on="stack"))
    crop = rc.Opened(dict(next(c for c in CASES if c["name"] == "cropped_front_live"), on="stack"))
    yield base.stack, crop.stack
    base.close(); crop.close()


def group_against_singles(g, members, guesses, points, mp, **prm):
    """match_refine on the group: the match is visfs_scan_group_match's, each refinement the single call's from that winner."""
    res0, status0, best0 = g.match(guesses, points, mp)
    assert g.rc == abi.OK
    res, status, best, ref = g.match_refine(guesses, points, mp, **prm)
    assert g.rc == abi.OK, g.last_error()
    assert (status, best) == (status0, best0)
    for i, st in enumerate(members):
        if status[i] != abi.OK:
            assert res[i] is None and ref[i]["status"] == status[i] and ref[i]["refined"] == 0 and len(sr.group_trace(g, i)) == 0
            continue
        assert res[i] == res0[i]
        w = res[i]
        if not w["matched"]:
            assert ref[i]["refined"] == 0 and (ref[i]["x"], ref[i]["y"], ref[i]["yaw"]) == (w["x"], w["y"], w["yaw"]) and len(sr.group_trace(g, i)) == 0
            continue
        code, single = st.refine((w["x"], w["y"], w["yaw"]), guesses[i][:2], points, **prm)
        assert code == abi.OK and single["refined"] == 1
        rc.same_refinement(ref[i], single, sr.group_trace(g, i), sr.stack_trace(st))
    return res, status, best, ref


def test_host_group_match_refine(stacks):
    base, crop = stacks
    scene = CASES[0]["scene"]
    mp = sf.default_params(linear_search_window=0.3, angular_search_window=0.2)
    g = sg.ScanStackGroup([base, crop, base])
    guesses = [scene["guess"], scene["guess"], rc._near(scene["guess"], 0.1, 0.05, 0.02)]
    res, status, best, ref = group_against_singles(g, [base, crop, base], guesses, scene["points"], mp)
    assert status == [abi.OK] * 3 and all(r["refined"] == 1 for r in ref) and g.last_counts()["kernel_launches"] == 0
    # one member unmatched through min_score: only the good members are refined
    scores = sorted(r["score"] for r in res)
    mp2 = sf.default_params(linear_search_window=0.3, angular_search_window=0.2, min_score=(scores[0] + scores[-1]) / 2)
    assert scores[0] < scores[-1]
    res, status, best, ref = group_against_singles(g, [base, crop, base], guesses, scene["points"], mp2)
    assert sorted(r["refined"] for r in ref) in ([0, 0, 1], [0, 1, 1])
    # n = 0: every guess back
    res, status, best, ref = g.match_refine(guesses, np.zeros((0, 3)), mp)
    assert g.rc == abi.OK and best == -1 and all(r["refined"] == 0 for r in ref)
    assert [(r["x"], r["y"], r["yaw"]) for r in ref] == [tuple(q) for q in guesses]
    # a refused refinement parameter refuses the whole call
    assert g.match_refine(guesses, scene["points"], mp, max_iterations=0) == (None, None, None, None) and g.rc == abi.ERR_BAD_ARGUMENT
    g.close()
