"""The scan refinement on the GPU (include/visfs_scan_refine.h on device sub-maps, device stacks and device groups) against the
one-core host twin, byte for byte: the record with its information matrix and the whole trace.  The CPU tests
(tests/test_scan_refine.py) hold the twin to the NumPy checker on the same cases."""
import numpy as np
import pytest

import scan_fast_cases as cases
import scan_match_cases as smc
import scan_refine_cases as rc
from visfs_amd import abi, backend
from visfs_amd import scan_fast as sf
from visfs_amd import scan_group as sg
from visfs_amd import scan_refine as sr
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu

CASES = rc.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


class World:
    """Device and host sub-maps per scene, filled once, and the cases opened on them."""

    def __init__(self, solver):
        self.solver, self.subs, self.opened = solver, {}, []

    def scene(self, scene):
        frames = scene["frames"]                                           # several cases share one scene's insertions
        key = (scene["limit"], len(frames), float(sum(np.sum(rd[1]) for _, rds in frames for rd in rds)))
        if key not in self.subs:
            pair = []
            for s in (self.solver, None):
                sub = sm.Submaps(sm.default_params(num_range_data_limit=scene["limit"]), solver=s)
                smc.fill(sub, scene)
                pair.append(sub)
            self.subs[key] = tuple(pair)
        return self.subs[key]

    def pair(self, case):
        """(device, host) Opened objects of a case."""
        if case["on"] == "grid":
            out = (rc.Opened(case, self.solver), rc.Opened(case))
        else:
            dev, host = self.scene(case["scene"])
            out = (rc.Opened(case, self.solver, subs=dev), rc.Opened(case, subs=host))
        self.opened += out
        return out

    def close(self):
        for o in self.opened:
            o.close()
        for dev, host in self.subs.values():
            dev.close(); host.close()


@pytest.fixture(scope="module")
def world(solver):
    w = World(solver)
    yield w
    w.close()


def same_on_both(dev, host, **kw):
    (sd, rd), (sh, rh) = dev.refine(**kw), host.refine(**kw)
    assert sd == sh == abi.OK, (dev.last_error(), host.last_error())
    rc.same_refinement(rd, rh, dev.trace(), host.trace())
    return rd


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_twin(world, case):
    """n = 1 with the priors (a singular occupied-space system), n about the workgroup size and 1025, every return outside (with and
    without priors: one trial, and ten rejected ones), 4 x 4 patches across the border, live sub-maps (one whose allocation trails
    its limits after a growing insertion), a stack made from a grid."""
    dev, host = world.pair(case)
    r = same_on_both(dev, host)
    assert r["refined"] == 1 and r["trials"] >= 1
    if case["name"].startswith("outside"):
        assert r["final_cost"] == r["initial_cost"] and r["termination"] == 1 and r["trials"] == (10 if case["name"] == "outside_free" else 1)


def test_point_counts_named_by_the_lanes():
    names = {c["name"]: len(c["points"]) for c in CASES}
    assert [names[f"n{n}"] for n in (rc.LANES - 1, rc.LANES, rc.LANES + 1, 1025)] == [rc.LANES - 1, rc.LANES, rc.LANES + 1, 1025]
    assert names["n1_priors"] == 1 and rc.LANES == sr.LANES


def test_the_sub_maps_are_unchanged(world):
    case = BY_NAME["after_growth_live"]
    dev, host = world.pair(case)
    i = case["scene"]["index"]
    before, info = dev.sub.download(i), dev.sub.describe()
    same_on_both(dev, host)
    after = dev.sub.download(i)
    assert dev.sub.describe() == info
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    hb = host.sub.download(i)
    assert hb[0].tobytes() == after[0].tobytes()


def test_live_sub_map_and_its_frozen_stack_agree(world):
    case = BY_NAME["after_growth_live"]
    dev, host = world.pair(case)
    fd, fh = world.pair(dict(case, on="stack"))
    a, b = same_on_both(dev, host), same_on_both(fd, fh)
    rc.same_refinement(a, b, dev.trace(), fd.trace())


def test_refused_arguments_launch_nothing_and_leave_the_hook(world):
    dev, host = world.pair(BY_NAME["base0"])
    same_on_both(dev, host)
    before = dev.trace()
    for kw in (dict(max_iterations=0), dict(translation_weight=-1.0), dict(points=np.zeros((sr.MAX_POINTS + 1, 3))), dict(initial=(np.nan, 0, 0))):
        status, _ = dev.refine(**kw)
        assert status in (abi.ERR_BAD_ARGUMENT, abi.ERR_UNSUPPORTED)
        assert dev.trace().tobytes() == before.tobytes()
    status, r = dev.refine(points=np.zeros((0, 3)))
    assert status == abi.OK and r["refined"] == 0 and len(dev.trace()) == 0


def test_sixteen_thousand_points(world):
    """The limit: 64 returns per lane."""
    dev, host = world.pair(BY_NAME["base1"])
    rng = np.random.default_rng(92)
    same_on_both(dev, host, points=smc.cast(smc.TRUTH, sr.MAX_POINTS, rng), max_iterations=3)


# ---------------------------------------------------------------- the group
def group_pair(world, cases_):
    pairs = [world.pair(dict(c, on="stack")) for c in cases_]
    gd, gh = sg.ScanStackGroup([p[0].stack for p in pairs]), sg.ScanStackGroup([p[1].stack for p in pairs])
    assert gd.status == gh.status == abi.OK, sg.create_error()
    return gd, gh, [p[0].stack for p in pairs]


def check_group(gd, gh, stacks, guesses, points, mkw, **prm):
    """match_refine on the device group: the match is byte for byte visfs_scan_group_match's, every refinement the device single
    call's from that winner and the host group's; one launch more than the plain call, equal copies and waits."""
    mp = sf.default_params(**mkw)
    res0, status0, best0 = gd.match(guesses, points, mp)
    assert gd.rc == abi.OK
    plain = gd.last_counts()
    hooks0 = [gd.match_download(i) for i in range(len(stacks))]
    res, status, best, ref = gd.match_refine(guesses, points, mp, **prm)
    assert gd.rc == abi.OK, gd.last_error()
    counts = gd.last_counts()
    assert counts == dict(plain, kernel_launches=plain["kernel_launches"] + 1)
    assert (status, best) == (status0, best0)
    resh, statush, besth, refh = gh.match_refine(guesses, points, mp, **prm)
    assert gh.rc == abi.OK and (statush, besth) == (status, best) and gd.last_error() == gh.last_error()
    for i, st in enumerate(stacks):
        rc.same_refinement(ref[i], refh[i], sr.group_trace(gd, i), sr.group_trace(gh, i))
        if status[i] != abi.OK:
            assert res[i] is None and hooks0[i] is None and gd.match_download(i) is None
            assert ref[i]["status"] == status[i] and ref[i]["refined"] == 0 and len(sr.group_trace(gd, i)) == 0
            continue
        cases.same_record(res[i], res0[i])
        cases.same_hook(gd.match_download(i), hooks0[i])
        w = res[i]
        if not w["matched"]:
            assert ref[i]["refined"] == 0 and (ref[i]["x"], ref[i]["y"], ref[i]["yaw"]) == (w["x"], w["y"], w["yaw"]) and len(sr.group_trace(gd, i)) == 0
            continue
        code, single = st.refine((w["x"], w["y"], w["yaw"]), guesses[i][:2], points, **prm)
        assert code == abi.OK and single["refined"] == 1
        rc.same_refinement(ref[i], single, sr.group_trace(gd, i), sr.stack_trace(st))
    return res, status, best, ref


def test_group_of_one(world):
    scene = BY_NAME["base0"]["scene"]
    gd, gh, stacks = group_pair(world, [BY_NAME["base0"]])
    res, status, best, ref = check_group(gd, gh, stacks, [scene["guess"]], scene["points"], dict(linear_search_window=0.3, angular_search_window=0.2))
    assert status == [abi.OK] and best == 0 and ref[0]["refined"] == 1
    gd.close(); gh.close()


def test_group_with_a_stack_twice_an_unmatched_and_an_overflowed_member(world):
    pairs = [world.pair(dict(BY_NAME[n], on="stack")) for n in ("base0", "cropped_front_live")]
    dev = [pairs[0][0].stack, pairs[0][0].stack, pairs[1][0].stack]       # one stack twice
    host = [pairs[0][1].stack, pairs[0][1].stack, pairs[1][1].stack]
    gd, gh = sg.ScanStackGroup(dev), sg.ScanStackGroup(host)
    guesses, points, mkw = rc.group_setting()
    res, status, best, ref = check_group(gd, gh, dev, guesses, points, mkw)
    assert status == [abi.OK, abi.ERR_UNSUPPORTED, abi.OK] and best == 0
    assert [r["refined"] for r in ref] == [1, 0, 0] and res[2]["matched"] == 0
    assert gd.last_error() == "member 1: frontier overflow at level 1: more than 32 nodes kept"
    # without the two obstacles every member is refined, members 0 and 1 differently (their guesses differ)
    mkw = dict(mkw, frontier_capacity=1 << 20, min_score=0.0)
    res, status, best, ref = check_group(gd, gh, dev, guesses, points, mkw)
    assert status == [abi.OK] * 3 and [r["refined"] for r in ref] == [1, 1, 1]
    # n = 0: nothing issued
    gd.match_refine(guesses, np.zeros((0, 3)), sf.default_params(**mkw))
    assert gd.rc == abi.OK and gd.last_counts() == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0)
    gd.close(); gh.close()
