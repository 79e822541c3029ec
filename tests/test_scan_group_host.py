"""The scan stack group (include/visfs_scan_group.h) on host-twin stacks: every member's record and hook data equal the single
call's on that member byte for byte, and the independent brute-force checker (tests/scan_fast_oracle.py); status, best_member,
per-member overflow, limits, errors, ABI."""
import ctypes as C

import numpy as np
import pytest

import scan_fast_cases as cases
import scan_group_cases as gc
import scan_match_cases as smc
import test_scan_fast_host as single                     # its caches of sub-maps, stacks and checker results, and its assertions
from visfs_amd import abi
from visfs_amd import scan_fast as sf
from visfs_amd import scan_group as sg

BASE, EDGE, MEMBERS, OVERFLOWS = gc.BASE, gc.EDGE, gc.MEMBERS, gc.OVERFLOWS
on, windows, single_call, argmax_lowest = gc.on, gc.windows, gc.single_call, gc.argmax_lowest


def stacks_of(members, depth=cases.DEPTH):
    return [single.stack_of(dict(c, depth=depth))[0] for c in members]


def assert_members_equal_single(group, stacks, guesses, points, **kw):
    """One group call against the single calls, member by member; returns the group's results."""
    res, status, best = group.match(guesses, points, **kw)
    assert group.rc == abi.OK, group.last_error()
    singles = []
    for i, st in enumerate(stacks):
        rc, r, hk = single_call(st, guesses[i], points, **kw)
        assert rc == abi.OK and status[i] == abi.OK, (i, st.last_error())
        cases.same_record(res[i], r)
        cases.same_hook(group.match_download(i), hk)
        singles.append(r)
    assert best == argmax_lowest(singles, status)
    return res, best


# ---------------------------------------------------------------- ABI, create
def test_abi_exports_and_create_errors(hiplib):
    lib = sg.load()
    assert lib.visfs_scan_group_abi_version() == sg.ABI_VERSION == 1
    assert sf.load().visfs_scan_fast_abi_version() == 1                     # the single matcher's ABI is as it was
    header = open(smc.ROOT + "/include/visfs_scan_group.h").read()
    for name in sg.EXPORTS:
        assert hasattr(hiplib, name), name
        assert name + "(" in header, name
    assert f"#define VISFS_SCAN_GROUP_MAX {sg.MAX_MEMBERS} " in header and f"#define VISFS_SCAN_GROUP_MAX_FRONTIER {sg.MAX_FRONTIER} " in header
    assert C.sizeof(sf.Result) == 88 and C.sizeof(sf.Params) == 32
    st7 = stacks_of([BASE[0]])[0]
    st3 = stacks_of([BASE[0]], depth=3)[0]
    for m in (0, 65):
        g = sg.ScanStackGroup([st7] * m)
        assert g.status == abi.ERR_UNSUPPORTED and g.h is None and "1 to 64" in sg.create_error()
    g = sg.ScanStackGroup([st7, st7, None])
    assert g.status == abi.ERR_BAD_ARGUMENT and "member 2" in sg.create_error() and "null" in sg.create_error()
    g = sg.ScanStackGroup([st7, st3])
    assert g.status == abi.ERR_BAD_ARGUMENT and "member 1" in sg.create_error() and "depth" in sg.create_error()
    limits, cells = cases.corner_grid()
    assert limits["resolution"] == 0.05
    fine = sf.ScanStack.from_grid(cells, limits, depth=7)
    coarse = sf.ScanStack.from_grid(cells, dict(limits, resolution=0.1), depth=7)
    assert fine.status == coarse.status == abi.OK
    g = sg.ScanStackGroup([st7, fine, coarse, fine])
    assert g.status == abi.ERR_BAD_ARGUMENT and "member 2" in sg.create_error() and "resolution" in sg.create_error()
    g = sg.ScanStackGroup([st7, fine] + [st7] * 62)                         # 64 members, grids of different sizes
    assert g.status == abi.OK and g.last_counts() == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0)
    assert g.match_download(63) is None                                     # no match yet
    g.close(); fine.close(); coarse.close()


# ---------------------------------------------------------------- a heterogeneous group
@pytest.fixture(scope="module")
def trio():
    stacks = stacks_of(MEMBERS)
    d = [st.describe() for st in stacks]
    assert len({(x["num_x_cells"], x["num_y_cells"], x["max_x"], x["max_y"]) for x in d}) >= 2      # limits differ
    assert all(x["resolution"] == cases.RES and x["depth"] == cases.DEPTH for x in d)
    g = sg.ScanStackGroup(stacks)
    assert g.status == abi.OK, sg.create_error()
    yield g, stacks
    g.close()


@pytest.mark.parametrize("case", BASE, ids=[c["name"] for c in BASE])
def test_three_different_sub_maps_equal_the_single_calls_and_the_checker(trio, case):
    g, stacks = trio
    res, best = assert_members_equal_single(g, stacks, [case["guess"]] * 3, case["points"], **windows(case))
    for i, member in enumerate(MEMBERS):
        o = single.checker(on(member, case))
        single.assert_winner(res[i], o, cases.DEPTH)
        single.assert_hook(g.match_download(i), res[i], o)
    assert res[0]["sum"] > 0 and best >= 0
    assert g.last_counts() == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0)    # a host group


def test_best_member_takes_the_lowest_index_among_equal_sums():
    a, b = stacks_of([EDGE["after_growth"], BASE[0]])           # two insertions against six: a lower sum
    case = BASE[0]
    g = sg.ScanStackGroup([a, b, b])
    res, best = assert_members_equal_single(g, [a, b, b], [case["guess"]] * 3, case["points"], **windows(case))
    assert res[1]["sum"] == res[2]["sum"] > res[0]["sum"] and best == 1
    g.close()
    g = sg.ScanStackGroup([b, b])
    res, status, best = g.match(case["guess"], case["points"], **windows(case))     # one guess for all
    assert best == 0 and res[0] == res[1]
    g.close()


def test_every_member_has_its_own_guess():
    st = stacks_of([BASE[0]])[0]
    g = sg.ScanStackGroup([st] * 5)
    guesses = [c["guess"] for c in BASE]
    assert len({tuple(x) for x in guesses}) == 5
    res, best = assert_members_equal_single(g, [st] * 5, guesses, BASE[0]["points"], **windows(BASE[0]))
    for i, c in enumerate(BASE):
        single.assert_winner(res[i], single.checker(c), cases.DEPTH)
    assert len({(r["x"], r["y"], r["yaw"]) for r in res}) > 1 and len({r["scan_index"] for r in res}) > 1
    g.close()


@pytest.mark.parametrize("depth,used,per", [(3, 3, 16), (1, 1, 169)])
def test_clipped_children_and_a_single_level(depth, used, per):
    """depth 3: L = 13, H = 2, the last children clipped by the window; depth 1: H = 0, every leaf a top node."""
    members = [BASE[0], EDGE["cropped_front"]]
    stacks = stacks_of(members, depth)
    g = sg.ScanStackGroup(stacks)
    case = BASE[1]
    res, best = assert_members_equal_single(g, stacks, [BASE[0]["guess"], case["guess"]], case["points"], **windows(case))
    for i, (member, search) in enumerate(zip(members, (BASE[0], case))):
        o = single.checker(on(member, search))
        single.assert_winner(res[i], o, depth)
        single.assert_hook(g.match_download(i), res[i], o)
        assert res[i]["depth_used"] == used and g.match_download(i)["bounds"].shape[1] == per
    g.close()


# ---------------------------------------------------------------- overflow of one member
@pytest.mark.parametrize("which,capacity,level", OVERFLOWS, ids=["keep_step", "level_sweep"])
def test_one_member_overflows_and_the_others_do_not_notice(which, capacity, level):
    over = cases.overflow_case()
    st = stacks_of([BASE[0]])[0]
    good = BASE[which]["guess"]
    kw = windows(over, frontier_capacity=capacity)
    rc, r_good, hk_good = single_call(st, good, over["points"], **kw)
    assert rc == abi.OK and capacity // 2 < max(hk_good["kept"]) <= capacity, st.last_error()     # the base member alone stays inside
    rc, _, _ = single_call(st, over["guess"], over["points"], **kw)
    assert rc == abi.ERR_UNSUPPORTED and f"frontier overflow at level {level}" in st.last_error()
    own = st.match_download()                            # the stack's own hook data: the last successful single call
    cases.same_hook(own, hk_good)
    g = sg.ScanStackGroup([st, st, st])
    res, status, best = g.match([good, over["guess"], good], over["points"], **kw)
    assert g.rc == abi.OK and status == [abi.OK, abi.ERR_UNSUPPORTED, abi.OK]
    assert res[1] is None and best == 0
    for i in (0, 2):
        cases.same_record(res[i], r_good)
        cases.same_hook(g.match_download(i), hk_good)
    assert g.match_download(1) is None                   # an all-zero header
    assert g.last_error() == f"member 1: frontier overflow at level {level}: more than {capacity} nodes kept"
    cases.same_hook(st.match_download(), own)            # the group call did not touch the member's own hook data
    # within the default capacity everything of member 1 ties at 0, and the error string is cleared
    res, status, best = g.match([good, over["guess"], good], over["points"], **windows(over))
    assert status == [abi.OK] * 3 and g.last_error() == "" and best == 0
    assert (res[1]["scan_index"], res[1]["x_offset"], res[1]["y_offset"], res[1]["sum"]) == (0, -1, -1, 0)
    assert g.match_download(1)["kept"] == g.match_download(1)["scored"]
    g.close()


# ---------------------------------------------------------------- n = 0, min_score, limits, single calls in between
def test_no_points_min_score_limits_and_single_calls_in_between(trio):
    g, stacks = trio
    case = BASE[0]
    guesses = [BASE[0]["guess"], BASE[1]["guess"], BASE[2]["guess"]]
    kw = windows(case)
    res0, status0, best0 = g.match(guesses, case["points"], **kw)
    assert g.rc == abi.OK
    hooks0 = [g.match_download(i) for i in range(3)]
    # n = 0: every guess back, nobody matched; the hook data of the last call that ran to its end stay
    res, status, best = g.match(guesses, np.zeros((0, 3)), **kw)
    assert g.rc == abi.OK and status == [abi.OK] * 3 and best == -1
    for r, gs in zip(res, guesses):
        assert r == dict(matched=0, x=gs[0], y=gs[1], yaw=gs[2], score=0.0, sum=0, scan_index=0, x_offset=0, y_offset=0, num_scans=0,
                         num_linear=0, angular_step=0.0, depth_used=0)
    for i in range(3):
        cases.same_hook(g.match_download(i), hooks0[i])
    # min_score is passed through per member: between the scores, the members below it are unmatched and cannot be best
    scores = sorted(r["score"] for r in res0)
    assert scores[0] < scores[-1]
    res, status, best = g.match(guesses, case["points"], min_score=scores[-1], **kw)
    assert [r["matched"] for r in res] == [int(r["score"] >= scores[-1]) for r in res0] and sum(r["matched"] for r in res) < 3
    assert best == argmax_lowest(res, status) and res[best]["score"] == scores[-1]
    for a, b in zip(res, res0):
        assert {k: v for k, v in a.items() if k != "matched"} == {k: v for k, v in b.items() if k != "matched"}
    res, status, best = g.match(guesses, case["points"], min_score=0.99, **kw)
    assert best == -1 and status == [abi.OK] * 3 and not any(r["matched"] for r in res)
    # the single call's checks run first and change nothing; so does the group's own limit
    refused = [
        (abi.ERR_UNSUPPORTED, guesses, case["points"], dict(kw, frontier_capacity=1 << 25), "2^26"),          # 3 * 2^25 > 2^26
        (abi.ERR_BAD_ARGUMENT, guesses, case["points"], dict(kw, frontier_capacity=3), "frontier_capacity"),
        (abi.ERR_BAD_ARGUMENT, [guesses[0], (0.0, np.nan, 0.0), guesses[2]], case["points"], kw, "member 1: the guess"),
        (abi.ERR_UNSUPPORTED, guesses, case["points"], dict(kw, linear_search_window=single.RES_L(513)), "member 0: the linear window"),
        (abi.ERR_UNSUPPORTED, guesses, np.tile(case["points"], (83, 1))[:sf.MAX_POINTS + 1], kw, "16384 points"),
    ]
    for want, gs, pts, k, word in refused:
        assert g.match(gs, pts, **k) == (None, None, None)
        assert g.rc == want and word in g.last_error(), (g.rc, g.last_error())
        for i in range(3):
            cases.same_hook(g.match_download(i), hooks0[i])
    assert sg.ScanStackGroup([stacks[0]] * 2).match(guesses[:2], case["points"], frontier_capacity=1 << 25, **kw)[1] == [abi.OK] * 2   # 2 * 2^25 is inside
    # a single call on a member between two group calls changes neither
    other = BASE[3]
    rc, r_single, hk_single = single_call(stacks[1], other["guess"], other["points"], **windows(other))
    assert rc == abi.OK
    for i in range(3):
        cases.same_hook(g.match_download(i), hooks0[i])
    res1, status1, best1 = g.match(guesses, case["points"], **kw)
    assert (status1, best1) == (status0, best0)
    for i in range(3):
        cases.same_record(res1[i], res0[i])
        cases.same_hook(g.match_download(i), hooks0[i])
    cases.same_hook(stacks[1].match_download(), hk_single)


def test_the_members_times_capacity_limit_is_the_group_s_alone():
    """frontier_capacity = 2^26 is a single call's own limit and is accepted there; a group of two refuses it."""
    case = BASE[0]
    st = stacks_of([case])[0]
    kw = windows(case, frontier_capacity=sg.MAX_FRONTIER)
    assert sg.MAX_FRONTIER == sf.MAX_FRONTIER == 2 ** 26
    rc, r, hk = single_call(st, case["guess"], case["points"], **kw)
    assert rc == abi.OK, st.last_error()
    rc, r0, hk0 = single_call(st, case["guess"], case["points"], **windows(case))
    assert rc == abi.OK
    cases.same_record(r, r0)
    cases.same_hook(hk, hk0)
    g = sg.ScanStackGroup([st, st])
    assert g.status == abi.OK
    assert g.match([case["guess"]] * 2, case["points"], **kw) == (None, None, None)
    assert g.rc == abi.ERR_UNSUPPORTED and g.last_error() == "members times frontier_capacity exceed 2^26"
    g.close()
