"""The scan stack group on the GPU (include/visfs_scan_group.h on device stacks) against the host group of the twins' stacks and
against device single calls on the same stacks, byte for byte: records, status, best_member and every hook array (B, the per-level
counts, the top level's bounds, the sorted survivors).  The CPU tests hold the host group to the brute-force checker on the same
sub-maps."""
import numpy as np
import pytest

import scan_fast_cases as cases
import scan_group_cases as gc
import scan_match_cases as smc
from visfs_amd import abi, backend
from visfs_amd import scan_group as sg
from visfs_amd import submap as sm

pytestmark = pytest.mark.gpu

BASE, EDGE, MEMBERS = gc.BASE, gc.EDGE, gc.MEMBERS
ZERO = dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0)


@pytest.fixture(scope="module")
def solver():
    s = backend.Solver(abi.default_params())
    yield s
    s.close()


class World:
    """Device and host sub-maps of the member cases, and their frozen stacks by (member, depth)."""

    def __init__(self, solver):
        self.subs, self.stacks = [], {}
        for case in MEMBERS:
            dev = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]), solver=solver)
            host = sm.Submaps(sm.default_params(num_range_data_limit=case["limit"]))
            smc.fill(dev, case)
            smc.fill(host, case)
            self.subs.append((dev, host, case["index"]))

    def pair(self, member, depth=cases.DEPTH):
        """(device stack, host stack) of member sub-map `member`."""
        if (member, depth) not in self.stacks:
            dev, host, index = self.subs[member]
            out = []
            for sub in (dev, host):
                st = sub.freeze(index, depth)
                assert st.status == abi.OK, sub.last_error()
                out.append(st)
            self.stacks[member, depth] = tuple(out)
        return self.stacks[member, depth]

    def groups(self, members, depth=cases.DEPTH):
        """(device group, host group, device stacks) over the member sub-maps listed."""
        pairs = [self.pair(i, depth) for i in members]
        gd, gh = sg.ScanStackGroup([p[0] for p in pairs]), sg.ScanStackGroup([p[1] for p in pairs])
        assert gd.status == gh.status == abi.OK, sg.create_error()
        return gd, gh, [p[0] for p in pairs]

    def close(self):
        for pair in self.stacks.values():
            for st in pair:
                st.close()
        for dev, host, _ in self.subs:
            dev.close(); host.close()


@pytest.fixture(scope="module")
def world(solver):
    w = World(solver)
    yield w
    w.close()


def same_groups(gd, gh, guesses, points, singles=None, **kw):
    """One call on the device group and one on the host group: status, best_member, records and hook data equal; with `singles`
    (the device stacks), equal to the device single calls as well.  Returns the device group's (results, status, best)."""
    rd, sd, bd = gd.match(guesses, points, **kw)
    assert gd.rc == abi.OK, gd.last_error()
    rh, sh, bh = gh.match(guesses, points, **kw)
    assert gh.rc == abi.OK, gh.last_error()
    assert (sd, bd) == (sh, bh) and gd.last_error() == gh.last_error()
    assert gh.last_counts() == ZERO
    for i in range(len(sd)):
        hd, hh = gd.match_download(i), gh.match_download(i)
        if sd[i] != abi.OK:
            assert rd[i] is None and rh[i] is None and hd is None and hh is None
            continue
        cases.same_record(rd[i], rh[i])
        cases.same_hook(hd, hh)
        if singles is not None:
            g = guesses[i] if np.ndim(guesses) == 2 else guesses
            rc, r, hk = gc.single_call(singles[i], g, points, **kw)
            assert rc == abi.OK, singles[i].last_error()
            cases.same_record(rd[i], r)
            cases.same_hook(hd, hk)
    return rd, sd, bd


@pytest.mark.parametrize("case", BASE, ids=[c["name"] for c in BASE])
def test_three_different_sub_maps(world, case):
    """200 x 200, a cropped front and a grid frozen after growth; L = 13, S = 27, n = 200, H = 4."""
    gd, gh, stacks = world.groups([0, 1, 2])
    res, status, best = same_groups(gd, gh, [case["guess"]] * 3, case["points"], singles=stacks, **gc.windows(case))
    assert status == [abi.OK] * 3 and best == gc.argmax_lowest(res, status) and best >= 0
    assert all((r["num_scans"], r["num_linear"], r["depth_used"]) == (27, 6, 5) for r in res)
    assert abs(res[0]["x"] - case["truth"][0]) <= 0.05 and abs(res[0]["y"] - case["truth"][1]) <= 0.05
    gd.close(); gh.close()


def test_one_member_and_sixty_four(world):
    """m = 1; m = 64 with one stack repeated: the last Ctrl, the last frontier segment, blockIdx.y = 63.  Member 63 has a guess of
    its own, so that a stride error cannot hide behind equal members."""
    case = BASE[0]
    gd, gh, stacks = world.groups([0])
    res1, _, best = same_groups(gd, gh, [case["guess"]], case["points"], singles=stacks, **gc.windows(case))
    assert best == 0
    gd.close(); gh.close()
    gd, gh, stacks = world.groups([0] * 64)
    guesses = [case["guess"]] * 63 + [BASE[3]["guess"]]
    res, status, best = same_groups(gd, gh, guesses, case["points"], **gc.windows(case))
    assert status == [abi.OK] * 64 and best == gc.argmax_lowest(res, status)
    assert all(r == res1[0] for r in res[:63]) and res[63] != res1[0]
    rc, r, hk = gc.single_call(stacks[63], guesses[63], case["points"], **gc.windows(case))
    assert rc == abi.OK
    cases.same_record(res[63], r)
    cases.same_hook(gd.match_download(63), hk)
    cases.same_hook(gd.match_download(62), gd.match_download(0))
    gd.close(); gh.close()


@pytest.mark.parametrize("name", ["n1", "n63", "n65", "n1025"])
def test_point_counts_about_a_wavefront_and_a_workgroup(world, name):
    """The boundaries of the lane loops, with member offsets: two different sub-maps, two different guesses."""
    case = EDGE[name]
    gd, gh, stacks = world.groups([0, 1])
    res, status, best = same_groups(gd, gh, [case["guess"], BASE[1]["guess"]], case["points"], singles=stacks, **gc.windows(case))
    assert status == [abi.OK] * 2 and gd.match_download(1)["n"] == int(name[1:])
    gd.close(); gh.close()


@pytest.mark.parametrize("depth,per", [(3, 16), (1, 169)])
def test_clipped_children_and_a_single_level(world, depth, per):
    """depth 3: L = 13, H = 2, the last children clipped; depth 1: H = 0, the top-level kernels alone."""
    case = BASE[1]
    gd, gh, stacks = world.groups([0, 1], depth)
    res, status, best = same_groups(gd, gh, [BASE[0]["guess"], case["guess"]], case["points"], singles=stacks, **gc.windows(case))
    assert all(r["depth_used"] == depth for r in res) and gd.match_download(1)["bounds"].shape[1] == per
    gd.close(); gh.close()


@pytest.mark.parametrize("which,capacity,level", gc.OVERFLOWS, ids=["keep_step", "level_sweep"])
def test_one_member_overflows_and_its_neighbours_do_not_notice(world, which, capacity, level):
    """The member after the truncated one has a known survivor list: it equals its single call, so nothing was written into its
    segment."""
    over = cases.overflow_case()
    gd, gh, stacks = world.groups([0, 0, 0])
    good = BASE[which]["guess"]
    kw = gc.windows(over, frontier_capacity=capacity)
    rc, r_good, hk_good = gc.single_call(stacks[0], good, over["points"], **kw)
    assert rc == abi.OK and max(hk_good["kept"]) <= capacity
    res, status, best = same_groups(gd, gh, [good, over["guess"], good], over["points"], **kw)
    assert status == [abi.OK, abi.ERR_UNSUPPORTED, abi.OK] and best == 0
    assert gd.last_error() == f"member 1: frontier overflow at level {level}: more than {capacity} nodes kept"
    for i in (0, 2):
        cases.same_record(res[i], r_good)
        cases.same_hook(gd.match_download(i), hk_good)
    cases.same_hook(stacks[0].match_download(), hk_good)                   # the member's own hook data: its single call's
    res, status, best = same_groups(gd, gh, [good, over["guess"], good], over["points"], singles=stacks, **gc.windows(over))
    assert status == [abi.OK] * 3 and gd.last_error() == "" and res[1]["sum"] == 0
    gd.close(); gh.close()


def test_a_window_beyond_the_exhaustive_limits(world):
    """nl = 40: L = 81, H = 6, four top nodes per scan."""
    case = cases.wide_case()
    gd, gh, stacks = world.groups([0, 1])
    res, status, best = same_groups(gd, gh, [case["guess"], BASE[4]["guess"]], case["points"], singles=stacks, **gc.windows(case))
    assert all((r["num_linear"], r["depth_used"]) == (40, 7) for r in res) and gd.match_download(0)["bounds"].shape[1] == 4
    gd.close(); gh.close()


def test_launches_and_waits_do_not_grow_with_the_members(world):
    case = BASE[0]
    for members in ([0], [0, 1, 2], [0, 1] * 32):
        gd, gh, stacks = world.groups(members)
        assert gd.last_counts() == ZERO
        res, status, best = gd.match(case["guess"], case["points"], **gc.windows(case))
        assert gd.rc == abi.OK and status == [abi.OK] * len(members)
        H = res[0]["depth_used"] - 1
        assert H == 4 and gd.last_counts() == dict(kernel_launches=H + 5, copies_and_memsets=2, synchronisations=1)    # one upload, one download
        gd.match(case["guess"], np.zeros((0, 3)), **gc.windows(case))
        assert gd.last_counts() == ZERO                                    # n = 0: nothing issued
        gd.close(); gh.close()


def test_a_single_call_between_two_group_calls(world):
    case, other = BASE[0], BASE[3]
    gd, gh, stacks = world.groups([0, 1, 2])
    guesses = [BASE[0]["guess"], BASE[1]["guess"], BASE[2]["guess"]]
    res0, status0, best0 = same_groups(gd, gh, guesses, case["points"], **gc.windows(case))
    hooks0 = [gd.match_download(i) for i in range(3)]
    rc, r_single, hk_single = gc.single_call(stacks[1], other["guess"], other["points"], **gc.windows(other))
    assert rc == abi.OK
    for i in range(3):
        cases.same_hook(gd.match_download(i), hooks0[i])
    res1, status1, best1 = gd.match(guesses, case["points"], **gc.windows(case))
    assert (status1, best1) == (status0, best0)
    for i in range(3):
        cases.same_record(res1[i], res0[i])
        cases.same_hook(gd.match_download(i), hooks0[i])
    cases.same_hook(stacks[1].match_download(), hk_single)                 # the member's own hook still holds its single call
    # a refused call changes nothing on the device either
    assert gd.match(guesses, case["points"], frontier_capacity=1 << 25, **gc.windows(case)) == (None, None, None) and gd.rc == abi.ERR_UNSUPPORTED
    for i in range(3):
        cases.same_hook(gd.match_download(i), hooks0[i])
    gd.close(); gh.close()


def fresh_pair(world, member=0):
    """A (device stack, host stack) of its own on a member sub-map: the caller closes both."""
    dev, host, index = world.subs[member]
    out = []
    for sub in (dev, host):
        st = sub.freeze(index, cases.DEPTH)
        assert st.status == abi.OK, sub.last_error()
        out.append(st)
    return out


def single_equals_the_twin(sd, sh, case):
    rc, r, hk = gc.single_call(sd, case["guess"], case["points"], **gc.windows(case))
    assert rc == abi.OK, sd.last_error()
    rc, rt, hkt = gc.single_call(sh, case["guess"], case["points"], **gc.windows(case))
    assert rc == abi.OK, sh.last_error()
    cases.same_record(r, rt)
    cases.same_hook(hk, hkt)
    return r, hk


def test_a_single_call_after_its_group_is_gone(world):
    """The stack's single calls run on its own block: the group's buffers going takes nothing from under them."""
    case, other = BASE[0], BASE[3]
    sd, sh = fresh_pair(world)
    gd, gh = sg.ScanStackGroup([sd]), sg.ScanStackGroup([sh])
    assert gd.status == gh.status == abi.OK, sg.create_error()
    same_groups(gd, gh, [case["guess"]], case["points"], **gc.windows(case))
    gd.close(); gh.close()
    single_equals_the_twin(sd, sh, other)
    cases.same_hook(sd.match_download(), sh.match_download())
    sd.close(); sh.close()


def test_a_stack_closed_before_its_group(world):
    """A single call, a group call, then the stack goes first: the group is only closed afterwards, never used.  The stack's and
    the group's blocks are apart, so each is freed once."""
    case, other = BASE[0], BASE[3]
    sd, sh = fresh_pair(world)
    gd, gh = sg.ScanStackGroup([sd]), sg.ScanStackGroup([sh])
    assert gd.status == gh.status == abi.OK, sg.create_error()
    r, hk = single_equals_the_twin(sd, sh, other)
    res, status, best = same_groups(gd, gh, [case["guess"]], case["points"], **gc.windows(case))
    assert status == [abi.OK] and res[0] != r
    cases.same_hook(sd.match_download(), hk)                               # the group call left the stack's own hook
    sd.close(); sh.close()
    gd.close(); gh.close()
