"""Tracker groups on the GPU (include/visfs_tracker_group.h): a device group against the host twins called singly, byte for byte in
every output array, flag and intermediate list (visfs_tracker_download of every member) after every call; against the same members
called singly on the device; and what a call issues: at most two synchronisations, and kernel launches that do not grow with the
number of members."""
import pytest

import group_cases as gc
import tracker_cases as tc
import tracker_oracle as to
from visfs_amd import abi, backend, flow, synth, tracker

pytestmark = pytest.mark.gpu


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _syncs_ok(rig):
    assert rig.counts and all(c["synchronisations"] <= 2 and c["kernel_launches"] > 0 for c in rig.counts), rig.counts


def _host_log(members, max_features, **kw):
    ref = gc.Rig(members, max_features, **kw)
    try:
        return gc.reference_log(members, ref)
    finally:
        ref.close()


@pytest.mark.parametrize("max_features", [60, 65])
def test_mixed_states_equal_the_host_twins(solver, max_features):
    members, log = gc.mixed_reference(max_features)
    dev = gc.Rig(members, max_features, solver=solver)
    try:
        gc.against(members, log, dev, f"mixed, {max_features}")
        _syncs_ok(dev)
    finally:
        dev.close()


def test_mixed_states_with_clahe_and_without_the_reverse_pass(solver):
    members, log = gc.mixed_reference(60, True, 0)
    dev = gc.Rig(members, 60, clahe_on=True, solver=solver, flow_back=0)
    try:
        gc.against(members, log, dev, "mixed, CLAHE")
        _syncs_ok(dev)
    finally:
        dev.close()


def test_staggered_members(solver):
    members = gc.staggered_three()
    log = _host_log(members, 60)
    assert gc.flags(log, 0) == [0, 0, to.NO_PREVIOUS] and gc.flags(log, 1) == [0, 0, to.BOOTSTRAPPED]
    dev = gc.Rig(members, 60, solver=solver)
    try:
        gc.against(members, log, dev, "staggered")
        _syncs_ok(dev)
    finally:
        dev.close()


def _group_of_one():
    members, log = gc.mixed_reference(60)
    return members[:1], [call[:1] for call in log]


def test_group_of_one(solver):
    members, log = _group_of_one()
    dev = gc.Rig(members, 60, solver=solver)
    try:
        gc.against(members, log, dev, "one")
        _syncs_ok(dev)
    finally:
        dev.close()


def test_group_of_nine_with_two_cameras(solver):
    members = gc.nine()
    log = _host_log(members, 60)
    assert gc.flags(log, 2) == [0] * 9
    dev = gc.Rig(members, 60, solver=solver)
    try:
        gc.against(members, log, dev, "nine")
        _syncs_ok(dev)
    finally:
        dev.close()


def _two_with_full_outlier_lists():
    rules = [None, None, tc.full_outlier_list, None]
    return [gc.member(tc.sequence(8)[:4], outliers=rules), gc.member(gc.seeded(8, 11)[:4], outliers=rules)]


def test_full_length_outlier_lists_of_both_members(solver):
    """Both members send 4096 ids: member 1's list starts at the very end of member 0's share of the upload block."""
    members = _two_with_full_outlier_lists()
    log = _host_log(members, 60)
    assert all(len(tc.full_outlier_list(log[1][i][0])) == tracker.MAX_OUTLIERS for i in range(2))
    assert gc.flags(log, 2) == [0, 0] and all(log[2][i][0]["blocked_id"].tolist() == tc.every_third(log[1][i][0]) for i in range(2))
    dev = gc.Rig(members, 60, solver=solver)
    try:
        gc.against(members, log, dev, "4096 outliers each")
        _syncs_ok(dev)
    finally:
        dev.close()


def test_a_member_goes_before_its_group_and_its_flow_object(solver):
    members = gc.staggered_three(2)[:2]
    dev = gc.Rig(members, 60, solver=solver)
    for i, m in enumerate(members):
        for pair in m["pre"]:
            dev.single(i, *pair)
    dev.grouped(gc.call_args(members, 0, [None] * 2))
    dev.single(0, *members[0]["frames"][1])
    dev.trks[0].close()
    dev.group.close()
    dev.flows[0].close()
    dev.flows[1].close()                       # member 1: the flow object first, then the orphaned tracker
    rc, _ = dev.trks[1].process_status(*members[1]["frames"][1])
    assert rc == abi.ERR_NOT_LOADED and "the flow object of this tracker is gone" in dev.trks[1].last_error()
    dev.trks[1].close()


def test_single_calls_between_group_calls(solver):
    """Call 3 of every member is made singly between grouped calls; then member 0 alone runs a frame ahead by a single call."""
    members, log = gc.mixed_reference(60)
    dev = gc.Rig(members, 60, solver=solver)
    try:
        prev = [None] * 4
        for k, want in enumerate(log):
            args = gc.call_args(members, k, prev)
            got = [dev.single(i, *a) for i, a in enumerate(args)] if k == 3 else dev.grouped(args)
            for i in range(4):
                gc.same(got[i], want[i], f"call {k}, member {i}")
            prev = [w[0] for w in want]
    finally:
        dev.close()
    a, b = tc.sequence(8), gc.seeded(8, 11)
    ahead = [gc.member([a[0], a[1], a[3], a[4]]), gc.member(b[:4])]
    ref, dev = gc.Rig(ahead, 60), gc.Rig(ahead, 60, solver=solver)
    try:
        prev = [None, None]
        for k in range(4):
            if k == 2:
                gc.same(dev.single(0, *a[2]), ref.single(0, *a[2]), "the single call")
            args = gc.call_args(ahead, k, prev)
            want, got = [ref.single(i, *x) for i, x in enumerate(args)], dev.grouped(args)
            for i in range(2):
                gc.same(got[i], want[i], f"ahead: call {k}, member {i}")
            prev = [w[0] for w in want]
    finally:
        ref.close(); dev.close()


def test_ba_between_group_calls_returns_the_same_bytes(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    members, log = gc.mixed_reference(60)
    dev = gc.Rig(members, 60, solver=solver)

    def solve(k):
        rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
        assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
        assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()

    try:
        gc.against(members, log, dev, "BA between", between=solve)
        solve(6)
    finally:
        dev.close()


def test_device_group_equals_the_members_called_singly_on_the_device(solver):
    members, _ = gc.mixed_reference(60)
    singly, dev = gc.Rig(members, 60, solver=solver), gc.Rig(members, 60, solver=solver)
    try:
        log = gc.reference_log(members, singly)
        gc.assert_mixed_conditions(log)
        gc.against(members, log, dev, "device singly")
    finally:
        singly.close(); dev.close()


def _launches(members, log, solver):
    dev = gc.Rig(members, 60, solver=solver)
    try:
        gc.against(members, log, dev, "counts")
        _syncs_ok(dev)
        return [c["kernel_launches"] for c in dev.counts]
    finally:
        dev.close()


def test_kernel_launches_do_not_grow_with_the_members(solver):
    members, log = gc.mixed_reference(60)
    four = _launches(members, log, solver)
    one = _launches(*_group_of_one(), solver)
    many = gc.nine()
    nine = _launches(many, _host_log(many, 60), solver)
    print("kernel launches per call: one", one, "four", four, "nine", nine)
    assert four[2] == one[2]                   # a steady frame
    assert four[4] == one[1]                   # one member of four bootstraps: the launches of a bootstrap, once
    assert nine[2] == one[2]
    assert one[1] > one[2] > one[0] > 0        # the bootstrap branch is extra; a first frame is the push alone


def test_mixed_host_and_device_members_are_refused(solver):
    fh, fd = flow.Flow(flow.default_params(), gc.W, gc.H), flow.Flow(flow.default_params(), gc.W, gc.H, solver=solver)
    p = tracker.default_params(max_features=60, min_distance=12, min_inliers=30)
    th, td = tracker.Tracker(fh, flow.camera(), p), tracker.Tracker(fd, flow.camera(), p)
    rc, _, why = tracker.group_create_status([td, th])
    assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in why and "host-twin" in why
    for x in (th, td, fh, fd):
        x.close()


def test_process_refusals_on_the_device_change_no_member(solver):
    members = gc.staggered_three(3)
    log = _host_log(members, 60)
    dev = gc.Rig(members, 60, solver=solver)
    try:
        prev = [None] * 3
        for i, m in enumerate(members):
            for pair in m["pre"]:
                dev.single(i, *pair)
        got = dev.grouped(gc.call_args(members, 0, prev))
        for i in range(3):
            gc.same(got[i], log[0][i], f"call 0, member {i}")
        args = gc.call_args(members, 1, prev)
        g = dev.group
        bad = list(args)
        bad[2] = (None, args[2][1])
        assert g.process_status(bad)[0] == abi.ERR_BAD_ARGUMENT and "member 2" in g.last_error()
        bad = list(args)
        bad[1] = (args[1][0], args[1][1], None, [1], 4097)
        assert g.process_status(bad)[0] == abi.ERR_BAD_ARGUMENT and "member 1" in g.last_error()
        assert g.last_counts() == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0)
        got = dev.grouped(args)
        for i in range(3):
            gc.same(got[i], log[1][i], f"call 1, member {i}")
        dev.flows[0].push_frame(*members[0]["frames"][2])
        args = gc.call_args(members, 2, prev)
        assert g.process_status(args)[0] == abi.ERR_NOT_LOADED and "member 0" in g.last_error()
        for i in (1, 2):
            gc.same(dev.single(i, *args[i]), log[2][i], f"call 2, member {i}")
        dev.trks[1].close()
        assert g.process_status(args)[0] == abi.ERR_NOT_LOADED
    finally:
        dev.close()
