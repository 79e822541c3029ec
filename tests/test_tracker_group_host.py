"""Tracker groups (include/visfs_tracker_group.h) on the CPU: a group of host-twin trackers against the same host twins called singly,
byte for byte in every output array, flag and intermediate list after every call; the refusals of create and process.  (A list that
mixes host-twin and device trackers needs a device: tests/test_gpu_tracker_group.py has that refusal.)"""
import numpy as np
import pytest

import group_cases as gc
import tracker_cases as tc
import tracker_oracle as to
from visfs_amd import abi, flow, tracker


def _pair(members, max_features, **kw):
    return gc.Rig(members, max_features, **kw), gc.Rig(members, max_features, **kw)


def test_mixed_states_equal_the_members_called_singly():
    members, log = gc.mixed_reference(60)
    print([gc.flags(log, k) for k in range(6)], [gc.from_rows(log, k) for k in range(1, 6)])
    assert gc.flags(log, 0) == [to.NO_PREVIOUS] * 4 and gc.flags(log, 1) == [to.BOOTSTRAPPED] * 4
    sub = gc.Rig(members, 60)
    try:
        gc.against(members, log, sub, "mixed")
        assert all(c == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0) for c in sub.counts) and len(sub.counts) == 6
    finally:
        sub.close()


def test_staggered_members():
    members = gc.staggered_three()
    ref, sub = _pair(members, 60)
    try:
        log = gc.reference_log(members, ref)
        assert gc.flags(log, 0) == [0, 0, to.NO_PREVIOUS] and gc.flags(log, 1) == [0, 0, to.BOOTSTRAPPED]
        gc.against(members, log, sub, "staggered")
    finally:
        ref.close(); sub.close()


def test_single_call_on_a_member_between_group_calls():
    """Calls 0-2 grouped, call 3 of member 1 single and of the others grouped one member at a time is not possible: a group call takes
    every member.  So the whole of call 3 is made singly, and calls 4 and 5 grouped again."""
    members, log = gc.mixed_reference(60)
    sub = gc.Rig(members, 60)
    try:
        prev = [None] * 4
        for k, want in enumerate(log):
            args = gc.call_args(members, k, prev)
            got = [sub.single(i, *a) for i, a in enumerate(args)] if k == 3 else sub.grouped(args)
            for i in range(4):
                gc.same(got[i], want[i], f"call {k}, member {i}")
            prev = [w[0] for w in want]
    finally:
        sub.close()


def test_one_member_runs_ahead_by_a_single_call():
    """Member 0 alone gets a single call between two group calls: it is one frame ahead of its group from then on."""
    a, b = tc.sequence(8), gc.seeded(8, 11)
    ahead = [gc.member([a[0], a[1], a[3], a[4]]), gc.member(b[:4])]
    ref, sub = _pair(ahead, 60)
    try:
        prev = [None, None]
        for k in range(4):
            if k == 2:
                want0, got0 = ref.single(0, *a[2]), sub.single(0, *a[2])
                gc.same(got0, want0, "the single call")
            args = gc.call_args(ahead, k, prev)
            want = [ref.single(i, *x) for i, x in enumerate(args)]
            got = sub.grouped(args)
            for i in range(2):
                gc.same(got[i], want[i], f"call {k}, member {i}")
            prev = [w[0] for w in want]
        assert want[0][0]["flags"] == 0 and want[1][0]["flags"] == 0
    finally:
        ref.close(); sub.close()


def _tracker(width=gc.W, height=gc.H, flow_kw=None, **kw):
    f = flow.Flow(flow.default_params(**(flow_kw or {})), width, height)
    p = dict(max_features=60, min_distance=12, min_inliers=30)
    p.update(kw)
    return f, tracker.Tracker(f, flow.camera(), tracker.default_params(**p))


def test_create_refusals_name_the_member():
    made = [_tracker() for _ in range(3)]
    trks = [t for _, t in made]
    rc, _, why = tracker.group_create_status([])
    assert rc == abi.ERR_UNSUPPORTED and "1 .. 64" in why
    many = [_tracker() for _ in range(65)]
    rc, _, why = tracker.group_create_status([t for _, t in many])
    assert rc == abi.ERR_UNSUPPORTED and "1 .. 64" in why
    rc, h, _ = tracker.group_create_status([t for _, t in many[:64]])                 # the largest group there is
    assert rc == abi.OK
    tracker.load().visfs_tracker_group_destroy(h)
    second = tracker.Tracker(made[1][0], flow.camera(), tracker.default_params(max_features=60, min_distance=12, min_inliers=30))
    rc, _, why = tracker.group_create_status([trks[0], trks[1], second])
    assert rc == abi.ERR_BAD_ARGUMENT and "member 2" in why and "flow object" in why
    for kw, word in ((dict(max_features=61), "tracker parameters"), (dict(flow_kw=dict(flow_back=0)), "flow parameters"),
                     (dict(width=328), "image size"), (dict(clahe=1), "tracker parameters")):
        f, t = _tracker(**kw)
        rc, _, why = tracker.group_create_status([trks[0], t, trks[2]])
        assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in why and word in why, (kw, why)
        t.close(); f.close()
    g = tracker.TrackerGroup(trks[:2])
    rc, _, why = tracker.group_create_status([trks[2], trks[1]])
    assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in why and "group already" in why
    g.close()
    g = tracker.TrackerGroup([trks[2], trks[1]])                                      # a closed group frees its members
    g.close()
    second.close()
    for f, t in made + many:
        t.close(); f.close()


def test_process_refusals_change_no_member():
    members = gc.staggered_three(3)
    ref, sub = _pair(members, 60)
    try:
        log = gc.reference_log(members, ref)
        prev = [None] * 3
        for i, m in enumerate(members):
            for pair in m["pre"]:
                sub.single(i, *pair)
        first = gc.call_args(members, 0, prev)
        got = sub.grouped(first)
        for i in range(3):
            gc.same(got[i], log[0][i], f"call 0, member {i}")
        args = gc.call_args(members, 1, prev)
        g = sub.group
        bad = list(args)
        bad[2] = (None, args[2][1])
        rc, _ = g.process_status(bad)
        assert rc == abi.ERR_BAD_ARGUMENT and "member 2" in g.last_error() and "NULL" in g.last_error()
        bad = list(args)
        bad[1] = (args[1][0], args[1][1], None, [1], 4097)
        rc, _ = g.process_status(bad)
        assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in g.last_error() and "n_outliers" in g.last_error()
        got = sub.grouped(args)                                                       # the refused calls pushed and changed nothing
        for i in range(3):
            gc.same(got[i], log[1][i], f"call 1, member {i}")
        # a foreign push on member 0's flow: refused, and the other members' next results are what they would have been
        sub.flows[0].push_frame(*members[0]["frames"][2])
        args = gc.call_args(members, 2, prev)
        rc, _ = g.process_status(args)
        assert rc == abi.ERR_NOT_LOADED and "member 0" in g.last_error() and "pushed" in g.last_error()
        for i in (1, 2):
            gc.same(sub.single(i, *args[i]), log[2][i], f"call 2, member {i}")
    finally:
        ref.close(); sub.close()


def test_a_destroyed_member_is_refused():
    members = gc.staggered_three(2)
    sub = gc.Rig(members, 60)
    try:
        args = gc.call_args(members, 0, [None] * 3)
        sub.grouped(args)
        sub.trks[1].close()
        rc, _ = sub.group.process_status(gc.call_args(members, 1, [None] * 3))
        assert rc == abi.ERR_NOT_LOADED and "member 1" in sub.group.last_error()
    finally:
        sub.close()
    sub = gc.Rig(members, 60)
    try:
        sub.grouped(args)
        sub.flows[2].close()                                                          # the flow object goes, the tracker stays
        rc, _ = sub.group.process_status(gc.call_args(members, 1, [None] * 3))
        assert rc == abi.ERR_NOT_LOADED and "member 2" in sub.group.last_error()
    finally:
        sub.close()


def test_a_member_goes_before_its_group_and_its_flow_object():
    members = gc.staggered_three(2)[:2]
    sub = gc.Rig(members, 60)
    for i, m in enumerate(members):
        for pair in m["pre"]:
            sub.single(i, *pair)
    sub.grouped(gc.call_args(members, 0, [None] * 2))
    sub.single(0, *members[0]["frames"][1])
    sub.trks[0].close()
    sub.group.close()
    sub.flows[0].close()
    sub.flows[1].close()                       # member 1: the flow object first, then the orphaned tracker
    rc, _ = sub.trks[1].process_status(*members[1]["frames"][1])
    assert rc == abi.ERR_NOT_LOADED and "the flow object of this tracker is gone" in sub.trks[1].last_error()
    sub.trks[1].close()
