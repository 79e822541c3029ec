"""The pose guess inside the resident front end (include/visfs_tracker_pnp.h) on the CPU: the host twin of
visfs_tracker_process with the pose guess enabled against the checker of tracker_pnp_oracle.py, which runs the staged
visfs_pnp_solve behind each staged frame: every output array, flag and intermediate list, the pose guess's among them, frame by
frame, byte for byte."""
import numpy as np
import pytest

import group_cases as gc
import tracker_cases as tc
import tracker_cull_cases as cc
import tracker_oracle as to
import tracker_pnp_cases as pc
import tracker_pnp_oracle as tpo
from visfs_amd import abi, backend, flow, pnp, tracker, tracker_pnp


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_host_twin_equals_the_checker(name):
    scn = pc.CASES[name]()
    ref, sub = pc.checker(scn), pc.Subject(scn)
    try:
        log = pc.lockstep(scn, ref, [sub], name)
    finally:
        ref.close(); sub.close()
    print(name, pc.summary(log))
    pc.assert_conditions(name, scn, log)


def test_rows_reach_the_wavefront_edges():
    """Over the edge cases the number of rows that enter the pose guess takes the values on both sides of a wavefront."""
    seen = set()
    for mf in pc.EDGE_FEATURES:
        _, log = pc.host_log(f"edge_mf{mf}_it{pc.EDGE_ITERATIONS[0]}")
        seen |= {i["pnp"]["m"] for _, i in log if i is not None}
    print(sorted(seen))
    assert {63, 64, 65} <= seen, sorted(seen)


def test_abi_versions():
    assert tracker.load().visfs_tracker_abi_version() == tracker.ABI_VERSION == 2
    assert tracker_pnp.load().visfs_tracker_pnp_abi_version() == tracker_pnp.ABI_VERSION == 1


def _plain_against(scn, sub):
    """The subject against tracker_cases.Subject, the tracker as it was, with an inactive pose guess in every call."""
    plain = tc.Subject(scn)
    try:
        for k, (left, right) in enumerate(scn["frames"]):
            want, got = plain.process(left, right), sub.process(left, right)
            gc.same(got, want, f"frame {k}")
            tpo.assert_same_pose(got[0]["pose"], tpo.not_ran(), f"frame {k}")
            if got[1] is not None:
                tpo.assert_same_hook(got[1]["pnp"], tpo.inactive(), f"frame {k}")
    finally:
        plain.close()


def test_never_enabled_is_the_tracker_without_it():
    scn = pc.steady()
    sub = pc.Subject(scn, enable=False)
    try:
        _plain_against(scn, sub)
    finally:
        sub.close()


def test_enabled_then_disabled_is_the_tracker_without_it():
    scn = pc.steady()
    sub = pc.Subject(scn)
    try:
        tracker_pnp.enable(sub.trk, None)
        _plain_against(scn, sub)
    finally:
        sub.close()


def test_disabling_in_the_middle_leaves_the_tracker_alone():
    """The pose guess on for three frames, off for the rest: the tracker's own outputs are those of the tracker without it all along,
    and the pose follows the switch."""
    scn = pc.steady()
    _, log = pc.host_log("steady")
    sub = pc.Subject(scn)
    try:
        for k, (left, right) in enumerate(scn["frames"]):
            if k == 3:
                tracker_pnp.enable(sub.trk, None)
            got = sub.process(left, right)
            gc.same(got, log[k], f"frame {k}")
            tpo.assert_same_pose(got[0]["pose"], log[k][0]["pose"] if k < 3 else tpo.not_ran(), f"frame {k}")
    finally:
        sub.close()


def test_host_group_equals_host_singles():
    members, log, boots = pc.rig_reference()
    sub = pc.Rig(members)
    try:
        pc.rig_against(members, log, sub, "host group")
        assert all(c == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0) for c in sub.counts)
    finally:
        sub.close()
    assert any(any(row) for row in boots[2:]) and not all(any(row) for row in boots)


def test_rig_singles_equal_the_checker():
    """Member 1 of the rig (the foreign frames behind the cull, lost and bootstrapped inside the run) against the staged chain."""
    members, log, _ = pc.rig_reference()
    m = members[1]
    scn = pc.with_pnp(cc.scenario(m["frames"], cc.RIG_FEATURES, cc.RIG_MIN_INLIERS, cc.RIG_ITERATIONS), **pc.RIG_PNP)
    ref = pc.checker(scn)
    try:
        for k, (left, right) in enumerate(m["frames"]):
            want = ref.process(left, right)
            pc.same(log[k][1], want, f"call {k}")
    finally:
        ref.close()


def _tracker(f, **kw):
    return tracker.Tracker(f, flow.camera(), tracker.default_params(max_features=60, min_distance=12, **kw))


def test_enable_refusals():
    f = flow.Flow(flow.default_params(), 320, 240)
    t = _tracker(f)
    try:
        bad = [dict(iterations=0), dict(refine_iterations=-1), dict(reproj_error=float("nan")), dict(reproj_error=-1.0),
               dict(refine_sigma=float("inf")), dict(refine_sigma=-0.5)]
        for kw in bad:
            assert tracker_pnp.enable_status(t, pnp.default_params(**kw)) == abi.ERR_BAD_ARGUMENT, kw
            assert t.last_error(), kw
        assert "iterations" in t.last_error() or "threshold" in t.last_error()
        for kw in (dict(iterations=4097), dict(refine_iterations=33)):
            assert tracker_pnp.enable_status(t, pnp.default_params(**kw)) == abi.ERR_UNSUPPORTED, kw
        for kw in (dict(iterations=4096, refine_iterations=32), dict(iterations=1, refine_iterations=0, min_inliers=-3)):
            assert tracker_pnp.enable_status(t, pnp.default_params(**kw)) == abi.OK, kw
        assert tracker_pnp.enable_status(t, None) == abi.OK
    finally:
        t.close(); f.close()


def test_enabling_inside_a_group_is_refused():
    flows = [flow.Flow(flow.default_params(), 320, 240) for _ in range(2)]
    trks = [_tracker(f) for f in flows]
    try:
        tracker_pnp.enable(trks[0], pnp.default_params())
        tracker_pnp.enable(trks[1], pnp.default_params())
        g = tracker.TrackerGroup(trks)
        assert tracker_pnp.enable_status(trks[0], pnp.default_params(iterations=10)) == abi.ERR_BAD_ARGUMENT
        assert "group" in trks[0].last_error()
        assert tracker_pnp.enable_status(trks[1], None) == abi.ERR_BAD_ARGUMENT
        g.close()
        assert tracker_pnp.enable_status(trks[1], None) == abi.OK              # free again once the group is gone
    finally:
        for t in trks:
            t.close()
        for f in flows:
            f.close()


def test_group_members_must_agree_on_the_pose_guess():
    flows = [flow.Flow(flow.default_params(), 320, 240) for _ in range(2)]

    def pair(a, b):
        trks = [_tracker(f) for f in flows]
        for t, kw in zip(trks, (a, b)):
            if kw is not None:
                tracker_pnp.enable(t, pnp.default_params(**kw))
        rc, h, why = tracker.group_create_status(trks)
        if h is not None:
            tracker.load().visfs_tracker_group_destroy(h)
        for t in trks:
            t.close()
        return rc, why

    try:
        base = dict(iterations=64)
        assert pair(base, base)[0] == abi.OK
        assert pair(None, None)[0] == abi.OK
        for other in (None, dict(iterations=65), dict(iterations=64, min_inliers=13), dict(iterations=64, reproj_error=1.5),
                      dict(iterations=64, refine_iterations=4), dict(iterations=64, refine_sigma=2.0), dict(iterations=64, seed=1)):
            rc, why = pair(base, other)
            assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in why and "pose guess" in why, (other, rc, why)
        rc, why = pair(None, base)
        assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in why
    finally:
        for f in flows:
            f.close()


def test_last_before_the_first_call_is_refused():
    scn = pc.steady()
    sub = pc.Subject(scn)
    try:
        assert tracker_pnp.last_status(sub.trk)[0] == abi.ERR_NOT_LOADED
        with pytest.raises(backend.BackendError, match=f"status {abi.ERR_NOT_LOADED}: no call to report on"):
            tracker_pnp.download(sub.trk)
        out, inter = sub.process(*scn["frames"][0])
        assert out["flags"] == to.NO_PREVIOUS and inter is None
        tpo.assert_same_pose(out["pose"], tpo.not_ran())
        out, inter = sub.process(*scn["frames"][1])
        assert out["pose"]["ran"] == 1 and out["pose"]["T"].any() and inter["pnp"]["m"] == len(out["pose"]["matches"])
        assert np.array_equal(out["pose"]["T"][3], [0.0, 0.0, 0.0, 1.0])
    finally:
        sub.close()
