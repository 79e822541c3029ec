"""Tracker/CullByFundationMatrix inside the resident front end (include/visfs_tracker.h ABI 2) on the CPU: the
host twin of visfs_tracker_process against the checker of tracker_cull_oracle.py, which runs the staged visfs_fund_cull behind the
staged track: every output array, flag and intermediate list, the cull's among them, frame by frame, byte for byte."""
import numpy as np
import pytest

import group_cases as gc
import tracker_cases as tc
import tracker_cull_cases as cc
import tracker_cull_oracle as tco
import tracker_oracle as to
from visfs_amd import abi, backend, flow, fund, tracker


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_host_twin_equals_the_checker(name):
    scn = cc.CASES[name]()
    ref, sub = cc.checker(scn), cc.Subject(scn)
    try:
        log = cc.lockstep(scn, ref, [sub], name)
    finally:
        ref.close(); sub.close()
    print(name, [(r["flags"], None if i is None else (cc.before_and_after(i), i["cull"]["m"], i["cull"]["n_hypotheses"])) for r, i in log])
    cc.assert_conditions(name, scn, log)
    if name == "foreign":                             # every sample of every frame gave a model: the search is a search
        assert all(i["cull"]["n_valid_samples"] == 64 for _, i in log[1:])


def test_abi_version_and_defaults():
    assert tracker.load().visfs_tracker_abi_version() == tracker.ABI_VERSION == 2
    p = tracker.default_params()
    assert p.cull == 0 and p.cull_params.pixel_error == 1.0 and p.cull_params.iterations == 1000 and p.cull_params.seed == 0


def test_cull_is_ignored_with_the_reverse_pass():
    """cull = 1 with flow_back = 1 is cull = 0 byte for byte, and the hook reports an inactive cull."""
    on = cc.scenario(tc.sequence(6), 60, 10, 64, flow_back=1)
    off = cc.scenario(tc.sequence(6), 60, 10, 64, flow_back=1, cull=0)
    a, b = cc.Subject(on), cc.Subject(off)
    try:
        log = cc.lockstep(on, b, [a], "ignored")
    finally:
        a.close(); b.close()
    assert log[2][1]["cull"]["applied"] == 0 and log[2][1]["cull"]["m"] == 0 and len(log[2][1]["cull"]["status"]) == 0
    plain = tc.Subject(tc.scenario(tc.sequence(6), 60, 12, flow_back=1))             # the parameters of before ABI 2
    try:
        for k, (left, right) in enumerate(on["frames"]):
            gc.same(plain.process(left, right), log[k], f"plain frame {k}")
    finally:
        plain.close()


def test_cull_off_is_the_tracker_without_it():
    """flow_back = 0 and cull = 0: the results of the checker without a cull, and an inactive hook."""
    scn = cc.scenario(tc.sequence(5), 60, 10, 64, cull=0)
    ref, sub = tc.checker(scn), cc.Subject(scn)
    try:
        for k, (left, right) in enumerate(scn["frames"]):
            want, got = ref.process(left, right), sub.process(left, right)
            gc.same(got, want, f"frame {k}")
            if got[1] is not None:
                tco.assert_same_cull(got[1]["cull"], tco.inactive(), f"frame {k}")
    finally:
        ref.close(); sub.close()


def test_pixel_error_zero_means_three():
    frames = cc.foreign_sequence()[:6]
    zero, three = cc.scenario(frames, 60, 10, 64, pixel_error=0.0), cc.scenario(frames, 60, 10, 64, pixel_error=3.0)
    a, b = cc.Subject(zero), cc.Subject(three)
    try:
        log = cc.lockstep(zero, b, [a], "pixel_error 0")
    finally:
        a.close(); b.close()
    one = cc.host_log("foreign")[1]
    assert any(log[k][1]["cull"]["n_inliers"] > one[k][1]["cull"]["n_inliers"] for k in range(3, 6))      # and 3 px is not 1 px


def test_host_group_equals_host_singles():
    members, log, boots = cc.rig_reference()
    sub = cc.Rig(members)
    try:
        cc.rig_against(members, log, sub, "host group")
        assert all(c == dict(kernel_launches=0, copies_and_memsets=0, synchronisations=0) for c in sub.counts)
    finally:
        sub.close()
    assert any(any(row) for row in boots[2:]) and not all(any(row) for row in boots)


def _create(f, **kw):
    cull_params = fund.default_params(**{k: kw.pop(k) for k in ("iterations", "pixel_error", "seed") if k in kw})
    return tracker.create_status(f, flow.camera(), tracker.default_params(max_features=60, min_distance=12, cull_params=cull_params, **kw))


def test_create_refusals():
    f = flow.Flow(flow.default_params(flow_back=0), 320, 240)
    try:
        assert _create(f, cull=1, iterations=0)[0] == abi.ERR_BAD_ARGUMENT and "iterations" in f.last_error()
        assert _create(f, cull=1, iterations=4097)[0] == abi.ERR_UNSUPPORTED
        assert _create(f, cull=1, pixel_error=float("nan"))[0] == abi.ERR_BAD_ARGUMENT and "pixel_error" in f.last_error()
        assert _create(f, cull=1, pixel_error=float("inf"))[0] == abi.ERR_BAD_ARGUMENT
        lib = tracker.load()
        for kw in (dict(cull=0, iterations=0), dict(cull=0, pixel_error=float("nan")), dict(cull=1, iterations=4096), dict(cull=1, iterations=1)):
            rc, h = _create(f, **kw)                  # the cull fields are looked at only when the cull is on
            assert rc == abi.OK, kw
            lib.visfs_tracker_destroy(h)
    finally:
        f.close()


def test_group_members_must_agree_on_the_cull():
    flows = [flow.Flow(flow.default_params(flow_back=0), 320, 240) for _ in range(2)]

    def pair(a, b):
        trks = [tracker.Tracker(f, flow.camera(), tracker.default_params(max_features=60, min_distance=12, cull=kw.pop("cull"),
                                                                         cull_params=fund.default_params(**kw)))
                for f, kw in zip(flows, (dict(a), dict(b)))]
        rc, h, why = tracker.group_create_status(trks)
        if h is not None:
            tracker.load().visfs_tracker_group_destroy(h)
        for t in trks:
            t.close()
        return rc, why

    try:
        base = dict(cull=1, iterations=64)
        assert pair(base, base)[0] == abi.OK
        for other in (dict(cull=0, iterations=64), dict(cull=1, iterations=65), dict(cull=1, iterations=64, pixel_error=2.0),
                      dict(cull=1, iterations=64, seed=1)):
            rc, why = pair(base, other)
            assert rc == abi.ERR_BAD_ARGUMENT and "member 1" in why and "tracker parameters differ" in why, (other, rc, why)
    finally:
        for f in flows:
            f.close()


def test_download_cull_before_a_call_is_refused():
    scn = cc.foreign()
    sub = cc.Subject(scn)
    refusal = f"status {abi.ERR_NOT_LOADED}: no call to report on"
    try:
        with pytest.raises(backend.BackendError, match=refusal):
            sub.trk.download_cull()
        out, inter = sub.process(*scn["frames"][0])
        assert out["flags"] == to.NO_PREVIOUS and inter is None
        with pytest.raises(backend.BackendError, match=refusal):
            sub.trk.download_cull()
        out, inter = sub.process(*scn["frames"][1])
        assert out["flags"] == to.BOOTSTRAPPED and inter["cull"]["applied"] == 1
    finally:
        sub.close()
