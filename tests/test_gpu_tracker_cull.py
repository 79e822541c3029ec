"""Tracker/CullByFundationMatrix inside the resident front end on the GPU: the device tracker against the
host twin on the cases of tracker_cull_cases.py, visfs_tracker_download_cull included; the checker driving the staged calls of a
device flow and a device cull alongside; the device group against the singly-run host twins; and what a call issues.  Every
comparison is of bytes."""
import pytest

import group_cases as gc
import tracker_cull_cases as cc
from visfs_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

STEADY, BOOT, ADDED = 16, 23, 3                # launches of a call without the cull, and what the cull adds


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_device_equals_the_host_twin(solver, name):
    scn, log = cc.host_log(name)
    dev = cc.Subject(scn, solver=solver)
    try:
        cc.against_log(scn, log, dev, name)
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["foreign", "nan_rows", "m7"])
def test_staged_chain_on_the_device_gives_the_same_bytes(solver, name):
    """The checker on a device flow object and a device visfs_fund: today's staged path, call by call, next to the resident call."""
    scn, log = cc.host_log(name)
    ref, dev = cc.checker(scn, solver=solver), cc.Subject(scn, solver=solver)
    try:
        staged = cc.lockstep(scn, ref, [dev], name + " staged")
        for k in range(len(log)):
            cc.same(staged[k], log[k], f"{name}: staged against the host twin, frame {k}")
    finally:
        ref.close(); dev.close()


def _syncs_ok(rig):
    assert rig.counts and all(c["synchronisations"] <= 2 and c["kernel_launches"] > 0 for c in rig.counts), rig.counts


def test_device_group_equals_the_host_twins(solver):
    members, log, _ = cc.rig_reference()
    dev = cc.Rig(members, solver=solver)
    try:
        cc.rig_against(members, log, dev, "rig")
        _syncs_ok(dev)
    finally:
        dev.close()


def test_ba_between_group_calls_changes_nothing(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    members, log, _ = cc.rig_reference()
    dev = cc.Rig(members, solver=solver)

    def solve(k):
        rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
        assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
        assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()

    try:
        cc.rig_against(members, log, dev, "BA between", between=solve)
        solve(len(log))
    finally:
        dev.close()


def _launches(members, log, solver, cull=1, flow_back=0):
    dev = cc.Rig(members, solver=solver, cull=cull, flow_back=flow_back)
    try:
        if cull and not flow_back:
            cc.rig_against(members, log, dev, "counts")
        else:                                  # other results: only the counts are looked at
            prev = [None] * len(members)
            for i, m in enumerate(members):
                for pair in m["pre"]:
                    prev[i] = dev.single(i, *pair)[0]
            for k in range(len(log)):
                prev = [r for r, _ in dev.grouped(gc.call_args(members, k, prev))]
        _syncs_ok(dev)
        return [c["kernel_launches"] for c in dev.counts]
    finally:
        dev.close()


def test_kernel_launches_of_a_call(solver):
    members, log, boots = cc.rig_reference()
    steady = [k for k, row in enumerate(boots) if not any(row)]
    one_boots = [k for k, row in enumerate(boots) if sum(row) == 1]
    assert steady and one_boots, boots
    four = _launches(members, log, solver)
    one = _launches(members[:1], [call[:1] for call in log], solver)
    print("kernel launches per call: one", one, "four", four, "member boots", boots)
    assert one[1] == BOOT + ADDED and one[2] == STEADY + ADDED         # member 0 bootstraps in call 1 and is steady from call 2 on
    assert all(four[k] == one[2] for k in steady)
    assert all(four[k] == one[1] for k in one_boots)
    assert all(four[k] == one[1] for k, row in enumerate(boots) if any(row))   # however many members boot
    off = _launches(members[:1], [call[:1] for call in log], solver, cull=0)
    assert off[1] == BOOT and off[2] == STEADY
    inert = _launches(members[:1], [call[:1] for call in log], solver, cull=1, flow_back=1)      # cull = 1 ignored with the reverse pass on
    assert inert[1] == BOOT and inert[2] == STEADY
