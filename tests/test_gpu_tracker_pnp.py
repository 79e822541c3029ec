"""The pose guess inside the resident front end on the GPU (include/visfs_tracker_pnp.h): the device tracker
against the host twin on the cases of tracker_pnp_cases.py, visfs_tracker_pnp_last and visfs_tracker_download_pnp included; the
checker driving the staged calls of a device flow and a device visfs_pnp alongside; the device group against the singly-run host
twins; and what a call issues.  Every comparison is of bytes."""
import pytest

import group_cases as gc
import tracker_pnp_cases as pc
import tracker_pnp_oracle as tpo
from visfs_amd import abi, backend, synth, tracker_pnp

pytestmark = pytest.mark.gpu

STEADY, BOOT, CULL, PNP = 16, 23, 3, 3         # launches of a call, what the cull adds (9j), what the pose guess adds (9k)


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_device_equals_the_host_twin(solver, name):
    scn, log = pc.host_log(name)
    dev = pc.Subject(scn, solver=solver)
    try:
        pc.against_log(scn, log, dev, name)
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["foreign", "foreign_cull", "tight", "nan_rows", "m4", "no_words"])
def test_staged_chain_on_the_device_gives_the_same_bytes(solver, name):
    """The checker on a device flow object and a device visfs_pnp: today's staged path, call by call, next to the resident call."""
    scn, log = pc.host_log(name)
    ref, dev = pc.checker(scn, solver=solver), pc.Subject(scn, solver=solver)
    try:
        staged = pc.lockstep(scn, ref, [dev], name + " staged")
        for k in range(len(log)):
            pc.same(staged[k], log[k], f"{name}: staged against the host twin, frame {k}")
        pc.assert_conditions(name, scn, staged)
    finally:
        ref.close(); dev.close()


def test_disabled_again_is_the_tracker_without_it(solver):
    """Enabled, one frame, disabled: from then on the pose guess does not run, and the tracker's outputs stay those of the log."""
    scn, log = pc.host_log("steady")
    dev = pc.Subject(scn, solver=solver)
    try:
        for k, (left, right) in enumerate(scn["frames"]):
            if k == 2:
                tracker_pnp.enable(dev.trk, None)
            got = dev.process(left, right)
            gc.same(got, log[k], f"frame {k}")
            tpo.assert_same_pose(got[0]["pose"], log[k][0]["pose"] if k < 2 else tpo.not_ran(), f"frame {k}")
            if k >= 2:
                tpo.assert_same_hook(got[1]["pnp"], tpo.inactive(), f"frame {k}")
    finally:
        dev.close()


def _syncs_ok(rig):
    assert rig.counts and all(c["synchronisations"] <= 2 and c["kernel_launches"] > 0 for c in rig.counts), rig.counts


def test_device_group_equals_the_host_twins(solver):
    members, log, _ = pc.rig_reference()
    dev = pc.Rig(members, solver=solver)
    try:
        pc.rig_against(members, log, dev, "rig")
        _syncs_ok(dev)
    finally:
        dev.close()


def test_ba_between_group_calls_changes_nothing(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    members, log, _ = pc.rig_reference()
    dev = pc.Rig(members, solver=solver)

    def solve(k):
        rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
        assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
        assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()

    try:
        pc.rig_against(members, log, dev, "BA between", between=solve)
        solve(len(log))
    finally:
        dev.close()


def _counts(members, log, solver, cull=1, enable=True):
    """The counts of every group call of a rig (results compared with the log where the log is of the same setting)."""
    dev = pc.Rig(members, solver=solver, cull=cull, enable=enable)
    try:
        if cull and enable:
            pc.rig_against(members, log, dev, "counts")
        else:                                  # other results or no pose: only the counts are looked at
            prev = [None] * len(members)
            for i, m in enumerate(members):
                for pair in m["pre"]:
                    prev[i] = dev.single(i, *pair)[0]
            for k in range(len(log)):
                prev = [r for r, _ in dev.grouped(gc.call_args(members, k, prev))]
        _syncs_ok(dev)
        return dev.counts
    finally:
        dev.close()


def test_what_a_call_issues(solver):
    members, log, boots = pc.rig_reference()
    steady = [k for k, row in enumerate(boots) if not any(row)]
    assert steady and any(any(row) for row in boots), boots
    one_log = [call[:1] for call in log]
    launches = lambda counts: [c["kernel_launches"] for c in counts]
    four_c = _counts(members, log, solver)
    four, one = launches(four_c), launches(_counts(members[:1], one_log, solver))
    print("kernel launches per call: one", one, "four", four, "member boots", boots)
    # member 0 bootstraps in call 1 and is steady from call 2 on
    assert one[1] == BOOT + CULL + PNP and one[2] == STEADY + CULL + PNP
    assert all(four[k] == one[2] for k in steady)
    assert all(four[k] == one[1] for k, row in enumerate(boots) if any(row))     # however many members boot
    no_cull = launches(_counts(members[:1], one_log, solver, cull=0))
    assert no_cull[1] == BOOT + PNP and no_cull[2] == STEADY + PNP
    off = launches(_counts(members[:1], one_log, solver, cull=0, enable=False))
    assert off[1] == BOOT and off[2] == STEADY
    off_cull_c = _counts(members, log, solver, enable=False)                        # the same calls without the pose guess
    assert launches(off_cull_c)[steady[0]] == STEADY + CULL
    assert [c["kernel_launches"] - PNP for c in four_c] == launches(off_cull_c)
    assert [c["copies_and_memsets"] for c in four_c] == [c["copies_and_memsets"] for c in off_cull_c]
