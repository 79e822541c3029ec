"""The resident front end on the GPU (include/visfs_tracker.h): visfs_tracker_process on the device against its host twin on the
cases of tests/test_tracker_host.py, byte for byte in every output array, flag and intermediate list; two trackers on one handle, a
BA solve between two calls, the refusal after a foreign push, and the staged chain on the device alongside."""
import numpy as np
import pytest

import tracker_cases as tc
import tracker_oracle as to
from visfs_amd import abi, backend, flow, synth, tracker

pytestmark = pytest.mark.gpu


@pytest.fixture()
def solver():
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    yield s
    s.close()


def _run(scn, solver, what=""):
    host, dev = tc.Subject(scn), tc.Subject(scn, solver=solver)
    try:
        return tc.lockstep(scn, host, [dev], what)
    finally:
        host.close(); dev.close()


@pytest.mark.parametrize("name", sorted(tc.BASE))
def test_base_sequence_equals_the_host_twin(solver, name):
    log = _run(tc.BASE[name](), solver, name)
    assert log[1][0]["flags"] == to.BOOTSTRAPPED and all(r["flags"] == 0 for r, _ in log[2:])
    assert any((i["disc_drawn"] == 0).any() for _, i in log[2:]) and sum(len(r["new_id"]) for r, _ in log[2:]) > 0


def test_full_size_equals_the_host_twin(solver):
    log = _run(tc.full_size(), solver, "full size")
    assert len(log[2][0]["word_id"]) > 150


@pytest.mark.parametrize("name", sorted(tc.WAVE))
def test_wave_boundary_counts_equal_the_host_twin(solver, name):
    scn = tc.WAVE[name]()
    log = _run(scn, solver, name)
    assert max(len(r["covisible_id"]) for r, _ in log) >= scn["trk"]["max_features"] - 8


@pytest.mark.parametrize("name", list(tc.WINDOW))
def test_window_sizes_equal_the_host_twin(solver, name):
    """tc.WINDOW on the device: the slot occupancies of the tracker's own copy of the wavefront's window cells."""
    log = _run(tc.WINDOW[name](), solver, name)
    assert log[1][0]["flags"] == to.BOOTSTRAPPED
    assert all(not (r["flags"] & to.LOST) for r, _ in log[2:]) and min(len(r["word_id"]) for r, _ in log[2:]) >= 40


@pytest.mark.parametrize("case", ["blocked_bootstrap", "bootstrap_nan", "lost_case", "no_top_up", "empty_top_up"])
def test_special_frames_equal_the_host_twin(solver, case):
    log = _run(getattr(tc, case)(), solver, case)
    if case == "bootstrap_nan":
        assert np.isnan(log[1][0]["covisible_from_xyz"]).any()
    if case == "lost_case":
        assert log[3][0]["flags"] == to.LOST and log[4][0]["flags"] == to.BOOTSTRAPPED
    if case == "no_top_up":
        assert any(len(r["covisible_id"]) == 8 and len(r["new_id"]) == 0 for r, _ in log)
    if case == "empty_top_up":
        assert len(log[3][0]["new_id"]) == 0 and len(log[3][1]["discs"]) > 0
    if case == "blocked_bootstrap":
        assert log[2][0]["flags"] == to.BOOTSTRAPPED and (log[2][1]["discs"]["radius"] == 6).all() and len(log[2][1]["discs"]) > 0


@pytest.mark.parametrize("name", sorted(tc.guess_cases()))
def test_guess_equals_the_host_twin(solver, name):
    _run(tc.guess_cases()[name], solver, name)


@pytest.mark.parametrize("name", sorted(tc.pretreatment_cases()))
def test_pretreatment_equals_the_host_twin(solver, name):
    log = _run(tc.pretreatment_cases()[name], solver, name)
    if name != "empty":
        assert any(len(r["blocked_id"]) > 0 for r, _ in log)


def test_full_length_outlier_list_equals_the_host_twin(solver):
    log = _run(tc.full_outliers(), solver, "4096 outliers")
    assert len(tc.full_outlier_list(log[1][0])) == tracker.MAX_OUTLIERS
    assert log[2][0]["flags"] == 0 and log[2][0]["blocked_id"].tolist() == tc.every_third(log[1][0])


def test_the_flow_object_goes_before_its_tracker(solver):
    """The tracker's own call block is freed while the flow object is still alive; the orphaned tracker refuses and can be destroyed."""
    scn = tc.scenario(tc.sequence(3), 60, 12)
    dev = tc.Subject(scn, solver=solver)
    dev.process(*scn["frames"][0])
    assert dev.process(*scn["frames"][1])[0]["flags"] == to.BOOTSTRAPPED
    dev.flow.close()
    rc, _ = dev.trk.process_status(*scn["frames"][2])
    assert rc == abi.ERR_NOT_LOADED and "the flow object of this tracker is gone" in dev.trk.last_error()
    dev.trk.close()


def test_min_inliers_at_and_just_above_the_kept_count(solver):
    seq = tc.sequence(4)
    kept = len(_run(tc.scenario(seq, 60, 12, min_inliers=0), solver, "kept count")[2][0]["covisible_id"])
    at = _run(tc.scenario(seq, 60, 12, min_inliers=kept), solver, "at")
    above = _run(tc.scenario(seq, 60, 12, min_inliers=kept + 1), solver, "above")
    assert at[2][0]["flags"] == 0 and above[2][0]["flags"] == to.LOST and above[3][0]["flags"] == to.BOOTSTRAPPED


def test_reset_and_argument_checks_on_the_device(solver):
    scn = tc.scenario(tc.sequence(4), 60, 12)
    host, dev = tc.Subject(scn), tc.Subject(scn, solver=solver)
    for k in range(3):
        to.assert_same(dev.process(*scn["frames"][k])[0], host.process(*scn["frames"][k])[0], f"frame {k}")
    host.trk.reset(); dev.trk.reset()
    want, got = host.process(*scn["frames"][3]), dev.process(*scn["frames"][3])
    to.assert_same(got[0], want[0], "after reset")
    to.assert_same(got[1], want[1], "after reset, intermediates")
    assert got[0]["flags"] == to.BOOTSTRAPPED and got[0]["covisible_id"].min() >= 60
    img = scn["frames"][0][0]
    assert dev.trk.process_status(img, img, outliers=[1], n_outliers=4097)[0] == abi.ERR_BAD_ARGUMENT
    assert dev.trk.process_status(None, img)[0] == abi.ERR_BAD_ARGUMENT
    assert tracker.create_status(dev.flow, flow.camera(), tracker.default_params(max_features=0))[0] == abi.ERR_BAD_ARGUMENT
    assert tracker.create_status(dev.flow, flow.camera(), tracker.default_params(max_features=4097))[0] == abi.ERR_UNSUPPORTED
    host.close(); dev.close()


def test_two_trackers_on_two_flows_of_one_handle(solver):
    a, b = tc.BASE["mf60_md12_clahe0_back1"](), tc.scenario(tc.sequence(8), 129, 12, clahe_on=True, flow_back=0, max_level=2)
    ha, hb, da, db = tc.Subject(a), tc.Subject(b), tc.Subject(a, solver=solver), tc.Subject(b, solver=solver)
    for k in range(8):
        fa, fb = a["frames"][k], b["frames"][7 - k]
        got_a = da.process(*fa)
        got_b = db.process(*fb)
        want_a, want_b = ha.process(*fa), hb.process(*fb)
        for got, want, what in ((got_a, want_a, "a"), (got_b, want_b, "b")):
            to.assert_same(got[0], want[0], f"{what} frame {k}")
            if want[1] is not None:
                to.assert_same(got[1], want[1], f"{what} frame {k} intermediates")
    for s in (ha, hb, da, db):
        s.close()


def test_ba_between_process_calls_returns_the_same_bytes(solver):
    wnd = synth.make_window("C1")
    rc0, rb0 = solver.solve_window(abi.WindowBuffers(wnd))
    assert rc0 == abi.OK
    scn = tc.scenario(tc.sequence(5), 60, 12)
    host, dev = tc.Subject(scn), tc.Subject(scn, solver=solver)
    for k, pair in enumerate(scn["frames"]):
        got, want = dev.process(*pair), host.process(*pair)
        to.assert_same(got[0], want[0], f"frame {k}")
        rc1, rb1 = solver.solve_window(abi.WindowBuffers(wnd))
        assert rc1 == rc0 and rb1.pose_Twr_out.tobytes() == rb0.pose_Twr_out.tobytes()
        assert rb1.struct.chi2_final == rb0.struct.chi2_final and rb1.outliers() == rb0.outliers()
    host.close(); dev.close()


def test_foreign_push_is_refused(solver):
    scn = tc.scenario(tc.sequence(4), 60, 12)
    dev = tc.Subject(scn, solver=solver)
    dev.process(*scn["frames"][0])
    dev.process(*scn["frames"][1])
    dev.flow.push_frame(*scn["frames"][2])
    rc, _ = dev.trk.process_status(*scn["frames"][3])
    assert rc == abi.ERR_NOT_LOADED and "pushed" in dev.trk.last_error()
    assert "member" not in dev.trk.last_error()
    dev.close()


def test_staged_chain_on_the_device_gives_the_same_bytes(solver):
    """The checker drives the staged calls (push_frame, track, corners, stereo) of a device flow next to the resident call on another
    device flow: the one call is pinned to the path users have today."""
    scn = tc.scenario(tc.sequence(8), 129, 13, outliers=[None, None, tc.first_middle_last, None, tc.every_third, None, None, tc.every_id],
                      guesses=[None, None, None, tc.translation(ty=0.023), None, None, None, None])
    staged, dev = tc.checker(scn, solver=solver), tc.Subject(scn, solver=solver)
    log = tc.lockstep(scn, staged, [dev], "staged on the device")
    assert sum(len(r["new_id"]) for r, _ in log[2:]) > 0 and staged.stats["undrawn"] > 0
    staged.close(); dev.close()
