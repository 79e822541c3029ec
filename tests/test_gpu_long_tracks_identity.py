"""GPU: the fused tail of the speculative unit (k_backsub<LINA>) on LONG tracks.

The fused tail of a lone window keeps the static data of every lane's FIRST observation, the landmark's index data and both estimate
buffers in registers, loaded in front of the kernel's gate; every later pass of a lane over its track loads as before.  The windows of
tests/test_gpu_parity.py::test_fused_speculative_unit_equals_the_two_launch_form_and_the_gated_unit have tracks of at most 10
observations on 8 lanes (two passes).  These have tracks of about 30 on 8 lanes (four passes) and on 4 lanes (eight passes), so the
hand-over from the pre-loaded pass to the loading ones, inactive edges in the middle of a lane's passes and rejected trials (the
pre-loaded estimate buffer that must NOT be taken) are all exercised.  Same three-way comparison, bit for bit: the gated unit
(VISFS_BA_SPEC=0), the two-launch form (VISFS_BA_SPEC_FUSED=0: a plain k_backsub and k_linearize<SPEC>) and the fused tail."""
import numpy as np
import pytest

from helpers import ragged_window
from visfs_amd import abi, synth

pytestmark = pytest.mark.gpu

LONG = dict(n_kf=40, n_lm=1200, n_obs=36000)        # >= 1024 landmarks: 8 lanes per landmark; tracks of 30


def _stats_tuple(st):
    return (list(st.iterations_run), list(st.trials_run), st.pcg_iterations, st.n_outliers, st.chi2_initial, st.chi2_phase1, st.chi2_final,
            [st.trace_lambda[i] for i in range(st.n_trace)], [st.trace_chi2[i] for i in range(st.n_trace)])


def _solve_in_mode(monkeypatch, w, env, **prm_kw):
    from visfs_amd import backend
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prm = abi.default_params(**prm_kw)
    s = backend.Solver(prm)
    gb, *_ = abi.pack_window_with(s.lib.visfs_ba_pack_window, prm, abi.WindowBuffers(w))
    s.upload(gb)
    info = s.describe()
    rc, st = s.optimize()
    out = s.download()
    s.close()
    return info, rc, st, out


def _window(case):
    if case == "RAGGED":        # 35 % of the references dropped: tracks of every length from 0 up, inactive edges after the outlier pass
        return ragged_window(seed=7, **LONG)
    if case == "HARD":          # large landmark noise, no fixed landmark: the LM loop rejects damped solves (checked with the CPU oracle: 29 trials for 20 iterations)
        return synth.make_window("custom", seed=5, point_noise=1.0, fixed_frac=0.0, **LONG)
    return synth.make_window("custom", seed=11, **LONG)


def test_long_track_windows_have_the_tracks_they_claim():
    """(no GPU needed for the claim itself, but the module is GPU-marked: it guards the cases below)"""
    cnt = np.bincount(np.asarray(_window("LONG")["ref_feature"]), minlength=LONG["n_lm"])
    assert cnt.min() == cnt.max() == 30
    cnt = np.bincount(np.asarray(_window("RAGGED")["ref_feature"]), minlength=LONG["n_lm"])
    assert cnt.min() == 0 and cnt.max() > 24 and len(set(cnt.tolist())) > 15


@pytest.mark.parametrize("case", ["LONG", "RAGGED", "HARD", "GROUP4"])
def test_fused_tail_on_long_tracks_equals_the_two_launch_form_and_the_gated_unit(monkeypatch, case):
    kw = dict(iterations=20, solver=2)
    w = _window(case)
    if case == "GROUP4":
        monkeypatch.setenv("VISFS_BA_GROUP", "4")
    _, rc0, st0, out0 = _solve_in_mode(monkeypatch, w, dict(VISFS_BA_SPEC="0"), **kw)
    _, rc1, st1, out1 = _solve_in_mode(monkeypatch, w, dict(VISFS_BA_SPEC="1", VISFS_BA_SPEC_FUSED="0"), **kw)
    info, rc2, st2, out2 = _solve_in_mode(monkeypatch, w, dict(VISFS_BA_SPEC="1", VISFS_BA_SPEC_FUSED="1"), **kw)
    assert rc0 == rc1 == rc2 == abi.OK
    assert info["lanes_per_landmark"] == (4 if case == "GROUP4" else 8) and info["unit_form"] == 2      # (2: the fused speculative unit)
    assert _stats_tuple(st0) == _stats_tuple(st1) == _stats_tuple(st2)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out0, out2))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out1, out2))
    if case == "HARD":
        assert sum(st0.trials_run) > sum(st0.iterations_run)          # the window really rejects trials
