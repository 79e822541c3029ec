"""Every kernel form that solves the reduced camera system S dx = b_s, held to an extended-precision truth of ITS OWN system.

check_stages (test_gpu_parity.py) compares dx_pose across two systems (the device's S and the oracle's differ by ~1e-13 and cond(S)
is 1e4 .. 1e11), so its bound has to be 1e-7.  Here each side's S and b_s are fetched and solved in numpy.longdouble
(tests/solver_truth.py); the device must be as near the truth of its system as the oracle is to the truth of its own:
    eg <= 10 * max(eo, 1e-13)
— the criterion of test_banded_solver_keeps_the_checker_s_accuracy_on_ill_conditioned_systems, now with a real truth and with every
solver code of visfs_ba_graph_describe (1 .. 7) and every switch behind it.  The cases and the per-step assertions live in
tests/solver_forms.py; measured values: profiles/solver_forms_truth.log."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import solver_forms as F
from helpers import graph_of, rel_err
from visfs_amd import abi, synth

pytestmark = pytest.mark.gpu

CHILD_ENV = {"gather0": ("VISFS_BA_PCG_GATHER", "0"), "gather2": ("VISFS_BA_PCG_GATHER", "2"), "gather3": ("VISFS_BA_PCG_GATHER", "3"),
             "small-lds": ("VISFS_BA_SMALL_PCG_LDS", "1")}
IN_PROCESS = [n for n in F.CASES if not any(n.startswith(f"pcg-{k}-") for k in CHILD_ENV)]
CHILD_TIMEOUT = 60                                    # seconds, each child its own


def _check(records):
    assert records
    for rec in records:
        print(F.log_line(rec))                         # (every figure before any assertion: pytest -s keeps them, profiles/solver_forms_truth.log)
    for rec in records:
        F.check_record(rec)


@pytest.mark.parametrize("name", IN_PROCESS)
def test_solver_form_against_the_truth_of_its_own_system(olib, monkeypatch, name):
    for k in ("VISFS_BA_PCG_CU", "VISFS_BA_PCG1", "VISFS_BA_SMALL_SOLVE", "VISFS_BA_BAND", "VISFS_BA_BAND_ROWS"):
        monkeypatch.delenv(k, raising=False)
    _check(F.run_case(olib, name))


def test_switches_read_once_per_process_in_a_child_process_each():
    """VISFS_BA_PCG_GATHER=0|2|3 (k_pcg1's gather variants) at 11 and 64 free poses, VISFS_BA_SMALL_PCG_LDS=1 (the LDS-row PCG of
    k_small_solve) at 1, 7 and 10: statics of the library, so each runs in a fresh child with the variable set, one child at a time, each
    under its own time limit.  A child that ends by a signal, with 134 / 139 or at its limit fails the test and no further child starts."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "solver_form_child.py")
    for key, (var, value) in CHILD_ENV.items():
        names = [n for n in F.CASES if n.startswith(f"pcg-{key}-")]
        assert names and all(F.CASES[n]["env"] == {var: value} for n in names)
        env = dict(os.environ); env[var] = value
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [child] + names
        try:
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{var}={value}: the child ran into its time limit of {CHILD_TIMEOUT} s; no further child is started")
        assert p.returncode == 0, f"{var}={value}: the child ended with {p.returncode}; no further child is started\n{p.stderr[-2000:]}"
        records = json.loads(p.stdout.strip().splitlines()[-1])["records"]
        assert {r["case"] for r in records} == set(names)
        _check(records)


# ---------------------------------------------------------------- batched launches against the checker
BATCH = [("custom", 12, 712), ("custom", 14, 714), ("custom", 33, 733), ("c3odo", 50, 750), ("custom", 57, 757), ("custom", 12, 812),
         ("custom", 33, 833), ("custom", 57, 857)]


@pytest.fixture(scope="module")
def batch_windows(olib):
    """The eight windows (11, 13, 32, 49 with odometry and 56 free poses, some twice with other seeds), packed once, and what the oracle's
    optimize() makes of each — computed once and shared by the three batch tests."""
    prm = abi.default_params(iterations=10, solver=2)
    out = []
    for kind, n_kf, seed in BATCH:
        w = synth.make_window("custom", n_kf=n_kf, n_lm=40 * n_kf, n_obs=400 * n_kf, seed=seed, odo=(kind == "c3odo"))
        wb, gb, *_ = graph_of(olib.oracle_pack_window, prm, w)
        o = oracle_lib.OracleSystem(olib, prm, gb)
        rc, st, _ = o.optimize()
        ref = (rc, list(st.iterations_run), list(st.trials_run), st.pcg_iterations) + tuple(o.download())
        o.close()
        out.append((gb, ref))
    return prm, out


def _batch_against_oracle(prm, windows, tuning, want_codes):
    from visfs_amd import backend
    s = backend.Solver(prm, tuning=tuning)
    try:
        codes = []
        for gb, _ in windows:                              # the kernel a window gets follows the handle, never the batch: a single upload says it
            s.upload(gb); codes.append(s.describe()["solver_kernel"])
        assert set(codes) == want_codes, codes
        s.batch_upload([gb for gb, _ in windows])
        s.batch_reset()
        rc, stats = s.batch_optimize()
        assert rc == abi.OK
        for i, (gb, (rco, it_o, tr_o, pcg_o, po, pto, outo, chio)) in enumerate(windows):
            st = stats[i]
            pg, ptg, outg, chig = s.batch_download(i)
            assert st.status == rco == abi.OK, i
            assert list(st.iterations_run) == it_o and list(st.trials_run) == tr_o and st.pcg_iterations == pcg_o, (i, list(st.iterations_run), it_o, st.pcg_iterations, pcg_o)
            assert np.array_equal(outo, outg), (i, "outlier sets differ")
            assert rel_err(pg, po) < 1e-6 and rel_err(ptg, pto) < 1e-6, i
    finally:
        s.close()
    return codes


def test_batch_on_a_throughput_handle_matches_the_oracle_member_by_member(batch_windows, monkeypatch):
    """The C5 share on the kernel the bench reports: batch_upload / batch_optimize on a handle tuned for throughput (k_pcg_cu: code 4 for
    every member here), every member held to oracle.optimize() — iterations, trials, PCG iterations, outliers equal; poses and points to 1e-6."""
    for k in ("VISFS_BA_PCG_CU", "VISFS_BA_PCG1"):
        monkeypatch.delenv(k, raising=False)
    prm, windows = batch_windows
    _batch_against_oracle(prm, windows, abi.TUNE_THROUGHPUT, {4})


def test_batch_on_the_default_tuning_matches_the_oracle_member_by_member(batch_windows, monkeypatch):
    for k in ("VISFS_BA_PCG_CU", "VISFS_BA_PCG1"):
        monkeypatch.delenv(k, raising=False)
    prm, windows = batch_windows
    _batch_against_oracle(prm, windows, None, {1})


def test_batch_on_the_four_wave_kernel_matches_the_oracle_member_by_member(batch_windows, monkeypatch):
    monkeypatch.delenv("VISFS_BA_PCG_CU", raising=False)
    monkeypatch.setenv("VISFS_BA_PCG1", "0")
    prm, windows = batch_windows
    _batch_against_oracle(prm, windows, None, {2})
