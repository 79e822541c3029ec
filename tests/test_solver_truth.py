"""The extended-precision truth of tests/solver_truth.py, checked on the CPU: the oracle's PCG against a long-double PCG of the same
recurrence on the oracle's own S and b_s (same iteration counts, no stopping test near its threshold), the criterion
e <= 10 * max(eo, 1e-13) shown to bite on three small wrongs, solve_truth against a known answer at cond 1e10, and the oracle's direct
solver on the five ill-conditioned seeds.  tests/test_gpu_solver_forms.py holds every device kernel form to the same truth."""
import numpy as np
import pytest

import oracle_lib
import solver_forms as F
import solver_truth as T
from helpers import graph_of
from visfs_amd import abi, synth

LD = np.longdouble
WINDOWS = {
    "K12": lambda: synth.make_window("custom", n_kf=12, n_lm=480, n_obs=4800, seed=412),
    "K33": lambda: synth.make_window("custom", n_kf=33, n_lm=1320, n_obs=13200, seed=433),
    "K57": lambda: synth.make_window("custom", n_kf=57, n_lm=2280, n_obs=22800, seed=457),
    "K65": lambda: synth.make_window("custom", n_kf=65, n_lm=1300, n_obs=13000, seed=465),
    "C3": lambda: synth.make_window("C3"),
}


def _oracle(olib, w, solver=2, **kw):
    prm = abi.default_params(iterations=10, solver=solver, **kw)
    wb, gb, *_ = graph_of(olib.oracle_pack_window, prm, w)
    return oracle_lib.OracleSystem(olib, prm, gb)


@pytest.fixture(scope="module")
def oracle_runs(olib):
    """Every window through both sequences on the oracle alone, once: {(window, sequence): records}."""
    runs = {}
    for name, make in WINDOWS.items():
        w = make()
        for seq_name, seq in (("fresh", F.FRESH), ("commit", F.COMMIT)):
            o = _oracle(olib, w)
            runs[name, seq_name] = F.step_pair(o, None, seq, 2)
            o.close()
    return runs


@pytest.mark.parametrize("window", list(WINDOWS))
def test_oracle_pcg_takes_the_truth_s_iterations_and_stays_clear_of_its_thresholds(oracle_runs, window):
    for seq in ("fresh", "commit"):
        for rec in oracle_runs[window, seq]:
            print(f"{window} {seq} step {rec['step']} lambda {rec['lam']:.3e}: iterations {rec['it_o']} (truth {rec['it_truth_o']}), floor binds "
                  f"{rec['binding_o']}, closest {rec['closest_o']:.3f}, eo {rec['e_o']:.3e}")
            assert rec["ok_o"] == 1
            assert rec["it_o"] == rec["it_truth_o"], (window, seq, rec)
            assert rec["closest_o"] >= F.MIN_CLOSEST, (window, seq, rec)
            assert np.isfinite(rec["e_o"])
    assert any(rec["binding_o"] for rec in oracle_runs[window, "commit"]), "the carried floor never binds in the commit sequence"
    assert not any(rec["binding_o"] for rec in oracle_runs[window, "fresh"])


@pytest.fixture(scope="module")
def k33(olib):
    """The oracle's own system of K33 at lambda = 1e-5 max_diag, its solution and the truth's."""
    o = _oracle(olib, WINDOWS["K33"]())
    _, md = o.linearize()
    assert o.trial(1e-5 * md)[3] == 1
    n6 = 6 * o.npf
    S = o.fetch(abi.BUF_S).reshape(n6, n6).copy(); b = o.fetch(abi.BUF_BS).copy(); x = o.fetch(abi.BUF_DX_POSE).copy()
    npf = o.npf
    o.close()
    xt, it, _, _, _ = T.pcg_truth(S, b, npf)
    return S, b, x, npf, xt, it, T.rel_err_ld(x, xt)


def test_criterion_holds_for_the_oracle_itself(k33):
    S, b, x, npf, xt, it, eo = k33
    assert T.within_criterion(eo, eo) and eo < T.FLOOR


def test_criterion_rejects_a_solution_taken_one_iteration_early(k33):
    S, b, x, npf, xt, it, eo = k33
    early, it2, *_ = T.pcg_truth(S, b, npf, stop_after=it - 1)
    assert it2 == it - 1
    assert not T.within_criterion(T.rel_err_ld(early.astype(np.float64), xt), eo)


def test_criterion_rejects_a_solve_that_skips_one_small_off_diagonal_block(k33):
    S, b, x, npf, xt, it, eo = k33
    norms = {(i, j): np.abs(S[6 * i:6 * i + 6, 6 * j:6 * j + 6]).max() for i in range(npf) for j in range(i)}
    i, j = min((k for k, v in norms.items() if v > 0), key=norms.get)              # the smallest block that is there at all
    S2 = S.copy()
    S2[6 * i:6 * i + 6, 6 * j:6 * j + 6] = 0.0; S2[6 * j:6 * j + 6, 6 * i:6 * i + 6] = 0.0
    x2, *_ = T.pcg_truth(S2, b, npf)
    assert not T.within_criterion(T.rel_err_ld(x2.astype(np.float64), xt), eo), (i, j, norms[i, j])


def test_criterion_rejects_one_component_moved_by_1e_10(k33):
    S, b, x, npf, xt, it, eo = k33
    x2 = x.copy()
    k = int(np.abs(x2).argmax())
    x2[k] *= 1.0 + 1e-10
    assert not T.within_criterion(T.rel_err_ld(x2, xt), eo)


def test_solve_truth_recovers_a_known_solution_at_cond_1e10():
    rng = np.random.default_rng(5)
    n, cond = 90, 1e10
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0, -10, n)) @ Q.T
    A = 0.5 * (A + A.T)                                                            # an fp64 matrix, taken as exact from here on
    x = rng.standard_normal(n)
    b = A.astype(LD) @ x.astype(LD)                                                # formed in long double, not rounded to fp64
    xt, res = T.solve_truth(A, b)
    e = T.rel_err_ld(xt, x)
    print(f"solve_truth at cond {np.linalg.cond(A):.2e}: error {e:.3e}, relative residual {res:.3e}")
    assert e <= 1e-15 * cond * 10 and res < n * np.finfo(LD).eps                   # (a backward-stable solve in long double)
    assert e < 0.01 * T.rel_err_ld(np.linalg.solve(A, b.astype(np.float64)), x)    # and far nearer than an fp64 solve gets


@pytest.mark.parametrize("seed", F.ILL_SEEDS)
def test_oracle_direct_solver_against_the_truth_on_ill_conditioned_systems(olib, seed):
    w, kw = F.make_window(("ill", seed))
    o = _oracle(olib, w, solver=0, **kw)
    for rec in F.step_pair(o, None, F.DIRECT, 0):
        n6, cond = 6 * o.npf, rec["cond_o"]
        print(f"seed {seed} lambda {rec['lam']:.0e}: cond {cond:.2e}, eo {rec['e_o']:.3e}, truth residual {rec['residual_o']:.3e}")
        assert rec["ok_o"] == 1 and rec["residual_o"] < n6 * np.finfo(LD).eps
        assert rec["e_o"] <= 1e-15 * cond * 10
    o.close()


def test_case_table_of_the_gpu_tests_names_every_solver_code_and_switch():
    """The table that tests/test_gpu_solver_forms.py runs (its describe() assertions prove on the GPU that each form ran; this only keeps
    a code or a switch from dropping out of the table unnoticed)."""
    cases = F.CASES.values()
    assert {c["code"] for c in cases} == {1, 2, 3, 4, 5, 6, 7}
    envs = {(k, v) for c in cases for k, v in c["env"].items()}
    for want in [("VISFS_BA_PCG_GATHER", "0"), ("VISFS_BA_PCG_GATHER", "2"), ("VISFS_BA_PCG_GATHER", "3"), ("VISFS_BA_SMALL_PCG_LDS", "1"),
                 ("VISFS_BA_PCG1", "0"), ("VISFS_BA_PCG_CU", "1"), ("VISFS_BA_SMALL_SOLVE", "0"), ("VISFS_BA_BAND", "0")]:
        assert want in envs, want
    assert any(c["tuning"] == abi.TUNE_THROUGHPUT and c["code"] == 4 and F.COMMIT in c["seqs"] for c in cases)
    assert any(c["band"] and c["band"][1] for c in cases) and any(c["band"] and c["band"][0] == "lds" for c in cases)
    assert any(c["band"] == ("fast", None) and c["npf"] == 49 for c in cases)      # C2 resident: ten blocks per row, the unrolled backward chain
