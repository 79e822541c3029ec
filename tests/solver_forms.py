"""Every kernel form that solves the reduced camera system, stepped beside the oracle and held to an extended-precision truth.

TEST INFRASTRUCTURE ONLY: the case table, the stepping helper and the per-step assertions of tests/test_gpu_solver_forms.py (the oracle
side alone serves tests/test_solver_truth.py on the CPU).  `run_case` steps a device / oracle pair through a sequence of damped solves;
per step it fetches each side's own S, b_s and dx_pose, solves each side's own system with tests/solver_truth.py (the PCG floor carried
from that side's previous truth solve, as both implementations carry LinearSolverPCG::_residual) and returns one record per step;
`check_record` asserts on it.  tests/solver_form_child.py runs named cases in a process of its own.
"""
import contextlib
import os

import numpy as np

import solver_truth as T
from helpers import graph_of, random_case
from visfs_amd import abi, synth

# a step: ("fresh", f)  LinearSolverPCG::init() on both sides, lambda = f * max_diag of the last linearisation
#         ("commit", f) commit the last trial, linearise, lambda = f * the previous lambda (the LM loop after an accepted step)
#         ("abs", lam)  lambda = lam as given (the direct solver's cases: the lambdas of the ill-conditioned seeds)
FRESH = (("fresh", 1e-5), ("fresh", 1.0))
COMMIT = (("fresh", 1e-5), ("commit", 1.0 / 3), ("commit", 1.0 / 3), ("commit", 1.0 / 3))
DIRECT = (("abs", 1e-2), ("abs", 1e-5))
ILL_SEEDS = (559, 764, 873, 1136, 1242)         # test_gpu_random.random_case: cond(S) 1e8 at lambda = 1e-2, 1e11 at 1e-5
MIN_CLOSEST = 0.05                              # a truth stopping test nearer than this to its threshold: replace the seed


def make_window(spec):
    kind = spec[0]
    if kind == "custom":                        # 40 landmarks and 400 observations per key-frame
        n_kf, seed = spec[1], spec[2]
        n_lm = 40 * n_kf
        return synth.make_window("custom", n_kf=n_kf, n_lm=n_lm, n_obs=min(400 * n_kf, n_lm * n_kf), seed=seed), {}
    if kind == "sparse":                        # the shapes of test_pcg_register_block_variants: 6 landmarks, 35 observations per key-frame
        n_kf, seed = spec[1], spec[2]
        return synth.make_window("custom", n_kf=n_kf, n_lm=6 * n_kf, n_obs=35 * n_kf, seed=seed), {}
    if kind == "c3":                            # C3 (49 wheel-odometry edges) at a reduced landmark count
        return synth.make_window("C3", n_kf=50, n_lm=2000, n_obs=20000), {}
    if kind == "C2":
        return synth.make_window("C2"), {}
    if kind == "ill":
        w, kw = random_case(spec[1])
        return w, dict(robust_kernel_delta=kw["robust_kernel_delta"])
    if kind == "hb15":                          # tracks of 16 key-frames: block half-bandwidth 15, the LDS backward sweep of k_band_chol
        return synth.make_window("custom", n_kf=30, n_lm=200, n_obs=3200, seed=12), {}
    raise KeyError(kind)


def _case(window, solver, code, npf=None, env=None, tuning=None, seqs=(FRESH,), band=None):
    return dict(window=window, solver=solver, code=code, npf=npf, env=dict(env or {}), tuning=tuning, seqs=tuple(seqs), band=band)


def custom_window(npf):
    if npf <= 64:
        return ("custom", npf + 1, 400 + npf + 1)
    # (257 free poses: seeds 17 and 18 bring a stopping test of the commit sequence within 5 % of its threshold on the truth — replaced)
    return ("sparse", npf + 1, 19 if npf == 257 else 17)


def _build_cases():
    cases = {}
    def pcg(form, code, sizes, env=None, tuning=None, both_first=True, window=None):
        for n, npf in enumerate(sizes):
            cases[f"pcg-{form}-{npf}"] = _case(window or custom_window(npf), 2, code, npf, env, tuning, (FRESH, COMMIT) if both_first and n == 0 else (FRESH,))
    pcg("small", 5, (1, 6, 7, 10))
    pcg("pcg1", 1, (11, 63, 64))
    pcg("pcg1-nosmall", 1, (1, 10), env={"VISFS_BA_SMALL_SOLVE": "0"}, both_first=False)
    pcg("fourwave-low", 2, (11, 64), env={"VISFS_BA_PCG1": "0"})
    pcg("fourwave", 2, (65, 128, 129, 256))
    pcg("rows", 3, (257,))
    pcg("cu", 4, (11, 32), env={"VISFS_BA_PCG_CU": "1"})
    pcg("cu-odo", 4, (49,), env={"VISFS_BA_PCG_CU": "1"}, both_first=False, window=("c3",))
    pcg("cu", 4, (56,), env={"VISFS_BA_PCG_CU": "1"}, both_first=False)
    pcg("cu-handle", 4, (56,), tuning=abi.TUNE_THROUGHPUT)
    pcg("cu-handle-above", 1, (57,), tuning=abi.TUNE_THROUGHPUT)
    # the switches read once per process (a child process each)
    for gv in (0, 2, 3):
        pcg(f"gather{gv}", 1, (11, 64), env={"VISFS_BA_PCG_GATHER": str(gv)}, both_first=False)
    pcg("small-lds", 5, (1, 7, 10), env={"VISFS_BA_SMALL_PCG_LDS": "1"}, both_first=False)

    def direct(name, window, code, env=None, npf=None, band=None):
        cases[f"direct-{name}"] = _case(window, 0, code, npf, env, None, (DIRECT,), band)
    for npf in (1, 5, 6, 10):
        direct(f"small-{npf}", custom_window(npf), 5, npf=npf)
    for seed in ILL_SEEDS:
        direct(f"band-ill{seed}", ("ill", seed), 7, band=("fast", None))
        direct(f"dense-ill{seed}", ("ill", seed), 6, env={"VISFS_BA_BAND": "0"})
    for seed, rows in STREAMING_ILL:
        direct(f"band-stream-ill{seed}", ("ill", seed), 7, env={"VISFS_BA_BAND_ROWS": str(rows)}, band=("fast", rows))
    # C2: half-bandwidth 9, ten blocks per row — resident, the one band width with the unrolled backward chain (every BASELINE window)
    direct("band-C2", ("C2",), 7, npf=49, band=("fast", None))
    direct("dense-C2", ("C2",), 6, env={"VISFS_BA_BAND": "0"}, npf=49)
    direct("band-stream-C2", ("C2",), 7, env={"VISFS_BA_BAND_ROWS": "12"}, npf=49, band=("fast", 12))
    direct("band-hb15", ("hb15",), 7, npf=29, band=("lds", None))
    direct("band-stream-hb15", ("hb15",), 7, env={"VISFS_BA_BAND_ROWS": "19"}, npf=29, band=("lds", 19))
    direct("dense-hb15", ("hb15",), 6, env={"VISFS_BA_BAND": "0"}, npf=29)
    return cases


# the ill-conditioned seeds whose window admits the streaming form (the plan takes VISFS_BA_BAND_ROWS from half-bandwidth + 3 rows on,
# below the free poses of the window: ba_plan.hpp, plan_band), with the rows they stream through
STREAMING_ILL = ((559, 4), (764, 4), (873, 6), (1136, 7), (1242, 4))      # half-bandwidths 1, 1, 3, 4, 1 of 12, 13, 13, 12, 11 block rows
CASES = _build_cases()


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _solve_side(side, lam, solver, floor):
    """One damped solve on one side and the truth of that side's own system."""
    _, _, iters, ok = side.trial(lam)
    n6 = 6 * side.npf
    S = side.fetch(abi.BUF_S).reshape(n6, n6); b = side.fetch(abi.BUF_BS); x = side.fetch(abi.BUF_DX_POSE)
    if solver == 2:
        xt, it, floor_out, binding, closest = T.pcg_truth(S, b, side.npf, floor)
        return dict(ok=int(ok), it=int(iters), it_truth=int(it), binding=bool(binding), closest=float(closest), e=T.rel_err_ld(x, xt)), floor_out
    xt, res = T.solve_truth(S, b)
    return dict(ok=int(ok), it=0, it_truth=0, binding=False, closest=float("inf"), e=T.rel_err_ld(x, xt), residual=res, cond=float(np.linalg.cond(S))), -1.0


def step_pair(o, s, seq, solver):
    """Run the steps of `seq` on the oracle `o` and, when given, the device `s`: one record per step."""
    sides = [("o", o)] + ([("g", s)] if s is not None else [])
    out = []
    floors = {k: -1.0 for k, _ in sides}
    lam = md = None
    for n, (kind, f) in enumerate(seq):
        if kind == "commit":
            for _, side in sides:
                side.commit()
        if kind == "commit" or md is None:
            for k, side in sides:
                _, m = side.linearize()
                if k == "o":
                    md = m
        if kind == "fresh":
            for k, side in sides:
                side.begin_phase(); floors[k] = -1.0
        lam = f * md if kind == "fresh" else f * lam if kind == "commit" else f
        rec = dict(step=n, kind=kind, lam=float(lam))
        for k, side in sides:
            r, floors[k] = _solve_side(side, lam, solver, floors[k])
            rec.update({f"{key}_{k}": v for key, v in r.items()})
        out.append(rec)
    return out


def run_case(olib, name):
    """All sequences of case `name` on a fresh device / oracle pair each: the records, each with what describe() said."""
    import oracle_lib
    from visfs_amd import backend
    case = CASES[name]
    w, prm_kw = make_window(case["window"])
    records = []
    with environment(case["env"]):
        for seq in case["seqs"]:
            prm = abi.default_params(iterations=10, solver=case["solver"], **prm_kw)
            wb, gb, *_ = graph_of(olib.oracle_pack_window, prm, w)
            o = oracle_lib.OracleSystem(olib, prm, gb)
            s = backend.Solver(prm, tuning=case["tuning"])
            try:
                s.upload(gb)
                info = s.describe()
                for rec in step_pair(o, s, seq, case["solver"]):
                    rec.update(case=name, seq="commit" if seq is COMMIT else "fresh" if seq is FRESH else "direct", code=info["solver_kernel"],
                               npf=info["n_free_poses"], npf_o=o.npf, band_blocks=info["band_blocks"])
                    records.append(rec)
            finally:
                s.close(); o.close()
    return records


def check_record(rec, factor=T.FACTOR, floor=T.FLOOR):
    """The assertions of one step: the form that ran, both solves succeeded, the PCG counts, the input's distance from the thresholds and
    the criterion  eg <= factor * max(eo, floor)."""
    case = CASES[rec["case"]]
    tag = (rec["case"], rec["seq"], rec["step"])
    assert rec["code"] == case["code"], (tag, "solver_kernel", rec["code"])
    assert rec["npf"] == rec["npf_o"] and (case["npf"] is None or rec["npf"] == case["npf"]), (tag, "n_free_poses", rec["npf"])
    if case["band"] is not None:
        sweep, rows = case["band"]
        B = rec["band_blocks"]
        assert (B <= 9) if sweep == "fast" else (B > 9), (tag, "band_blocks", B)      # 6 (B + 1) <= 64: the register backward sweep
        assert rows is None or B + 3 <= rows < rec["npf"], (tag, "the plan does not take these streaming rows", B, rows, rec["npf"])
    assert rec["ok_o"] == 1 and rec["ok_g"] == 1, (tag, "solver_ok", rec["ok_o"], rec["ok_g"])
    if case["solver"] == 2:
        assert rec["closest_o"] >= MIN_CLOSEST and rec["closest_g"] >= MIN_CLOSEST, (tag, "input too near a stopping threshold: take another seed", rec["closest_o"], rec["closest_g"])
        assert rec["it_g"] == rec["it_truth_g"] == rec["it_o"] == rec["it_truth_o"], (tag, "PCG iterations", rec["it_g"], rec["it_truth_g"], rec["it_o"], rec["it_truth_o"])
    assert T.within_criterion(rec["e_g"], rec["e_o"], factor, floor), (tag, "eo, eg", rec["e_o"], rec["e_g"])


def log_line(rec):
    return (f"{rec['case']:<28} {rec['seq']:<6} step {rec['step']} lambda {rec['lam']:.3e} code {rec['code']} npf {rec['npf']:>3} band {rec['band_blocks']:>2} "
            f"it o/g/truth {rec['it_o']}/{rec['it_g']}/{rec['it_truth_g']} floor_binds {int(rec['binding_g'])} closest {min(rec['closest_o'], rec['closest_g']):.3f} "
            f"eo {rec['e_o']:.3e} eg {rec['e_g']:.3e} eg/eo {rec['e_g'] / max(rec['e_o'], 1e-300):.2f}")
