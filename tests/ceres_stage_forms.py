"""The Ceres branch (Optimizer/Framework=1, both trust-region strategies) stepped stage by stage beside the oracle and held to the
extended-precision truth of tests/stage_truth.py, on the windows of tests/stage_forms.py.

TEST INFRASTRUCTURE ONLY: the case table, the stepping helper and the per-record assertions of tests/test_gpu_ceres_stage_forms.py (the
oracle side alone serves tests/test_stage_truth.py on the CPU).  A case runs one strategy on one window under one set of switches:

    lm (LEVENBERG_MARQUARDT)   linearize (iteration zero), trial at lambda = 1e-4 (the initial radius 1e4), trial at lambda = 1, commit,
                               linearize (the other estimate buffer, scaling kept), trial at 1e-4, mark_outliers
    dl (DOGLEG)                linearize, six trials — mu in (1e-8, 1e-3) times the radii 2 |gn_s|, |cauchy| / 2 and (|cauchy| + |gn_s|) / 2
                               (all three cases of the traditional dogleg must be seen) —, commit, linearize, one trial, mark_outliers

The radii come from the truth's own norms at that mu — stage_truth.dogleg_norms on the oracle's buffers after an unrecorded trial at an
unbounded radius, which leaves dn there — and are handed to the device as they are: both sides step the same inputs.  Every stage is judged on that side's own inputs (stage_truth, the table above its
Ceres section), one record per step and stage with eo, eg, n; `check_record` asserts the form, the conditions on the input (no chi2 on a
threshold, no H_ii s^2 on a clamp bound, no laser coordinate on a rounding boundary, no marginal dogleg case: take another seed / radius),
that the outlier flags are the truth's, and the criterion  eg <= FACTOR * max(eo, (64 + n) u)  of DESIGN.md 4b as it stands.
"""
import numpy as np

import solver_truth as T
import stage_forms as F
import stage_truth as ST
from helpers import graph_of
from solver_forms import custom_window, environment, make_window
from visfs_amd import abi, synth

FACTOR = T.FACTOR
MIN_CLOSEST = 1e-9                               # chi2 against delta^2 / delta, H_ii s^2 against a clamp bound (relative)
MIN_DOGLEG_MARGIN = 0.01                         # |gn_s| and alpha |g_s| against the radius
MUS = (1e-8, 1e-3)
LM_SEQ = (("linearize",), ("trial", 1e-4), ("trial", 1.0), ("commit",), ("linearize",), ("trial", 1e-4), ("mark",))


def dl_seq(last=0):
    """last: which radius the one trial after the commit takes (0: 2 |gn_s|, the full Gauss-Newton step through pass 2; 1: |cauchy| / 2)."""
    return (("linearize",),) + tuple(("dogleg", mu, r) for mu in MUS for r in (0, 1, 2)) + (("commit",), ("linearize",), ("dogleg", MUS[0], last), ("mark",))


# The laser windows take |cauchy| / 2 for the trial after the commit.  A laser coordinate within the fp64 chain's error of a rounding
# boundary is a condition on the input (stage_truth._laser_functor): of 600 coordinates one lies that near about once in thirty states, and
# after a commit each side stands on a state of its own, so the oracle's margin on the CPU says nothing of the device's (seen: 91 against
# 0.36 at 2 |gn_s|).  The gradient step of case 2 depends on b and m alone, not on the solve: both sides' candidates agree to the last
# bits and the margin found on the CPU (109 and 69) holds for the device.
LIN_BUFS = F.LIN_BUFS + (("s2p", abi.BUF_S2P), ("s2l", abi.BUF_S2L))
STAGES = dict(linearize=ST.CERES_LIN_STAGES, trial=ST.CERES_TRIAL_STAGES, dogleg=ST.DOGLEG_STAGES)


CLAMP_FAR, CLAMP_SCALE = 5, 1e6
STRIDED_LM = 4100                                # 4 landmarks per workgroup at 64 lanes: 1025 landmark partials
LIN_TRIAL = (("linearize",), ("trial", 1e-4))
LIN_DOGLEG = (("linearize",), ("dogleg", MUS[0], 0))
# iteration zero armed again: after a commit stage_begin_phase makes the next linearisation estimate the scaling from the NEW diagonals;
# a reset brings back the uploaded estimate and its linearisation the first scaling
REARM_LM = (("linearize",), ("trial", 1e-4), ("commit",), ("linearize",), ("begin",), ("linearize",), ("reset",), ("linearize",))
REARM_DL = (("linearize",), ("dogleg", MUS[0], 0), ("commit",), ("linearize",), ("begin",), ("linearize",), ("reset",), ("linearize",))


def stage_window(spec):
    if spec[0] == "hb15":
        return make_window(spec)
    if spec[0] == "clamp":
        # the small-10 window with its first five landmarks moved a million times further out: J ~ f / z, so their H_ii (already s^2 ~ 1
        # there) fall below min_lm_diagonal = 1e-6 and the damping of those variables is the clamp's 1e-6 / s^2, not H_ii
        w, kw = make_window(custom_window(10))
        w["point_xyz"] = np.array(w["point_xyz"], dtype=np.float64)
        w["point_xyz"][:CLAMP_FAR] *= CLAMP_SCALE
        return w, kw
    if spec[0] == "strided":
        return synth.make_window("custom", n_kf=6, n_lm=STRIDED_LM, n_obs=3 * STRIDED_LM, seed=5), {}
    return F.stage_window(spec)


def _case(window, env=None, expect=None):
    return dict(window=window, env=dict(env or {}), expect=dict(expect or {}))


def _build_windows():
    c = {}
    for G in (4, 8, 16, 32, 64):
        c[f"group-{G}"] = _case(("group", G), env={"VISFS_BA_GROUP": str(G)}, expect=dict(lanes_per_landmark=G))
    c["chunks"] = _case(("chunks",))
    for npf in (1, 6, 10):
        c[f"small-{npf}"] = _case(custom_window(npf), expect=dict(solver_kernel=5, n_free_poses=npf))
    for wname, wspec in (("k30", ("k30",)), ("hard", ("hard",))):
        c[f"band-{wname}"] = _case(wspec, expect=dict(solver_kernel=7))
        c[f"dense-{wname}"] = _case(wspec, env={"VISFS_BA_BAND": "0"}, expect=dict(solver_kernel=6))
        for p in (1, 2, 3):
            c[f"passes{p}-{wname}"] = _case(wspec, env={"VISFS_BA_SCH_PASSES": str(p), "VISFS_BA_SCHUR_RUNS": "0"}, expect=dict(schur_runs=0, passes=p))
        c[f"runs-{wname}"] = _case(wspec, env={"VISFS_BA_SCHUR_RUNS": "1"}, expect=dict(runs=True))
    c["band-hb15"] = _case(("hb15",), expect=dict(solver_kernel=7, n_free_poses=29, band_lds=True))
    c["laser-visual"] = dict(_case(("laser", True, F.LASER_SEED)), dl_last=1)
    c["laser-only"] = dict(_case(("laser", False, F.LASER_SEED)), dl_last=1)
    c["odo-c3"] = _case(("c3s",))
    c["odo-noroot"] = _case(("noroot",))
    c["clamp"] = _case(("clamp",), expect=dict(solver_kernel=5, n_free_poses=10, on_lower_clamp=True))
    # more landmark partials than k_ceres_lin_finalize has threads (1024) and k_dogleg_mid / k_decide have (256): their strided loops
    # take more than one round
    c["rearm"] = dict(_case(custom_window(6), expect=dict(solver_kernel=5, n_free_poses=6, rearm=True)), seq=(REARM_LM, REARM_DL))
    c["strided"] = dict(_case(("strided",), env={"VISFS_BA_GROUP": "64"}, expect=dict(lanes_per_landmark=64, landmark_partials_above=1024)), short=True)
    return c


WINDOWS = _build_windows()
CASES = {f"{s}-{n}": dict(c, strategy=s, base=n) for s in ("lm", "dl") for n, c in WINDOWS.items()}
# the windows the CPU test runs the oracle through: every window of the table, each under both strategies (the oracle does not depend on
# the device's switches)
CPU_CASES = tuple(f"{s}-{n}" for s in ("lm", "dl") for n in ("group-4", "group-8", "group-16", "group-32", "group-64", "chunks", "small-1", "small-6",
                                                              "small-10", "band-k30", "band-hard", "band-hb15", "laser-visual", "laser-only",
                                                              "odo-c3", "odo-noroot", "clamp", "rearm", "strided"))


def seq_of(case):
    if "seq" in case:
        return case["seq"][1 if case["strategy"] == "dl" else 0]
    if case.get("short"):
        return LIN_DOGLEG if case["strategy"] == "dl" else LIN_TRIAL
    return dl_seq(case.get("dl_last", 0)) if case["strategy"] == "dl" else LM_SEQ


def params_of(strategy, prm_kw=None):
    return abi.default_params(**{**dict(iterations=10, solver=0, framework=1, trust_region=1 if strategy == "dl" else 0), **(prm_kw or {})})


def graph_arrays(gb, prm):
    g = F.graph_arrays(gb, prm)
    g["ceres"] = True
    return g


# ----------------------------------------------------------------- stepping
def _fetch(side, bufs):
    return {name: side.fetch(b).copy() for name, b in bufs}


def truth_outliers(graph, pose, pt):
    """Optimizer.cpp:529-540: every stereo residual block, those between two constant blocks included, is tested with
    error . (pixelInfo error) > delta — the information value ONCE, unsquared delta.  Returns (flags, smallest relative distance from delta)."""
    e, _, _, _ = ST.stereo_edge(ST._ld(pose)[graph["obs_pose"]], ST._ld(pt)[graph["obs_point"]], graph["obs_uvr"], graph["intr"])
    c = (e * (ST.LD(graph["w_px"]) * e)).sum(axis=1)
    d = ST.LD(graph["delta"])
    if not graph["delta"] > 0 or len(c) == 0:
        return np.zeros(len(c), np.uint8), ST.INF
    return (c > d).astype(np.uint8), float(np.abs(c / d - 1).min())


def run_side(side, gb, graph, seq, radii=None):
    """Step one side through `seq`.  radii: the dogleg radii to use, one per dogleg step (None: they are computed here, from the truth's
    norms of this side's buffers).  Returns (one entry per step, the radii used)."""
    pose = gb.pose_tq.copy(); pt = gb.point_xyz.copy()
    out, used = [], []
    lin = tr = kept = first = prev = None
    probe = {}
    di = 0
    for n, step in enumerate(seq):
        kind = step[0]
        base = dict(step=n, kind=kind, lam=0.0, radius=0.0, stages={}, closest=(ST.INF, ST.INF, ST.INF), ok=1, n_out=0, flags_ok=1, case=0, dl_margin=ST.INF, n_low=0,
                    s2_vs_prev=-1, s2_vs_first=-1)
        if kind == "linearize":
            chi, gmax, xn = side.ceres_linearize()
            lin = _fetch(side, LIN_BUFS)
            stages, closest, n_low = ST.judge_ceres_linearize(graph, pose, pt, lin, chi, gmax, xn, kept)
            vs_prev = vs_first = -1
            if kept is None:                                         # an iteration zero: does its estimate differ from the one before, from the first?
                kept = (lin["s2p"].copy(), lin["s2l"].copy())
                free = ~graph["point_fixed"]
                same = lambda a: int(np.array_equal(a[0], kept[0]) and np.array_equal(a[1].reshape(-1, 3)[free], kept[1].reshape(-1, 3)[free]))
                if prev is not None:
                    vs_prev, vs_first = 1 - same(prev), 1 - same(first)
                first = first or kept
                prev = kept
            probe = {}
            out.append(dict(base, stages=stages, closest=closest, n_low=n_low, s2_vs_prev=vs_prev, s2_vs_first=vs_first))
        elif kind == "trial":
            lam = step[1]
            chi, sc, sn, ok = side.ceres_trial(lam)
            tr = _fetch(side, F.TRIAL_BUFS)
            stages, margin = ST.judge_ceres_trial(graph, pose, pt, lam, {**lin, **tr}, chi, sc, sn) if ok else ({}, ST.INF)
            out.append(dict(base, lam=float(lam), stages=stages, closest=(ST.INF, ST.INF, margin), ok=int(ok)))
        elif kind == "dogleg":
            mu, which = step[1], step[2]
            if radii is not None:
                radius = radii[di]
            else:
                if mu not in probe:                                  # an unbounded trial leaves dn at this mu in the DX buffers; the norms are the truth's
                    p = side.dogleg_stage(1e300, mu)
                    assert p["ok"] == 1.0 and p["A"] == 0.0 and p["B"] == 1.0
                    probe[mu] = ST.dogleg_norms(graph, pose, pt, {**lin, **_fetch(side, F.TRIAL_BUFS)})
                gn, cauchy = probe[mu]
                radius = float((2 * gn, cauchy / 2, (cauchy + gn) / 2)[which])
            di += 1; used.append(radius)
            res = side.dogleg_stage(radius, mu)
            ok = int(res["ok"] == 1.0)
            tr = _fetch(side, F.TRIAL_BUFS)
            stages, margin, case, dl_margin = ST.judge_dogleg(graph, pose, pt, radius, mu, {**lin, **tr}, res) if ok else ({}, ST.INF, 0, ST.INF)
            out.append(dict(base, lam=float(mu), radius=radius, stages=stages, closest=(ST.INF, ST.INF, margin), ok=ok, case=case, dl_margin=dl_margin))
        elif kind == "commit":
            side.commit()
            pose = tr["pose_trial"].reshape(-1, 7).copy(); pt = tr["point_trial"].reshape(-1, 3).copy()
            out.append(None)
        elif kind == "begin":
            side.begin_phase()
            kept = None
            out.append(None)
        elif kind == "reset":
            side.reset()
            pose = gb.pose_tq.copy(); pt = gb.point_xyz.copy()
            kept = None
            out.append(None)
        elif kind == "mark":
            side.mark_outliers()
            flags = np.asarray(side.download()[2]).astype(np.uint8)
            want, closest = truth_outliers(graph, pose, pt)
            out.append(dict(base, closest=(ST.INF, closest, ST.INF), n_out=int(flags.sum()), flags_ok=int(np.array_equal(flags, want))))
        else:
            raise KeyError(kind)
    return out, used


_oracle_cache = {}


def oracle_steps(olib, name):
    """The oracle's side of case `name`, once per (window, strategy, sequence)."""
    import oracle_lib
    case = CASES[name]
    key = (case["window"], case["strategy"], seq_of(case))
    if key not in _oracle_cache:
        w, prm_kw = stage_window(case["window"])
        prm = params_of(case["strategy"], prm_kw)
        wb, gb, *_ = graph_of(olib.oracle_pack_window, prm, w)
        graph = graph_arrays(gb, prm)
        o = oracle_lib.OracleSystem(olib, prm, gb)
        try:
            steps, radii = run_side(o, gb, graph, seq_of(case))
        finally:
            o.close()
        _oracle_cache[key] = (prm, wb, gb, graph, steps, radii, o.npf)
    return _oracle_cache[key]


def records_of(name, osteps, gsteps, info):
    """One record per step and stage (and one per mark_outliers step)."""
    recs = []
    for so, sg in zip(osteps, gsteps):
        ref = sg if sg is not None else so
        if ref is None:
            continue
        both = [s for s in (so, sg) if s is not None]
        base = dict(case=name, step=ref["step"], kind=ref["kind"], lam=ref["lam"], radius=ref["radius"], info=info,
                    ok=min(s["ok"] for s in both), n_out=[s["n_out"] for s in both], flags_ok=min(s["flags_ok"] for s in both),
                    closest=min(min(s["closest"][:2]) for s in both), laser_margin=min(s["closest"][2] for s in both),
                    dl_case=[s["case"] for s in both], dl_margin=min(s["dl_margin"] for s in both), n_low=[s["n_low"] for s in both],
                    s2_vs_prev=[s["s2_vs_prev"] for s in both], s2_vs_first=[s["s2_vs_first"] for s in both])
        if ref["kind"] == "mark":
            recs.append(dict(base, stage="mark", n=0, e_o=0.0, e_g=0.0))
            continue
        for st in STAGES[ref["kind"]]:
            a = so["stages"].get(st) if so else None
            b = sg["stages"].get(st) if sg else None
            src = b or a
            if src is None:
                recs.append(dict(base, stage=st, n=0, e_o=ST.INF, e_g=ST.INF))         # (a failed solve: check_record says so)
                continue
            rec = dict(base, stage=st, n=src["n"], e_o=a["e"] if a else 0.0, e_g=b["e"] if b else None, block_g=b["block"] if b else -1)
            if st == "S":
                rec.update(cond=src["cond"], cancel_o=a["cancel"] if a else 1.0, e_mag_o=a["e_mag"] if a else 0.0, e_mag_g=b["e_mag"] if b else None)
            recs.append(rec)
    return recs


def run_oracle_case(olib, name):
    """Case `name` on the oracle alone (the CPU test): records with e_g = None."""
    prm, wb, gb, graph, osteps, radii, npf = oracle_steps(olib, name)
    return records_of(name, osteps, [None] * len(osteps), dict(n_free_poses=npf))


def run_case(olib, name):
    """Case `name` on a device / oracle pair: the records, each with what describe() said."""
    from visfs_amd import backend
    case = CASES[name]
    prm, wb, gb, graph, osteps, radii, npf_o = oracle_steps(olib, name)
    F.check_window(case["base"], gb, graph)
    with environment(case["env"]):
        s = backend.Solver(prm)
        try:
            s.upload(gb)
            info = s.describe()
            info["npf_o"] = npf_o
            info["own_run_lr"] = None
            if "passes" in case["expect"]:
                info["chunks_expected"] = [F.schur_chunks(graph, p) for p in (1, 2, 3)]
            gsteps, _ = run_side(s, gb, graph, seq_of(case), radii=radii)
        finally:
            s.close()
    return records_of(name, osteps, gsteps, info)


def check_form(name, info):
    """The form that ran is the one the case names."""
    exp = CASES[name]["expect"]
    F.check_form(name, info, exp)
    if "landmark_partials_above" in exp:         # what the plan reports: one partial per workgroup of the landmark-major passes
        assert info["landmark_partials"] > exp["landmark_partials_above"], (name, "landmark partials", info["landmark_partials"])
    if exp.get("band_lds"):
        assert info["band_blocks"] > 9, (name, "band_blocks", info["band_blocks"])    # 6 (B + 1) > 64: the LDS backward sweep of k_band_chol


def check_sequence(name, records):
    """A DOGLEG case has seen all three cases of the dogleg, on both sides alike; the clamp case has variables on the lower clamp."""
    if CASES[name]["expect"].get("on_lower_clamp"):
        low = [r["n_low"] for r in records if r["kind"] == "linearize" and r["stage"] == "s2l"]
        assert low and all(min(v) >= 3 * CLAMP_FAR for v in low), (name, "variables on the lower clamp", low)
    if CASES[name]["expect"].get("rearm"):
        lins = [r for r in records if r["kind"] == "linearize" and r["stage"] == "s2p"]
        assert len(lins) == 4, (name, len(lins))
        kept, begun, reset = lins[1], lins[2], lins[3]
        assert set(kept["s2_vs_prev"]) == {-1}, (name, "the linearisation after the commit estimated the scaling again")
        assert set(begun["s2_vs_prev"]) == {1} and set(begun["s2_vs_first"]) == {1}, (name, "begin_phase: the scaling was not estimated from the new diagonals", begun["s2_vs_prev"])
        assert set(reset["s2_vs_prev"]) == {1} and set(reset["s2_vs_first"]) == {0}, (name, "reset: the scaling is not the first one again", reset["s2_vs_prev"], reset["s2_vs_first"])
    if CASES[name]["strategy"] != "dl" or CASES[name].get("short") or "seq" in CASES[name]:
        return
    seen = [tuple(r["dl_case"]) for r in records if r["kind"] == "dogleg" and r["stage"] == "A"]
    assert all(len(set(c)) == 1 for c in seen), (name, "the sides took different dogleg cases", seen)
    assert {c[0] for c in seen} == {1, 2, 3}, (name, "dogleg cases seen", seen)


def check_record(rec, device=True):
    """The assertions of one record."""
    name = rec["case"]
    tag = (name, rec["step"], rec["kind"], rec["stage"])
    if device:
        check_form(name, rec["info"])
    assert rec["closest"] >= MIN_CLOSEST, (tag, "a chi2 sits on a threshold or an H_ii s^2 on a clamp bound: take another seed", rec["closest"])
    assert rec["laser_margin"] >= 1.0, (tag, "a laser point's grid coordinate sits on an fp64 rounding boundary: take another seed", rec["laser_margin"])
    assert rec["dl_margin"] >= MIN_DOGLEG_MARGIN, (tag, "the dogleg case is marginal: take another radius", rec["dl_margin"])
    assert rec["ok"] == 1, (tag, "solver_ok")
    if rec["stage"] == "mark":
        assert rec["flags_ok"] == 1 and len(set(rec["n_out"])) == 1, (tag, "outlier flags against the truth's", rec["n_out"])
        return
    assert T.within_criterion(rec["e_g"], rec["e_o"], FACTOR, ST.floor_of(rec["n"])), (tag, "eo, eg, floor", rec["e_o"], rec["e_g"], ST.floor_of(rec["n"]), "block", rec.get("block_g"))


def log_lines(records):
    """The records of one case, one line per step (profiles/ceres_stage_truth.log): the form describe() reported, lambda (LM) or mu, radius
    and the dogleg case, then for every stage  name n eo eg ratio  (S: also eo / eg on sum|terms| and cond of the worst landmark)."""
    out = []
    for step in sorted({r["step"] for r in records}):
        recs = [r for r in records if r["step"] == step]
        i = recs[0]["info"]
        head = (f"{recs[0]['case']} step {step} {recs[0]['kind']} lanes {i.get('lanes_per_landmark', 0)} chunks {i.get('n_schur_chunks', 0)} runs {i.get('schur_runs', 0)}x{i.get('schur_run_landmarks', 0)} "
                f"code {i.get('solver_kernel', 0)} npf {i.get('n_free_poses', 0)}")
        if recs[0]["stage"] == "mark":
            out.append(f"{head} | mark outliers {'/'.join(str(v) for v in recs[0]['n_out'])} flags {'as the truth' if recs[0]['flags_ok'] else 'DIFFER'}")
            continue
        if recs[0]["kind"] == "dogleg":
            head += f" mu {recs[0]['lam']:.1e} radius {recs[0]['radius']:.6e} case {'/'.join(str(v) for v in recs[0]['dl_case'])}"
        elif recs[0]["kind"] == "trial":
            head += f" lambda {recs[0]['lam']:.1e}"
        else:
            head += f" on-lower-clamp {'/'.join(str(v) for v in recs[0]['n_low'])}"
        parts = []
        for r in recs:
            eg = r["e_g"]
            part = f"{r['stage']} {r['n']} {r['e_o']:.1e} {'-' if eg is None else format(eg, '.1e')} {'-' if eg is None else format(eg / max(r['e_o'], ST.floor_of(r['n'])), '.2f')}"
            if r["stage"] == "S":
                em = r["e_mag_g"]
                part += f" ({r['e_mag_o']:.1e} {'-' if em is None else format(em, '.1e')} cond {r['cond']:.1e})"
            parts.append(part)
        out.append(f"{head} | " + "; ".join(parts))
    return out
