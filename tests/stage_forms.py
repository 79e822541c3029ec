"""Every linearisation, Schur and back-substitution form, stepped beside the oracle and held to the extended-precision truth of
tests/stage_truth.py.

TEST INFRASTRUCTURE ONLY: the case table, the stepping helper and the per-record assertions of tests/test_gpu_stage_forms.py (the oracle
side alone serves tests/test_stage_truth.py on the CPU).  `run_case` steps a device / oracle pair through
    linearize, trial(1e-5 md), trial(md), commit, linearize (the other sel / lin_sel buffer set), mark_outliers, linearize (level-1 edges:
    weight 0, tile 0, absent from every sum), trial
fetches every stage buffer of each side after each step and has stage_truth judge every stage ON THAT SIDE'S OWN INPUTS; one record per
step and stage with eo, eg, n and what describe() said.  `check_record` asserts that the form the case names is the one that ran, that
both sides marked the same number of outliers, that no observation sits on a threshold of a discrete decision, and the criterion
    eg <= FACTOR * max(eo, (64 + n) u).
"""
import os
import re

import numpy as np

import solver_truth as T
import stage_truth as ST
from helpers import drop_refs, graph_of, hard_window
from solver_forms import ILL_SEEDS, custom_window, environment, make_window
from visfs_amd import abi, synth

FACTOR = T.FACTOR
MIN_CLOSEST = 1e-9                               # an active chi2 nearer than this (relative) to delta^2 or delta: take another seed
FULL = (("linearize", 0), ("trial", 1e-5), ("trial", 1.0), ("commit", 0), ("linearize", 0), ("mark", 0), ("linearize", 0), ("trial", 1e-5))
ABS = (("linearize", 0), ("abs", 1e-2), ("abs", 1e-5))       # the ill-conditioned seeds at their absolute lambdas
LIN_S = (("linearize", 0), ("trial", 1e-5))                  # 841 poses: linearisation and one trial (S is compared on its block set, as everywhere)
LIN_BUFS = (("err", abi.BUF_OBS_ERR), ("chi2", abi.BUF_OBS_CHI2), ("weight", abi.BUF_OBS_WEIGHT), ("Hpl", abi.BUF_HPL), ("Hll", abi.BUF_HLL),
            ("bl", abi.BUF_BL), ("Hpp", abi.BUF_HPP), ("bp", abi.BUF_BP))
TRIAL_BUFS = (("S", abi.BUF_S), ("bs", abi.BUF_BS), ("dx_pose", abi.BUF_DX_POSE), ("dx_point", abi.BUF_DX_POINT),
              ("pose_trial", abi.BUF_POSE_TRIAL), ("point_trial", abi.BUF_POINT_TRIAL))
SWITCHES = ("VISFS_BA_GROUP", "VISFS_BA_SCH_PASSES", "VISFS_BA_SCHUR_RUNS", "VISFS_BA_RUN_LR", "VISFS_BA_RUN_M", "VISFS_BA_FIN_PCG",
            "VISFS_BA_FIN_ARRIVE", "VISFS_BA_PCG_CU", "VISFS_BA_PCG1", "VISFS_BA_SMALL_SOLVE", "VISFS_BA_BAND", "VISFS_BA_BAND_ROWS",
            "VISFS_BA_FUSED", "VISFS_BA_SPEC")


def lin_chunk():
    """LIN_CHUNK of visfs_amd/csrc/ba_limits.hpp: observations per pose-major workgroup."""
    path = os.path.join(os.path.dirname(os.path.abspath(abi.__file__)), "csrc", "ba_limits.hpp")
    with open(path) as f:
        return int(re.search(r"constexpr\s+int\s+LIN_CHUNK\s*=\s*(\d+)", f.read()).group(1))


# ----------------------------------------------------------------- windows
GROUP_KF, GROUP_LM = 41, 61
CHUNK_COUNTS = (0, 1, 255, 256, 257, 513)
LASER_SEED = 7                                   # (seeds 1, 4 and 6 bring a laser coordinate within the fp64 chain's error of a rounding boundary)


def group_tracks(G):
    """Track lengths of the 61 landmarks of the lanes-per-landmark window for G lanes: 0, 1, G-1, G, G+1, 2G+1 where <= 40 (G = 64, which
    allows no loop: 1, 33, 40), the rest ragged between 2 and 40.  Landmarks 58, 59, 60 are the fixed / free combinations."""
    first = [0, 1, 33, 40] if G == 64 else [0, 1] + [n for n in (G - 1, G, G + 1, 2 * G + 1) if n <= 40]
    rng = np.random.default_rng(100 + G)
    lengths = np.concatenate([first, rng.integers(2, 41, GROUP_LM - len(first))]).astype(np.int64)
    return lengths, first


def _root_index(w):
    return int(np.nonzero(np.asarray(w["pose_ids"]) == w["root_id"])[0][0])


def group_window(G):
    """41 key-frames, 61 landmarks: 256 / G landmarks per workgroup leave the last workgroup partial for every G.  Landmark 58 is fixed
    and seen from free poses, 59 is free and seen only from the fixed pose, 60 is fixed and seen only from the fixed pose."""
    w = synth.make_window("custom", n_kf=GROUP_KF, n_lm=GROUP_LM, n_obs=GROUP_LM * 40, seed=31, fixed_frac=0.0)
    lengths, _ = group_tracks(G)
    ids = np.asarray(w["point_ids"]); feat = np.searchsorted(ids, np.asarray(w["ref_feature"]))
    root_id = np.asarray(w["pose_ids"])[_root_index(w)]
    keep = np.zeros(len(feat), bool)
    for l in range(GROUP_LM):
        idx = np.nonzero(feat == l)[0]
        if l in (59, 60):
            idx = idx[np.asarray(w["ref_pose"])[idx] == root_id]
            assert len(idx) == 1
        elif l == 58:
            idx = idx[np.asarray(w["ref_pose"])[idx] != root_id][:7]
        else:
            idx = idx[len(idx) - lengths[l]:] if lengths[l] else idx[:0]          # (the LAST observations: the root, first in time, is left to 59 and 60)
        keep[idx] = True
    w = drop_refs(w, keep)
    fixed = np.zeros(GROUP_LM, np.uint8); fixed[[58, 60]] = 1
    w["point_fixed"] = fixed
    return w


def chunk_window():
    """Seven key-frames, 520 landmarks: the six free poses see exactly 0, 1, 255, 256, 257 and 513 observations (no chunk, one, one
    chunk less one, a full chunk, a chunk plus one, three chunks); the fixed pose sees every landmark."""
    n_lm = 520
    w = synth.make_window("custom", n_kf=7, n_lm=n_lm, n_obs=7 * n_lm, seed=77, fixed_frac=0.0, odo=False)
    ids = np.asarray(w["point_ids"]); feat = np.searchsorted(ids, np.asarray(w["ref_feature"]))
    pose_ids = np.asarray(w["pose_ids"]); root = _root_index(w)
    free = [i for i in range(7) if i != root]
    want = {pose_ids[root]: n_lm}
    want.update({pose_ids[p]: c for p, c in zip(free, CHUNK_COUNTS)})
    limit = np.array([want[p] for p in np.asarray(w["ref_pose"])])
    return drop_refs(w, feat < limit)


def big_window():
    """841 key-frames (one more than the landmark kernels stage as R|t in LDS), 3 landmarks per key-frame, tracks of 2 .. 4."""
    n_kf = 841; n_lm = 3 * n_kf
    w = synth.make_window("custom", n_kf=n_kf, n_lm=n_lm, n_obs=4 * n_lm, seed=17)
    ids = np.asarray(w["point_ids"]); feat = np.searchsorted(ids, np.asarray(w["ref_feature"]))
    first = np.r_[True, feat[1:] != feat[:-1]]
    pos = np.arange(len(feat)) - np.maximum.accumulate(np.where(first, np.arange(len(feat)), 0))
    return drop_refs(w, pos < 2 + feat % 3)


def stage_window(spec):
    """(window dict, parameter keywords) of a case's window."""
    kind = spec[0]
    if kind in ("custom", "sparse", "ill"):
        return make_window(spec)
    if kind == "group":
        return group_window(spec[1]), {}
    if kind == "chunks":
        return chunk_window(), {}
    if kind == "big":
        return big_window(), {}
    if kind == "C1":
        return synth.make_window("C1"), {}
    if kind == "c3s":                            # C3 (wheel odometry) at the shape of the parity tests
        return synth.make_window("C3", n_kf=12, n_lm=300, n_obs=2400), {}
    if kind == "noroot":                         # the root id lies outside the window: no fixed pose, every odometry edge has two free ends
        w = synth.make_window("C3", n_kf=12, n_lm=300, n_obs=2400)
        w["root_id"] = 10 ** 6
        return w, {}
    if kind == "laser":
        return synth.make_laser_window(n_kf=6, with_visual=spec[1], n_points=300, seed=spec[2]), {}
    if kind == "k30":
        return synth.make_window("custom", n_kf=30, n_lm=800, n_obs=8000, seed=11), {}
    if kind == "hard":
        return hard_window(), {}
    raise KeyError(kind)


def graph_arrays(gb, prm):
    """The plain arrays stage_truth takes, from a packed graph and its parameters."""
    g = gb.struct
    laser = None
    if g.n_laser > 0 and gb.grid is not None:
        gs = gb.grid.struct
        laser = dict(pose=int(g.laser_pose), xyz=gb.laser_xyz.copy(), Tcr=np.array(list(g.Tcr)), resolution=gs.resolution, max_x=gs.max_x,
                     max_y=gs.max_y, cost=gb.grid.cost.copy())
    return dict(pose_fixed=gb.pose_fixed.astype(bool), point_fixed=gb.point_fixed.astype(bool), obs_point=gb.obs_point.copy(),
                obs_pose=gb.obs_pose.copy(), obs_uvr=gb.obs_uvr.copy(), odo_from=gb.odo_from.copy(), odo_to=gb.odo_to.copy(),
                odo_tq=gb.odo_tq.copy(), intr=(g.fx, g.fy, g.cx, g.cy, g.bf), w_px=1.0 / prm.pixel_variance,
                w_odo=1.0 / prm.odometry_covariance, w_laser=1.0 / prm.laser_covariance, delta=float(prm.robust_kernel_delta), laser=laser)


def schur_chunks(g, passes):
    """The chunks the pair-list gather must have for `passes` passes: sum over the blocks of S of ceil(pairs / (64 passes)), a pair being
    two observations of one free landmark from free poses i <= j (an observation with itself on the diagonal) — counted on the packed graph."""
    pidx = ST.pose_index(g)
    op = np.asarray(g["obs_pose"], dtype=np.int64); ol = np.asarray(g["obs_point"], dtype=np.int64)
    el = np.nonzero((pidx[op] >= 0) & ~g["point_fixed"][ol] if len(op) else np.zeros(0, bool))[0]
    el = el[np.lexsort((pidx[op[el]], ol[el]))]
    lm = ol[el]; pi = pidx[op[el]]; npf = int(pidx.max()) + 1
    keys = []
    for d in range(int(np.bincount(lm).max()) if len(lm) else 0):
        k1 = np.arange(len(el) - d); k2 = k1 + d
        ok = lm[k1] == lm[k2]
        keys.append(pi[k1[ok]] * npf + pi[k2[ok]])
    if not keys:
        return 0
    _, cnt = np.unique(np.concatenate(keys), return_counts=True)
    return int(((cnt + 64 * passes - 1) // (64 * passes)).sum())


def check_window(name, gb, g):
    """The structural claims of case `name`, asserted on the packed graph before anything is compared."""
    fixed = gb.pose_fixed.astype(bool)
    if name.startswith("group-"):
        G = int(name.split("-")[1])
        lengths, first = group_tracks(G)
        track = np.bincount(gb.obs_point, minlength=GROUP_LM)
        assert gb.n_poses == GROUP_KF and gb.n_points == GROUP_LM and GROUP_LM % (256 // G) != 0, name       # the last workgroup is partial
        assert list(track[:len(first)]) == first and list(track[:58]) == list(lengths[:58]) and list(track[58:]) == [7, 1, 1], (name, track)
        assert fixed.sum() == 1 and list(gb.point_fixed[58:]) == [1, 0, 1], name
        root = int(np.nonzero(fixed)[0][0])
        assert not (gb.obs_pose[gb.obs_point == 58] == root).any() and (gb.obs_pose[gb.obs_point >= 59] == root).all(), name
    elif name == "chunks":
        L = lin_chunk()
        per_pose = np.bincount(gb.obs_pose, minlength=gb.n_poses)[~fixed]
        assert L == 256 and sorted(per_pose.tolist()) == sorted(CHUNK_COUNTS) == [0, 1, L - 1, L, L + 1, 2 * L + 1], (name, per_pose)
    elif name == "poses-841":
        track = np.bincount(gb.obs_point, minlength=gb.n_points)
        assert gb.n_poses == 841 and gb.n_points == 3 * 841 and set(track.tolist()) == {2, 3, 4}, name
    elif name == "odo-noroot":
        assert fixed.sum() == 0 and len(gb.odo_from) == 11, name
    elif name == "odo-c3":
        ends = fixed[gb.odo_from].astype(int) + fixed[gb.odo_to].astype(int)
        assert (ends == 1).any() and (ends == 0).any() and (gb.n_poses, gb.n_points, gb.n_obs) == (12, 300, 2400), name
    elif name == "laser-only":
        assert gb.n_points == 0 and gb.n_obs == 0 and g["laser"] is not None and len(g["laser"]["xyz"]) == 300, name
    elif name == "laser-visual":
        assert gb.n_points > 0 and gb.n_obs > 0 and g["laser"] is not None and not fixed[g["laser"]["pose"]], name
    elif name.endswith("-k30"):
        assert (gb.n_poses, gb.n_points, gb.n_obs) == (30, 800, 8000), name
    elif name.endswith("-hard"):
        assert (gb.n_poses, gb.n_points, gb.n_obs) == (20, 400, 4000) and gb.point_fixed.sum() == 0, name
    elif name.startswith("small-") or name.startswith("pcg-cu-"):
        assert (~fixed).sum() == int(name.split("-")[-1]), name


# ----------------------------------------------------------------- the case table
def _case(window, seq=FULL, prm=None, env=None, expect=None, oracle_prm=None, factor=None):
    return dict(window=window, seq=seq, prm=dict(prm or {}), env=dict(env or {}), expect=dict(expect or {}), oracle_prm=dict(oracle_prm or {}),
                factor=dict(factor or {}))


def _build_cases():
    c = {}
    for G in (4, 8, 16, 32, 64):
        c[f"group-{G}"] = _case(("group", G), env={"VISFS_BA_GROUP": str(G)}, expect=dict(lanes_per_landmark=G))
    c["chunks"] = _case(("chunks",))
    # (the oracle's scalar Cholesky of 5040 rows takes half a minute: its side solves this window with its PCG.  Every stage is judged on
    #  the side's own dx_pose, so the solver does not enter; the device runs solver=0 as the case says)
    c["poses-841"] = _case(("big",), seq=LIN_S, prm=dict(solver=0), oracle_prm=dict(solver=2), expect=dict(n_free_poses=840))
    c["odo-c3"] = _case(("c3s",))
    c["odo-noroot"] = _case(("noroot",))
    c["laser-visual"] = _case(("laser", True, LASER_SEED))
    c["laser-only"] = _case(("laser", False, LASER_SEED))
    for wname, wspec in (("k30", ("k30",)), ("hard", ("hard",))):
        for p in (1, 2, 3):
            c[f"passes{p}-{wname}"] = _case(wspec, env={"VISFS_BA_SCH_PASSES": str(p), "VISFS_BA_SCHUR_RUNS": "0"}, expect=dict(schur_runs=0, passes=p))
        c[f"runs-{wname}"] = _case(wspec, env={"VISFS_BA_SCHUR_RUNS": "1"}, expect=dict(runs=True))
        for lr in (8, 64):
            for m in (1, 4):
                c[f"runs-lr{lr}-m{m}-{wname}"] = _case(wspec, env={"VISFS_BA_SCHUR_RUNS": "1", "VISFS_BA_RUN_LR": str(lr), "VISFS_BA_RUN_M": str(m)},
                                                       expect=dict(runs=True, run_lr=lr, run_m=m))
        c[f"finalize-{wname}"] = _case(wspec, env={"VISFS_BA_SCHUR_RUNS": "0", "VISFS_BA_FIN_PCG": "0"}, expect=dict(schur_runs=0, finalize_launches=True))
        c[f"fin-pcg-{wname}"] = _case(wspec, env={"VISFS_BA_SCHUR_RUNS": "0", "VISFS_BA_FIN_PCG": "1"}, expect=dict(schur_runs=0, finalize_launches=False, solver_kernel=1))
    for npf in (1, 6, 10):
        c[f"small-{npf}"] = _case(custom_window(npf), expect=dict(solver_kernel=5, n_free_poses=npf))
    c["pcg-cu-32"] = _case(custom_window(32), env={"VISFS_BA_PCG_CU": "1"}, expect=dict(solver_kernel=4, n_free_poses=32))
    for seed in ILL_SEEDS:
        c[f"ill{seed}"] = _case(("ill", seed), seq=ABS, prm=dict(solver=0), env={"VISFS_BA_SCHUR_RUNS": "0"}, expect=dict(schur_runs=0))
        c[f"ill{seed}-runs"] = _case(("ill", seed), seq=ABS, prm=dict(solver=0), env={"VISFS_BA_SCHUR_RUNS": "1"}, expect=dict(runs_if_admitted=True))
    c["no-kernel-C1"] = _case(("C1",), prm=dict(robust_kernel_delta=0.0))
    c["gauss-newton-C1"] = _case(("C1",), prm=dict(trust_region=1))
    return c


CASES = _build_cases()
# the windows the CPU test runs the oracle through (every window of the table; the 841-pose one with its PCG on the oracle's side)
CPU_CASES = ("group-4", "group-8", "group-16", "group-32", "group-64", "chunks", "poses-841", "odo-c3", "odo-noroot", "laser-visual", "laser-only",
             "finalize-k30", "finalize-hard", "small-1", "small-6", "small-10", "pcg-cu-32") + tuple(f"ill{s}" for s in ILL_SEEDS) + \
            ("no-kernel-C1", "gauss-newton-C1")


# ----------------------------------------------------------------- stepping
def _fetch(side, bufs):
    return {name: side.fetch(b).copy() for name, b in bufs}


def run_side(side, gb, graph, seq, lams=None):
    """Step one side through `seq`.  lams: the lambdas of the trial steps (None: f * this side's max_diag, or f as given for "abs").
    Returns (one entry per step, the lambdas used)."""
    pose = gb.pose_tq.copy(); pt = gb.point_xyz.copy(); level = np.zeros(gb.n_obs, np.uint8)
    out, used = [], []
    lin = tr = md = None
    ti = 0
    for n, (kind, f) in enumerate(seq):
        if kind == "linearize":
            chi, md = side.linearize()
            lin = _fetch(side, LIN_BUFS)
            stages, closest = ST.judge_linearize(graph, pose, pt, level, lin, chi, md)
            out.append(dict(step=n, kind=kind, lam=0.0, stages=stages, closest=closest, ok=1, n_out=0))
        elif kind in ("trial", "abs"):
            lam = lams[ti] if lams is not None else (f * md if kind == "trial" else f)
            ti += 1; used.append(lam)
            side.begin_phase()
            chi, sc, _, ok = side.trial(lam)
            tr = _fetch(side, TRIAL_BUFS)
            stages, margin = ST.judge_trial(graph, pose, pt, level, lam, {**lin, **tr}, chi, sc) if ok else ({}, ST.INF)
            out.append(dict(step=n, kind=kind, lam=float(lam), stages=stages, closest=(ST.INF, ST.INF, margin), ok=int(ok), n_out=0))
        elif kind == "commit":
            side.commit()
            pose = tr["pose_trial"].reshape(-1, 7).copy(); pt = tr["point_trial"].reshape(-1, 3).copy()
            out.append(None)
        elif kind == "mark":
            side.mark_outliers()
            flags = np.asarray(side.download()[2]).astype(np.uint8)
            out.append(dict(step=n, kind=kind, lam=0.0, stages={}, closest=(ST.INF, ST.INF, ST.INF), ok=1, n_out=int(flags.sum()) - int(level.sum())))
            level = flags.copy()
        else:
            raise KeyError(kind)
    return out, used


_oracle_cache = {}


def oracle_steps(olib, name):
    """The oracle's side of case `name`, once per (window, parameters, sequence): it does not depend on the device's switches."""
    import oracle_lib
    case = CASES[name]
    key = (case["window"], tuple(sorted(case["prm"].items())), case["seq"])
    if key not in _oracle_cache:
        w, prm_kw = stage_window(case["window"])
        prm = abi.default_params(**{**dict(iterations=10, solver=2), **prm_kw, **case["prm"]})
        wb, gb, *_ = graph_of(olib.oracle_pack_window, prm, w)
        graph = graph_arrays(gb, prm)
        prm_o = abi.default_params(**{**dict(iterations=10, solver=2), **prm_kw, **case["prm"], **case["oracle_prm"]})
        o = oracle_lib.OracleSystem(olib, prm_o, gb)
        try:
            steps, lams = run_side(o, gb, graph, case["seq"])
        finally:
            o.close()
        _oracle_cache[key] = (prm, wb, gb, graph, steps, lams, o.npf)
    return _oracle_cache[key]


def records_of(name, osteps, gsteps, info):
    """One record per step and stage (and one per mark_outliers step)."""
    recs = []
    for so, sg in zip(osteps, gsteps):
        ref = sg if sg is not None else so
        if ref is None:
            continue
        base = dict(case=name, step=ref["step"], kind=ref["kind"], lam=ref["lam"], info=info,
                    ok_o=so["ok"] if so else 1, ok_g=sg["ok"] if sg else 1, n_out_o=so["n_out"] if so else 0, n_out_g=sg["n_out"] if sg else 0,
                    closest=min((so or ref)["closest"][:2] + (sg or ref)["closest"][:2]), laser_margin=min((so or ref)["closest"][2], (sg or ref)["closest"][2]))
        if ref["kind"] == "mark":
            recs.append(dict(base, stage="mark", n=0, e_o=0.0, e_g=0.0))
            continue
        stages = ST.LIN_STAGES if ref["kind"] == "linearize" else ST.TRIAL_STAGES
        for st in stages:
            a = so["stages"].get(st) if so else None
            b = sg["stages"].get(st) if sg else None
            src = b or a
            if src is None:
                recs.append(dict(base, stage=st, n=0, e_o=ST.INF, e_g=ST.INF))         # (a failed solve: check_record says so)
                continue
            rec = dict(base, stage=st, n=src["n"], e_o=a["e"] if a else 0.0, e_g=b["e"] if b else None, block_o=a["block"] if a else -1,
                       block_g=b["block"] if b else -1)
            if st == "S":
                rec.update(cond=src["cond"], cancel_o=a["cancel"] if a else 1.0, e_mag_o=a["e_mag"] if a else 0.0, e_mag_g=b["e_mag"] if b else None, residual=src["residual"])
            recs.append(rec)
    return recs


def run_oracle_case(olib, name):
    """Case `name` on the oracle alone (the CPU test): records with e_g = None."""
    prm, wb, gb, graph, osteps, lams, npf = oracle_steps(olib, name)
    return records_of(name, osteps, [None] * len(osteps), dict(n_free_poses=npf))


def run_case(olib, name):
    """Case `name` on a device / oracle pair: the records, each with what describe() said."""
    from visfs_amd import backend
    case = CASES[name]
    prm, wb, gb, graph, osteps, lams, npf_o = oracle_steps(olib, name)
    check_window(name, gb, graph)
    own_lr = None
    if "run_lr" in case["expect"]:               # the plan's own run length: with one sub-batch per workgroup describe() reports it as it is
        with environment({"VISFS_BA_SCHUR_RUNS": "1", "VISFS_BA_RUN_M": "1"}):
            s = backend.Solver(prm)
            try:
                s.upload(gb)
                own_lr = s.describe()["schur_run_landmarks"]
            finally:
                s.close()
    with environment(case["env"]):
        s = backend.Solver(prm)
        try:
            s.upload(gb)
            info = s.describe()
            info["npf_o"] = npf_o
            info["own_run_lr"] = own_lr
            if "passes" in case["expect"]:
                info["chunks_expected"] = [schur_chunks(graph, p) for p in (1, 2, 3)]
            gsteps, _ = run_side(s, gb, graph, case["seq"], lams=lams)
            if "finalize_launches" in case["expect"]:
                # describe() does not say where S is finalised and the profile counts launches of optimize() only: the resident graph
                # is optimised once more under the profile (stage_trial and optimize() follow the same flag of the upload's plan)
                s.reset(); s.profile_enable(True)
                s.optimize()
                prof = s.profile_read()
                info["finalize_launches"] = int(prof.get("k_schur_finalize", {}).get("launches", 0))
                info["schur_launches"] = int(prof.get("k_schur_partial", {}).get("launches", 0))
        finally:
            s.close()
    return records_of(name, osteps, gsteps, info)


def check_form(name, info, exp=None):
    """The form that ran is the one the case names (exp: the expectations of a case of another table, tests/ceres_stage_forms.py)."""
    exp = CASES[name]["expect"] if exp is None else exp
    assert info["n_free_poses"] == info["npf_o"], (name, "n_free_poses", info["n_free_poses"], info["npf_o"])
    for key in ("lanes_per_landmark", "solver_kernel", "n_free_poses", "schur_runs"):
        if key in exp:
            assert info[key] == exp[key], (name, key, info[key])
    admitted = info["n_free_poses"] > 10
    if exp.get("runs") or (exp.get("runs_if_admitted") and admitted):
        assert info["schur_runs"] >= 1 and info["n_schur_chunks"] == 0 and info["schur_run_landmarks"] >= 8, (name, "k_schur_runs did not run", info)
    if exp.get("runs_if_admitted") and not admitted:
        assert info["schur_runs"] == 0, (name, info)
    if "run_m" in exp:                           # a requested run length is taken when it is below the plan's own (never above what fits)
        own = info["own_run_lr"]
        assert own in (8, 16, 32, 64), (name, "the plan's own run length", own)
        assert info["schur_run_landmarks"] == min(exp["run_lr"], own) * exp["run_m"], (name, "run length", info["schur_run_landmarks"], own)
    if "passes" in exp:                          # the chunk count the packed graph gives for these passes, and for no other number of passes
        want = info["chunks_expected"]
        assert len(set(want)) == 3 and info["schur_runs"] == 0 and info["n_schur_chunks"] == want[exp["passes"] - 1], (name, "Schur chunks", info["n_schur_chunks"], want)
    if "finalize_launches" in exp:
        assert info["schur_launches"] > 0 and (info["finalize_launches"] > 0) == exp["finalize_launches"], (name, "k_schur_finalize launches", info["finalize_launches"], info["schur_launches"])


def check_record(rec, device=True):
    """The assertions of one record."""
    name = rec["case"]
    tag = (name, rec["step"], rec["kind"], rec["stage"])
    if device:
        check_form(name, rec["info"])
    assert rec["closest"] >= MIN_CLOSEST, (tag, "an observation's chi2 sits on a threshold: take another seed", rec["closest"])
    assert rec["laser_margin"] >= 1.0, (tag, "a laser point's grid coordinate sits on an fp64 rounding boundary: take another seed", rec["laser_margin"])
    assert rec["ok_o"] == 1 and rec["ok_g"] == 1, (tag, "solver_ok", rec["ok_o"], rec["ok_g"])
    if rec["stage"] == "mark":
        assert rec["n_out_o"] == rec["n_out_g"], (tag, "outliers marked", rec["n_out_o"], rec["n_out_g"])
        return
    factor = CASES[name]["factor"].get(rec["stage"], FACTOR)
    assert T.within_criterion(rec["e_g"], rec["e_o"], factor, ST.floor_of(rec["n"])), (tag, "eo, eg, floor", rec["e_o"], rec["e_g"], ST.floor_of(rec["n"]), "block", rec.get("block_g"))


def log_lines(records):
    """The records of one case, one line per step (profiles/stage_forms_truth.log): the form describe() reported, lambda, then for every
    stage  name n eo eg ratio  (S: also eo / eg on sum|terms| and cond(H_ll + lambda) of the worst landmark)."""
    out = []
    for step in sorted({r["step"] for r in records}):
        recs = [r for r in records if r["step"] == step]
        i = recs[0]["info"]
        head = (f"{recs[0]['case']} step {step} lanes {i.get('lanes_per_landmark', 0)} chunks {i.get('n_schur_chunks', 0)} runs {i.get('schur_runs', 0)}x{i.get('schur_run_landmarks', 0)} "
                f"code {i.get('solver_kernel', 0)} npf {i.get('n_free_poses', 0)}")
        if recs[0]["stage"] == "mark":
            out.append(f"{head} | mark outliers o/g {recs[0]['n_out_o']}/{recs[0]['n_out_g']}")
            continue
        parts = []
        for r in recs:
            eg = r["e_g"]
            part = f"{r['stage']} {r['n']} {r['e_o']:.1e} {'-' if eg is None else format(eg, '.1e')} {'-' if eg is None else format(eg / max(r['e_o'], ST.floor_of(r['n'])), '.2f')}"
            if r["stage"] == "S":
                em = r["e_mag_g"]
                part += f" ({r['e_mag_o']:.1e} {'-' if em is None else format(em, '.1e')} cond {r['cond']:.1e})"
            parts.append(part)
        out.append(f"{head} lambda {recs[0]['lam']:.3e} | " + "; ".join(parts))
    return out
