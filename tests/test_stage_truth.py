"""The extended-precision truth of tests/stage_truth.py, checked on the CPU: its Jacobians against central differences in long double,
its Schur complement against a dense long-double A - B D^-1 B^T, the oracle against it on every window of the GPU case table
(tests/stage_forms.py), and the criterion eg <= 10 max(eo, (64 + n) u) shown to bite on nine single wrongs applied to the oracle's own
buffers.  tests/test_gpu_stage_forms.py holds every device kernel form to the same truth.

The second half does the same for the Ceres branch (Optimizer/Framework=1, tests/ceres_stage_forms.py): the factor's
Jacobians against central differences, the damped Schur truth against the dense long-double solve of (H + lambda diag m) dx = b, the
dogleg truth against the textbook construction in the scaled variables, the oracle on every window under both strategies, and nine
single wrongs of that branch refused at their own stage.  tests/test_gpu_ceres_stage_forms.py holds the device to it."""
import numpy as np
import pytest

import oracle_lib
import stage_forms as F
import stage_truth as ST
from visfs_amd import abi

LD = np.longdouble
FD_TOL = 1e-8                                    # central differences with step 1e-9 * scale: truncation ~1e-18, rounding ~1e-19 / 1e-9


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ----------------------------------------------------------------- the truth is right
@pytest.fixture(scope="module")
def c3(olib):
    """The packed C3 window of the parity tests' shape (odometry, outliers, fixed landmarks) and its truth arrays."""
    prm, wb, gb, graph, steps, lams, npf = F.oracle_steps(olib, "odo-c3")
    return gb, graph


def test_stereo_jacobians_agree_with_central_differences(c3):
    gb, g = c3
    k = np.arange(0, gb.n_obs, 97)
    tq = ST._ld(gb.pose_tq)[g["obs_pose"][k]]; pw = ST._ld(gb.point_xyz)[g["obs_point"][k]]; uvr = g["obs_uvr"][k]
    e0, _, Ji, Jj = ST.stereo_edge(tq, pw, uvr, g["intr"])
    h = LD(1e-9) * np.abs(pw).max()
    fd = np.empty_like(Ji)
    for c in range(3):
        d = np.zeros(3, dtype=LD); d[c] = h
        fd[:, :, c] = (ST.stereo_edge(tq, pw + d, uvr, g["intr"])[0] - ST.stereo_edge(tq, pw - d, uvr, g["intr"])[0]) / (2 * h)
    assert max(_rel(fd[n], Ji[n]) for n in range(len(k))) < FD_TOL
    # Jj is written for the camera-frame point moved by dt + dtheta x pc
    pc = np.einsum("nij,nj->ni", ST.quat_to_R(tq[:, 3:]), pw) + tq[:, :3]
    ident = np.tile(ST._ld([0, 0, 0, 0, 0, 0, 1]), (len(k), 1))
    h = LD(1e-9) * np.abs(pc).max()
    fd = np.empty_like(Jj)
    for c in range(6):
        d = np.zeros(6, dtype=LD); d[c] = h
        move = d[:3] + np.cross(d[3:], pc)
        fd[:, :, c] = (ST.stereo_edge(ident, pc + move, uvr, g["intr"])[0] - ST.stereo_edge(ident, pc - move, uvr, g["intr"])[0]) / (2 * h)
    assert max(_rel(fd[n], Jj[n]) for n in range(len(k))) < FD_TOL


def _left(tq, d):
    """The left update the odometry Jacobians are written for: t + dt, (dtheta / 2, 1) * q normalised."""
    return ST.pose_update(tq, d)


def test_odometry_jacobians_agree_with_central_differences_under_the_left_update(c3):
    gb, g = c3
    assert len(g["odo_from"]) == 11
    a = ST._ld(gb.pose_tq)[g["odo_from"]]; b = ST._ld(gb.pose_tq)[g["odo_to"]]; m = g["odo_tq"]
    e0, Ji, Jj = ST.odo_edge(a, b, m)
    fi = np.empty_like(Ji); fj = np.empty_like(Jj)
    for c in range(6):
        h = LD(1e-9) * (np.abs(a[:, :3]).max() if c < 3 else 1)
        d = np.zeros(6, dtype=LD); d[c] = h
        fi[:, :, c] = (ST.odo_edge(_left(a, d), b, m)[0] - ST.odo_edge(_left(a, -d), b, m)[0]) / (2 * h)
        fj[:, :, c] = (ST.odo_edge(a, _left(b, d), m)[0] - ST.odo_edge(a, _left(b, -d), m)[0]) / (2 * h)
    assert max(_rel(fi[n], Ji[n]) for n in range(len(a))) < FD_TOL
    assert max(_rel(fj[n], Jj[n]) for n in range(len(a))) < FD_TOL


def test_laser_jacobian_agrees_with_central_differences(olib):
    """The function the reference differentiates: the functor with q.w := P.x, with respect to (t, qx, qy, qz), here without the
    coordinate's rounding to a double (a step of 1e-9 cannot be seen through a spacing of 2^-23)."""
    prm, wb, gb, g, steps, lams, npf = F.oracle_steps(olib, "laser-only")
    la = g["laser"]
    tq = ST._ld(gb.pose_tq)[la["pose"]]
    P = ST._ld(la["xyz"])
    e0, J, _ = ST.laser_edge(tq, la["Tcr"], P, la, exact=True, alias_w=True)
    assert np.abs(J).max() > 0
    fd = np.empty_like(J)
    for c in range(6):
        h = LD(1e-9) * (np.abs(tq[:3]).max() if c < 3 else 1)
        d = np.zeros(7, dtype=LD); d[c] = h
        fd[:, c] = (ST.laser_edge(tq + d, la["Tcr"], P, la, exact=True, alias_w=True)[0] - ST.laser_edge(tq - d, la["Tcr"], P, la, exact=True, alias_w=True)[0]) / (2 * h)
    live = np.abs(J).max(axis=1) > 0
    # a point whose coordinate lies within the differences' reach of a knot of the piecewise cubic is no test of a derivative
    ones = np.ones(len(P), dtype=LD)
    r, c, _ = ST._laser_functor([ST._Jet(ones * tq[i]) for i in range(6)] + [ST._Jet(P[:, 0].copy())], P, la["Tcr"], la, exact=True)
    knot = np.minimum(np.abs(r.a - np.round(r.a)), np.abs(c.a - np.round(c.a))) < 1e-5
    assert (live & ~knot).sum() > 50 and knot.sum() < 5
    # (where the grid is all but flat — float 0.9 beside the border's double 0.9 — |J| is 1e-6 and the differences' own rounding,
    #  eps |e| / h, shows: it is allowed for beside the 1e-8 of the block)
    noise = 16 * float(np.finfo(LD).eps) * np.abs(e0) / (LD(1e-9) * min(float(np.abs(tq[:3]).max()), 1.0))
    for n in np.nonzero(live & ~knot)[0]:
        assert np.abs(fd[n] - J[n]).max() <= FD_TOL * np.abs(J[n]).max() + noise[n], n
    strong = live & ~knot & (np.abs(J).max(axis=1) > 1e-3)
    assert strong.sum() > 30 and max(_rel(fd[n], J[n]) for n in np.nonzero(strong)[0]) < FD_TOL
    assert np.abs(fd[~live]).max(initial=0) == 0


def test_bicubic_reproduces_the_grid_and_the_border(olib):
    prm, wb, gb, g, steps, lams, npf = F.oracle_steps(olib, "laser-only")
    la = g["laser"]
    ny, nx = la["cost"].shape
    f, _, _ = ST.bicubic(la, ST._ld([5.0, ny - 2.0, -7.0, ny + 3.0]), ST._ld([9.0, 3.0, 4.0, 2.0]))
    assert float(f[0]) == float(la["cost"][5, 9]) and float(f[1]) == float(la["cost"][ny - 2, 3])     # Catmull-Rom interpolates its knots
    assert f[2] == ST.K_MAX_COST and f[3] == ST.K_MAX_COST                                            # the maximum-cost border


def test_huber_both_branches_and_no_kernel():
    rho, rho1 = ST.huber(np.array([4.0, 64.0, 100.0]), 8.0)
    assert list(map(float, rho)) == [4.0, 64.0, 2 * 10 * 8 - 64] and list(map(float, rho1)) == [1.0, 1.0, 0.8]
    rho, rho1 = ST.huber(np.array([100.0]), 0.0)
    assert float(rho[0]) == 100.0 and float(rho1[0]) == 1.0


def test_schur_truth_equals_the_dense_long_double_complement_on_a_hand_built_system():
    rng = np.random.default_rng(3)
    npf, Nl = 3, 4
    obs = [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (1, 2), (2, 2), (0, 3)]                      # (pose, landmark), landmark-major
    obs.sort(key=lambda t: (t[1], t[0]))
    g = dict(pose_fixed=np.zeros(npf, bool), point_fixed=np.zeros(Nl, bool), obs_pose=np.array([o[0] for o in obs]), obs_point=np.array([o[1] for o in obs]))
    Hpl = rng.standard_normal((len(obs), 6, 3))
    M = rng.standard_normal((Nl, 3, 3)); Hl = M @ M.transpose(0, 2, 1) + 0.1 * np.eye(3)
    Hll = np.stack([Hl[:, 0, 0], Hl[:, 0, 1], Hl[:, 0, 2], Hl[:, 1, 1], Hl[:, 1, 2], Hl[:, 2, 2]], axis=1)
    Hpp = np.zeros((6 * npf, 6 * npf))
    for a in range(npf):
        A = rng.standard_normal((6, 6)); Hpp[6 * a:6 * a + 6, 6 * a:6 * a + 6] = A @ A.T + 6 * np.eye(6)
    X = rng.standard_normal((6, 6)); Hpp[0:6, 6:12] = X; Hpp[6:12, 0:6] = X.T                   # an odometry block
    bp = rng.standard_normal(6 * npf); bl = rng.standard_normal((Nl, 3)); lam = 0.37
    tr = ST.schur_truth(g, lam, Hpp, bp, Hpl, Hll, bl, np.ones(len(obs)))
    B = np.zeros((6 * npf, 3 * Nl), dtype=LD)
    for k, (a, l) in enumerate(obs):
        B[6 * a:6 * a + 6, 3 * l:3 * l + 3] = Hpl[k]
    Dm = np.zeros((3 * Nl, 3 * Nl), dtype=LD)
    for l in range(Nl):
        Dm[3 * l:3 * l + 3, 3 * l:3 * l + 3] = Hl[l].astype(LD) + LD(lam) * np.eye(3, dtype=LD)
    Di = np.linalg.inv(Dm.astype(np.float64)).astype(LD)
    for _ in range(3):
        Di = Di @ (2 * np.eye(3 * Nl, dtype=LD) - Dm @ Di)
    dense = Hpp.astype(LD) + LD(lam) * np.eye(6 * npf, dtype=LD) - B @ Di @ B.T
    dense_b = bp.astype(LD) - B @ Di @ bl.reshape(-1).astype(LD)
    assert {tuple(k) for k in tr["keys"]} == {(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)}
    for (i, j), blk in zip(tr["keys"], tr["S"]):
        assert np.abs(blk - dense[6 * i:6 * i + 6, 6 * j:6 * j + 6]).max() < 1e-17 * np.abs(dense).max()
    assert np.abs(tr["bs"].reshape(-1) - dense_b).max() < 1e-17 * np.abs(dense_b).max()
    assert tr["residual"] < 1e-17
    e_own, e_mag, _, _ = ST.compare_S(dense.astype(np.float64), npf, tr)
    assert e_own < 4 * ST.U
    # a pose whose H_pp diagonal is all zero is pinned; a fixed landmark and a landmark without active edge contribute nothing
    Hpp2 = Hpp.copy(); Hpp2[12:, :] = 0; Hpp2[:, 12:] = 0
    w = np.ones(len(obs)); w[[k for k, o in enumerate(obs) if o[0] == 2 or o[1] == 3]] = 0
    g2 = dict(g, point_fixed=np.array([False, True, False, False]))
    tr2 = ST.schur_truth(g2, lam, Hpp2, bp, Hpl, Hll, bl, w)
    blocks = {tuple(k): b for k, b in zip(tr2["keys"], tr2["S"])}
    assert np.array_equal(blocks[2, 2], np.eye(6)) and not tr2["used"][1] and not tr2["used"][3] and tr2["n_terms"] == 4


# ----------------------------------------------------------------- the oracle meets the truth
@pytest.mark.parametrize("name", F.CPU_CASES)
def test_oracle_meets_the_truth_on_every_window_of_the_case_table(olib, name):
    """Every stage's eo below 10 x its floor, except S, b_s and dx_point on the ill-conditioned seeds, which are held to
    64 u cond(H_ll + lambda)^2 of the worst landmark and, tighter, to the forward error of the 3x3 inverse, 10 x floor + 64 u cond.
    S is asserted on the block's own magnitude: where the terms of the worst block cancel (the hard window after its outliers left, 841
    poses) that figure is the block's error on sum|terms| times its cancellation sum|terms| / |block|, and it may exceed the bound by
    that measured factor and no more."""
    recs = F.run_oracle_case(olib, name)
    assert recs
    ill = name.startswith("ill")
    conds = {r["step"]: r["cond"] for r in recs if r["stage"] == "S"}
    print("\n".join(F.log_lines(recs)))
    for r in recs:
        tag = (name, r["step"], r["stage"])
        assert r["closest"] >= F.MIN_CLOSEST and r["laser_margin"] >= 1.0 and r["ok_o"] == 1, (tag, "take another seed", r["closest"], r["laser_margin"])
        if r["stage"] == "mark":
            continue
        bound = 10 * ST.floor_of(r["n"])
        if ill and r["stage"] in ("S", "bs", "dx_point"):
            cond = conds[r["step"]]
            assert r["e_o"] <= 64 * ST.U * cond ** 2, (tag, r["e_o"], cond)
            bound += 64 * ST.U * cond
        if r["stage"] == "S":
            print(f"{name} step {r['step']} S: eo {r['e_o']:.2e} on sum|terms| {r['e_mag_o']:.2e} cancellation {r['cancel_o']:.1f} cond {r['cond']:.2e}")
            assert r["e_mag_o"] < bound and r["e_o"] < bound * max(r["cancel_o"], 1.0), (tag, r["e_o"], r["e_mag_o"], r["cancel_o"], bound)
        else:
            assert r["e_o"] < bound, (tag, r["e_o"], bound)


def test_cpu_cases_cover_every_window_of_the_table():
    assert {F.CASES[n]["window"] for n in F.CPU_CASES} == {c["window"] for c in F.CASES.values()}
    for n in F.CPU_CASES:                                          # (the same parameters as some case of the table, so the oracle's side is shared)
        assert n in F.CASES


def test_the_windows_have_the_shapes_their_cases_claim(olib):
    for name in F.CPU_CASES:
        prm, wb, gb, g, *_ = F.oracle_steps(olib, name)
        F.check_window(name, gb, g)


def test_every_term_of_the_schur_sum_is_seen(c3, olib):
    """Leaving out any one co-observation term of the truth's sum moves its block by more than the bound the oracle is held to."""
    gb, g = c3
    o = oracle_lib.OracleSystem(olib, abi.default_params(iterations=10, solver=2), gb)
    _, md = o.linearize()
    lin = F._fetch(o, F.LIN_BUFS)
    lam = 1e-5 * md
    assert o.trial(lam)[3] == 1
    S = o.fetch(abi.BUF_S).copy()
    npf = o.npf
    o.close()
    args = (g, lam, lin["Hpp"], lin["bp"], lin["Hpl"], lin["Hll"], lin["bl"], lin["weight"])
    tr = ST.schur_truth(*args)
    bound = 10 * ST.floor_of(tr["n_S"])
    assert ST.compare_S(S, npf, tr)[0] < bound
    rel = tr["term_max"] / ST._own(tr["S"])[tr["term_block"]]
    assert tr["n_terms"] > 1000 and float(rel.min()) > 100 * bound
    for k in (int(np.argmin(rel)), 0, tr["n_terms"] // 2, tr["n_terms"] - 1):
        assert ST.compare_S(S, npf, ST.schur_truth(*args, drop_term=k))[0] > bound, k


# ----------------------------------------------------------------- the criterion bites
NAME = "odo-c3"


@pytest.fixture(scope="module")
def stepped(olib, c3):
    """The oracle on the C3 window: its first linearisation and trial, and the linearisation after mark_outliers, with every buffer."""
    gb, g = c3
    o = oracle_lib.OracleSystem(olib, abi.default_params(iterations=10, solver=2), gb)
    pose = gb.pose_tq.copy(); pt = gb.point_xyz.copy(); level = np.zeros(gb.n_obs, np.uint8)
    chi, md = o.linearize()
    lin = F._fetch(o, F.LIN_BUFS)
    lam = 1e-5 * md
    tchi, sc, _, ok = o.trial(lam)
    assert ok == 1
    tr = F._fetch(o, F.TRIAL_BUFS)
    o.commit(); o.linearize()
    assert o.mark_outliers() > 0
    level2 = np.asarray(o.download()[2]).astype(np.uint8)
    chi2, md2 = o.linearize()
    lin2 = F._fetch(o, F.LIN_BUFS)
    pose2 = tr["pose_trial"].reshape(-1, 7).copy(); pt2 = tr["point_trial"].reshape(-1, 3).copy()
    o.close()
    return dict(gb=gb, g=g, pose=pose, pt=pt, level=level, chi=chi, md=md, lin=lin, lam=lam, tchi=tchi, sc=sc, tr=tr,
                pose2=pose2, pt2=pt2, level2=level2, chi2=chi2, md2=md2, lin2=lin2)


def _failing(kind, so, sg):
    """The stages of one step at which check_record refuses the (mutated) side `sg` beside the oracle `so`, in stage order."""
    step_o = dict(step=0, kind=kind, lam=0.0, stages=so, closest=(1.0, 1.0, ST.INF), ok=1, n_out=0)
    step_g = dict(step_o, stages=sg)
    bad = []
    for rec in F.records_of(NAME, [step_o], [step_g], dict(n_free_poses=0)):
        try:
            F.check_record(rec, device=False)
        except AssertionError:
            bad.append(rec["stage"])
    return bad


def _lin(s, second=False, **mut):
    lin = dict(s["lin2"] if second else s["lin"])
    lin.update(mut)
    args = (s["pose2"], s["pt2"], s["level2"]) if second else (s["pose"], s["pt"], s["level"])
    ret = (s["chi2"], s["md2"]) if second else (s["chi"], s["md"])
    return ST.judge_linearize(s["g"], *args, lin, *ret)[0]


def _trial(s, **mut):
    side = {**s["lin"], **s["tr"]}
    side.update(mut)
    return ST.judge_trial(s["g"], s["pose"], s["pt"], s["level"], s["lam"], side, s["tchi"], s["sc"])[0]


def _edge(s, k, second=False):
    g, gb = s["g"], s["gb"]
    pose, pt = (s["pose2"], s["pt2"]) if second else (s["pose"], s["pt"])
    return ST.stereo_edge(pose[g["obs_pose"][k]], pt[g["obs_point"][k]], g["obs_uvr"][k], g["intr"])


def test_the_unmutated_oracle_passes_every_stage(stepped):
    s = stepped
    assert _failing("linearize", _lin(s), _lin(s)) == [] and _failing("trial", _trial(s), _trial(s)) == []
    assert _failing("linearize", _lin(s, True), _lin(s, True)) == []


def test_criterion_rejects_one_observation_dropped_from_the_longest_track(stepped):
    s = stepped; g = s["g"]
    active = ST.active_edges(g, s["level"]) & ~g["point_fixed"][g["obs_point"]]
    track = np.bincount(g["obs_point"][active], minlength=len(g["point_fixed"]))
    l = int(np.argmax(track))
    k = int(np.nonzero(active & (g["obs_point"] == l))[0][0])
    _, _, Ji, _ = _edge(s, k)
    wo = s["lin"]["weight"][k] * g["w_px"]
    c = (Ji[0].T @ (wo * Ji[0]))[np.triu_indices(3)].astype(np.float64)
    Hll = s["lin"]["Hll"].copy(); Hll[6 * l:6 * l + 6] -= c
    bad = _failing("linearize", _lin(s), _lin(s, Hll=Hll))
    assert track[l] >= 8 and bad[0] == "Hll", bad


def test_criterion_rejects_an_hpl_tile_transposed_in_its_last_two_columns(stepped):
    s = stepped
    Hpl = s["lin"]["Hpl"].copy().reshape(-1, 6, 3)
    k = int(np.argmin(np.where(np.abs(Hpl).max(axis=(1, 2)) > 0, np.abs(Hpl).max(axis=(1, 2)), np.inf)))     # the smallest tile that is there at all
    Hpl[k] = Hpl[k][:, [0, 2, 1]]
    assert _failing("linearize", _lin(s), _lin(s, Hpl=Hpl.reshape(-1)))[0] == "Hpl"


def test_criterion_rejects_the_huber_weight_taken_as_delta_over_chi2(stepped):
    s = stepped; g = s["g"]
    chi = s["lin"]["chi2"]
    out = chi > g["delta"] ** 2
    assert out.sum() > 0
    w = s["lin"]["weight"].copy(); w[out] = g["delta"] / chi[out]
    assert _failing("linearize", _lin(s), _lin(s, weight=w))[0] == "weight"


def test_criterion_rejects_the_bs_contribution_of_one_landmark_dropped(stepped):
    s = stepped; g = s["g"]; lin = s["lin"]
    tr = ST.schur_truth(g, s["lam"], lin["Hpp"], lin["bp"], lin["Hpl"], lin["Hll"], lin["bl"], lin["weight"])
    pidx = ST.pose_index(g)
    l = int(g["obs_point"][tr["el"][len(tr["el"]) // 2]])
    bs = s["tr"]["bs"].copy().reshape(-1, 6)
    Db = (tr["D"][l] @ ST._ld(lin["bl"]).reshape(-1, 3)[l])
    for k in tr["el"][g["obs_point"][tr["el"]] == l]:
        bs[pidx[g["obs_pose"][k]]] += (ST._ld(lin["Hpl"]).reshape(-1, 6, 3)[k] @ Db).astype(np.float64)
    assert _failing("trial", _trial(s), _trial(s, bs=bs.reshape(-1)))[0] == "bs"


def test_criterion_rejects_an_off_diagonal_block_of_s_without_its_mirror(stepped):
    s = stepped
    n6 = len(s["tr"]["bs"]); npf = n6 // 6
    S = s["tr"]["S"].copy().reshape(npf, 6, npf, 6)
    assert np.abs(S[1, :, 3, :]).max() > 0
    S[3, :, 1, :] = 0.0
    assert _failing("trial", _trial(s), _trial(s, S=S.reshape(-1)))[0] == "S"


def test_criterion_rejects_one_s_entry_moved_by_1e_11_of_its_block(stepped):
    s = stepped
    n6 = len(s["tr"]["bs"]); npf = n6 // 6
    S = s["tr"]["S"].copy().reshape(npf, 6, npf, 6)
    S[2, 4, 5, 1] += 1e-11 * np.abs(S[2, :, 5, :]).max()
    assert np.abs(s["tr"]["S"].reshape(npf, 6, npf, 6)[2, :, 5, :]).max() > 0
    assert _failing("trial", _trial(s), _trial(s, S=S.reshape(-1)))[0] == "S"


def test_criterion_rejects_a_level_1_edge_left_in_hpp(stepped):
    s = stepped; g = s["g"]
    pidx = ST.pose_index(g)
    cand = np.nonzero((s["level2"] == 1) & (pidx[g["obs_pose"]] >= 0))[0]
    k = int(cand[0]); a = int(pidx[g["obs_pose"][k]])
    _, _, _, Jj = _edge(s, k, second=True)
    n6 = len(s["lin2"]["bp"])
    Hpp = s["lin2"]["Hpp"].copy().reshape(n6, n6)
    Hpp[6 * a:6 * a + 6, 6 * a:6 * a + 6] += (Jj[0].T @ (LD(g["w_px"]) * Jj[0])).astype(np.float64)
    assert s["lin2"]["weight"][k] == 0 and not np.any(s["lin2"]["Hpl"].reshape(-1, 18)[k])           # the oracle itself left it out
    assert _failing("linearize", _lin(s, True), _lin(s, True, Hpp=Hpp.reshape(-1)))[0] == "Hpp"


def test_criterion_rejects_a_pose_update_that_normalises_before_multiplying(stepped):
    """q <- (d / 2, 1) * normalise(q), the product left as it is: off by |d|^2 / 8."""
    s = stepped; g = s["g"]
    free = ~g["pose_fixed"]
    d = s["tr"]["dx_pose"].reshape(-1, 6)
    pose = s["pose"].copy()
    dq = np.concatenate([d[:, 3:] / 2, np.ones((len(d), 1))], axis=1)
    q = ST.quat_mul(dq, ST.quat_normalize(pose[free][:, 3:])).astype(np.float64)
    pt = s["tr"]["pose_trial"].copy().reshape(-1, 7)
    pt[free, 3:] = q
    assert _failing("trial", _trial(s), _trial(s, pose_trial=pt.reshape(-1)))[0] == "pose_trial"


def test_criterion_rejects_dx_point_computed_with_hll_without_lambda(stepped):
    s = stepped; g = s["g"]; lin = s["lin"]
    Nl = len(g["point_fixed"])
    x = ST._ld(s["tr"]["dx_point"]).reshape(Nl, 3)
    used = np.abs(x).max(axis=1) > 0
    A1, _ = ST.sym3_inverse(lin["Hll"].reshape(Nl, 6)[used], s["lam"])          # (H_ll + lambda)^-1, inverted again below: c = (H_ll + lambda) x
    D0, _ = ST.sym3_inverse(lin["Hll"].reshape(Nl, 6)[used], 0.0)
    c = np.linalg.solve(A1.astype(np.float64), x[used].astype(np.float64)[:, :, None])[:, :, 0]
    xm = s["tr"]["dx_point"].copy().reshape(Nl, 3)
    xm[used] = np.einsum("lrc,lc->lr", D0.astype(np.float64), c)
    assert _failing("trial", _trial(s), _trial(s, dx_point=xm.reshape(-1)))[0] == "dx_point"


# ===================================================================== Optimizer/Framework=1: the Ceres branch (tests/ceres_stage_forms.py)
import ceres_stage_forms as CF  # noqa: E402


def _solve_ld(A, b):
    """A x = b in long double: an fp64 solve refined three times."""
    A = ST._ld(A); b = ST._ld(b)
    x = np.linalg.solve(A.astype(np.float64), b.astype(np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(A.astype(np.float64), (b - A @ x).astype(np.float64)).astype(LD)
    return x


# ----------------------------------------------------------------- (a) the truth is right
def test_ceres_stereo_jacobians_agree_with_central_differences(c3):
    """The residual info * e (StereoObservationFactor.cpp:24-25) against info * (Jj, Ji) (:43, :73), to 1e-8 of the block.  The pose
    block is the factor's own: written, as EdgeStereo's, for the camera-frame point moved by dt + dtheta x pc, and handed to
    PoseLocalParameterization's [I6; 0] as it is; the translation columns are also what Plus (t + dt) gives."""
    gb, g = c3
    k = np.arange(0, gb.n_obs, 97)
    tq = ST._ld(gb.pose_tq)[g["obs_pose"][k]]; pw = ST._ld(gb.point_xyz)[g["obs_point"][k]]; uvr = g["obs_uvr"][k]
    info = LD(g["w_px"])
    _, _, Ji, Jj = ST.stereo_edge(tq, pw, uvr, g["intr"])
    pc = np.einsum("nij,nj->ni", ST.quat_to_R(tq[:, 3:]), pw) + tq[:, :3]
    ident = np.tile(ST._ld([0, 0, 0, 0, 0, 0, 1]), (len(k), 1))
    h = LD(1e-9) * np.abs(pc).max()
    fd = np.empty_like(Jj)
    for c in range(6):
        d = np.zeros(6, dtype=LD); d[c] = h
        move = d[:3] + np.cross(d[3:], pc)
        fd[:, :, c] = info * (ST.stereo_edge(ident, pc + move, uvr, g["intr"])[0] - ST.stereo_edge(ident, pc - move, uvr, g["intr"])[0]) / (2 * h)
    assert max(_rel(fd[n], info * Jj[n]) for n in range(len(k))) < FD_TOL
    for c in range(3):
        d = np.zeros(6, dtype=LD); d[c] = h
        plus = info * (ST.stereo_edge(ST.pose_update(tq, d), pw, uvr, g["intr"])[0] - ST.stereo_edge(ST.pose_update(tq, -d), pw, uvr, g["intr"])[0]) / (2 * h)
        assert max(_rel(plus[n], info * Jj[n, :, c]) for n in range(len(k))) < FD_TOL
    fl = np.empty_like(Ji)
    h = LD(1e-9) * np.abs(pw).max()
    for c in range(3):
        d = np.zeros(3, dtype=LD); d[c] = h
        fl[:, :, c] = info * (ST.stereo_edge(tq, pw + d, uvr, g["intr"])[0] - ST.stereo_edge(tq, pw - d, uvr, g["intr"])[0]) / (2 * h)
    assert max(_rel(fl[n], info * Ji[n]) for n in range(len(k))) < FD_TOL


def test_ceres_laser_jacobian_is_taken_over_the_raw_parameters_at_the_poses_own_w(olib):
    """OccupiedSpace2dFactor differentiates over the seven raw parameters and the local parameterisation drops q.w: central differences
    in (t, qx, qy, qz) with q.w held — not the g2o edge's aliased function, which differs from it."""
    prm, wb, gb, g, steps, lams, npf = F.oracle_steps(olib, "laser-only")
    la = g["laser"]
    tq = ST._ld(gb.pose_tq)[la["pose"]]; P = ST._ld(la["xyz"])
    e0, J, _ = ST.laser_edge(tq, la["Tcr"], P, la, exact=True, own_w=True)
    Jg2o = ST.laser_edge(tq, la["Tcr"], P, la, exact=True)[1]
    fd = np.empty_like(J)
    for c in range(6):
        h = LD(1e-9) * (np.abs(tq[:3]).max() if c < 3 else 1)
        d = np.zeros(7, dtype=LD); d[c] = h
        fd[:, c] = (ST.laser_edge(tq + d, la["Tcr"], P, la, exact=True)[0] - ST.laser_edge(tq - d, la["Tcr"], P, la, exact=True)[0]) / (2 * h)
    ones = np.ones(len(P), dtype=LD)
    r, c_, _ = ST._laser_functor([ST._Jet(ones * tq[i]) for i in range(7)], P, la["Tcr"], la, exact=True)
    knot = np.minimum(np.abs(r.a - np.round(r.a)), np.abs(c_.a - np.round(c_.a))) < 1e-5
    strong = ~knot & (np.abs(J).max(axis=1) > 1e-3)
    assert strong.sum() > 30 and max(_rel(fd[n], J[n]) for n in np.nonzero(strong)[0]) < FD_TOL
    assert max(_rel(Jg2o[n], J[n]) for n in np.nonzero(strong)[0]) > 1e-3


def _hand_system(rng):
    """3 free poses, 4 landmarks, 8 observations: H = J^T J of a random Jacobian (so every Schur term and ||J v||^2 exist), gradient, and
    Ceres' scaling and multipliers of it."""
    npf, Nl = 3, 4
    obs = sorted([(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (1, 2), (2, 2), (0, 3)], key=lambda t: (t[1], t[0]))
    n = 6 * npf + 3 * Nl
    J = np.zeros((3 * len(obs), n))
    for k, (a, l) in enumerate(obs):
        J[3 * k:3 * k + 3, 6 * a:6 * a + 6] = rng.standard_normal((3, 6))
        J[3 * k:3 * k + 3, 6 * npf + 3 * l:6 * npf + 3 * l + 3] = rng.standard_normal((3, 3)) * (1e-4 if l == 3 else 1.0)   # (landmark 3: on the lower clamp)
    f = rng.standard_normal(3 * len(obs))
    H = ST._ld(J).T @ ST._ld(J); b = -(ST._ld(J).T @ ST._ld(f))
    s2 = ST.jacobi_scale2(np.diag(H))
    m, margin, n_low = ST.multipliers(np.diag(H), s2)
    assert n_low == 3 and margin > 1e-3
    return npf, Nl, obs, J, H, b, m


def test_damped_schur_truth_equals_the_dense_long_double_solve(olib):
    npf, Nl, obs, J, H, b, m = _hand_system(np.random.default_rng(5))
    n6 = 6 * npf
    lam = 0.37
    g = dict(pose_fixed=np.zeros(npf, bool), point_fixed=np.zeros(Nl, bool), obs_pose=np.array([o[0] for o in obs]), obs_point=np.array([o[1] for o in obs]))
    Hf = H.astype(np.float64)
    Hpl = np.stack([Hf[6 * a:6 * a + 6, n6 + 3 * l:n6 + 3 * l + 3] for a, l in obs])
    Hll = np.stack([Hf[n6 + 3 * l:n6 + 3 * l + 3, n6 + 3 * l:n6 + 3 * l + 3][np.triu_indices(3)] for l in range(Nl)])
    Hpp = np.zeros((n6, n6))
    for a in range(npf):
        Hpp[6 * a:6 * a + 6, 6 * a:6 * a + 6] = Hf[6 * a:6 * a + 6, 6 * a:6 * a + 6]
    bf = b.astype(np.float64)
    # (the multipliers are taken from the fp64 copies the truth is given)
    s2 = ST.jacobi_scale2(np.diag(Hf)); mm, _, _ = ST.multipliers(np.diag(Hf), s2)
    mp, ml = mm[:n6].reshape(npf, 6), mm[n6:].reshape(Nl, 3)
    tr = ST.schur_truth(g, lam, Hpp, bf[:n6], Hpl, Hll, bf[n6:].reshape(Nl, 3), np.ones(len(obs)), mp=mp, ml=ml)
    A = ST._ld(Hf) + LD(lam) * np.diag(mm)
    dx = _solve_ld(A, bf)
    S = np.zeros((n6, n6), dtype=LD)
    for (i, j), blk in zip(tr["keys"], tr["S"]):
        S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk; S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blk.T
    xp = _solve_ld(S, tr["bs"].reshape(-1))
    assert np.abs(xp - dx[:n6]).max() < 1e-15 * np.abs(dx).max()
    Bm = ST._ld(Hf)[:n6, n6:]
    xl = np.einsum("lrc,lc->lr", tr["D"], ST._ld(bf[n6:]).reshape(Nl, 3) - (Bm.T @ xp).reshape(Nl, 3))
    assert np.abs(xl.reshape(-1) - dx[n6:]).max() < 1e-15 * np.abs(dx).max()
    # with the plain lambda in place of lambda m the solve is another one
    tr0 = ST.schur_truth(g, lam, Hpp, bf[:n6], Hpl, Hll, bf[n6:].reshape(Nl, 3), np.ones(len(obs)))
    assert np.abs(tr0["bs"] - tr["bs"]).max() > 1e-3 * np.abs(tr["bs"]).max()


def test_dogleg_truth_equals_the_textbook_construction_in_the_scaled_variables():
    npf, Nl, obs, J, H, b, m = _hand_system(np.random.default_rng(6))
    g = -b
    mu = LD(1e-3)
    D = np.sqrt(m)
    Hs = H / np.outer(D, D); gs = g / D
    gn_s = _solve_ld(Hs + mu * np.eye(len(D), dtype=LD), -gs)                      # the regularised Gauss-Newton step, scaled
    alpha = (gs @ gs) / (gs @ Hs @ gs)
    cauchy = -alpha * gs
    dn = gn_s / D; v = g / m
    Jv = ST._ld(J) @ v
    s1, s2, s3, jv2 = gs @ gs, gn_s @ gn_s, gs @ gn_s, Jv @ Jv
    gn_norm, c_norm = float(np.sqrt(s2)), float(np.sqrt(cauchy @ cauchy))
    assert c_norm < gn_norm
    seen = set()
    for radius in (2 * gn_norm, 0.5 * c_norm, 0.5 * (c_norm + gn_norm)):
        r = LD(radius)
        if gn_norm <= radius:
            step_s = gn_s
        elif c_norm >= radius:
            step_s = -(r / np.sqrt(gs @ gs)) * gs
        else:                                                                        # |cauchy + t (gn - cauchy)| = radius, t in (0, 1): bisection
            lo, hi = LD(0), LD(1)
            for _ in range(200):
                t = (lo + hi) / 2
                p = cauchy + t * (gn_s - cauchy)
                lo, hi = (t, hi) if p @ p < r * r else (lo, t)
            step_s = cauchy + lo * (gn_s - cauchy)
        T_ = ST.dogleg_truth(s1, s2, s3, jv2, radius, mu)
        seen.add(T_["case"])
        assert T_["margin"] > 0.01
        got_s = T_["A"] * gs + T_["B"] * gn_s
        assert np.abs(got_s - step_s).max() < 1e-15 * np.abs(step_s).max()
        assert abs(T_["norm"] - np.sqrt(step_s @ step_s)) < 1e-15 * np.sqrt(step_s @ step_s)
        step = T_["A"] * v + T_["B"] * dn                                            # the same step in the unscaled variables
        assert np.abs(step - step_s / D).max() < 1e-15 * np.abs(step).max()
        mcc = -(g @ step + (step @ H @ step) / 2)
        assert abs(T_["mcc"] - mcc) < 1e-14 * T_["mcc_mag"]
        # without mu in s^T H s the model cost change is another one (H dn = -g - mu M dn)
        shs0 = T_["A"] ** 2 * jv2 + 2 * T_["A"] * T_["B"] * (-s1) + T_["B"] ** 2 * (-s3)
        if T_["B"] != 0:
            assert abs(-(T_["A"] * s1 + T_["B"] * s3 + shs0 / 2) - mcc) > 1e-9 * T_["mcc_mag"]
    assert seen == {1, 2, 3}


# ----------------------------------------------------------------- (c) the oracle meets the truth
@pytest.mark.parametrize("name", CF.CPU_CASES)
def test_oracle_meets_the_ceres_truth_on_every_window_of_the_case_table(olib, name):
    """Every stage's eo below 10 x its floor; S as in the g2o test above: on sum|terms| below the bound, on the block's own magnitude
    within the block's measured cancellation.  No window needs a conditioning term, the clamp window's far landmarks (cond 2e6 at the
    dogleg's mu = 1e-8) included."""
    recs = CF.run_oracle_case(olib, name)
    assert recs
    print("\n".join(CF.log_lines(recs)))
    CF.check_sequence(name, recs)
    for r in recs:
        tag = (name, r["step"], r["stage"])
        CF.check_record(dict(r, e_g=r["e_o"]), device=False)                          # the conditions on the input; the criterion is trivially met
        if r["stage"] == "mark":
            continue
        bound = 10 * ST.floor_of(r["n"])
        if r["stage"] == "S":
            assert r["e_mag_o"] < bound and r["e_o"] < bound * max(r["cancel_o"], 1.0), (tag, r["e_o"], r["e_mag_o"], r["cancel_o"], r["cond"], bound)
        else:
            assert r["e_o"] < bound, (tag, r["e_o"], bound)


def test_ceres_cpu_cases_cover_every_window_of_the_table():
    assert {(CF.CASES[n]["window"], CF.CASES[n]["strategy"]) for n in CF.CPU_CASES} == {(c["window"], c["strategy"]) for c in CF.CASES.values()}


def test_the_clamp_window_has_variables_on_the_lower_clamp(olib):
    for name in ("lm-clamp", "dl-clamp"):
        recs = CF.run_oracle_case(olib, name)
        low = [r["n_low"] for r in recs if r["kind"] == "linearize" and r["stage"] == "s2l"]
        assert low and all(v == [3 * CF.CLAMP_FAR] for v in low), low
        assert min(r["closest"] for r in recs) >= CF.MIN_CLOSEST


# ----------------------------------------------------------------- (b) the criterion bites on the Ceres stages
def _ceres_stepped(olib, window, strategy, trial, prm_kw=None):
    """The oracle on `window` under `strategy`: its iteration-zero linearisation and one trial (("trial", lambda) or ("dogleg", mu, which)),
    with every buffer and what the calls returned."""
    w, kw = CF.stage_window(window)
    prm = CF.params_of(strategy, {**kw, **(prm_kw or {})})
    wb, gb, *_ = F.graph_of(olib.oracle_pack_window, prm, w)
    g = CF.graph_arrays(gb, prm)
    o = oracle_lib.OracleSystem(olib, prm, gb)
    try:
        chi, gmax, xn = o.ceres_linearize()
        lin = CF._fetch(o, CF.LIN_BUFS)
        s = dict(g=g, gb=gb, pose=gb.pose_tq.copy(), pt=gb.point_xyz.copy(), lin=lin, chi=chi, gmax=gmax, xn=xn)
        if trial[0] == "trial":
            tchi, sc, sn, ok = o.ceres_trial(trial[1])
            s.update(lam=trial[1], tchi=tchi, sc=sc, sn=sn)
        else:
            assert o.dogleg_stage(1e300, trial[1])["ok"] == 1                        # (leaves dn in the DX buffers: the truth's norms of it)
            gn, cauchy = ST.dogleg_norms(g, s["pose"], s["pt"], {**lin, **CF._fetch(o, F.TRIAL_BUFS)})
            radius = float((2 * gn, cauchy / 2, (cauchy + gn) / 2)[trial[2]])
            res = o.dogleg_stage(radius, trial[1])
            ok = res["ok"]
            s.update(mu=trial[1], radius=radius, res=res)
        assert ok == 1
        s["tr"] = CF._fetch(o, F.TRIAL_BUFS)
    finally:
        o.close()
    return s


@pytest.fixture(scope="module")
def lv_lm(olib):
    return _ceres_stepped(olib, ("laser", True, F.LASER_SEED), "lm", ("trial", 1e-4), dict(pixel_variance=2.0))


@pytest.fixture(scope="module")
def lv_dl(olib):
    return _ceres_stepped(olib, ("laser", True, F.LASER_SEED), "dl", ("dogleg", 1e-3, 2), dict(pixel_variance=2.0))


@pytest.fixture(scope="module")
def clamp_lm(olib):
    return _ceres_stepped(olib, ("clamp",), "lm", ("trial", 1e-4))


def _clin(s, **mut):
    return ST.judge_ceres_linearize(s["g"], s["pose"], s["pt"], {**s["lin"], **mut}, s["chi"], s["gmax"], s["xn"])[0]


def _ctrial(s, **mut):
    return ST.judge_ceres_trial(s["g"], s["pose"], s["pt"], s["lam"], {**s["lin"], **s["tr"], **mut}, s["tchi"], s["sc"], s["sn"])[0]


def _cdog(s, res=None, **mut):
    return ST.judge_dogleg(s["g"], s["pose"], s["pt"], s["radius"], s["mu"], {**s["lin"], **s["tr"], **mut}, {**s["res"], **(res or {})})[0]


def _refused(kind, so, sg):
    """The stages of one step at which CF.check_record refuses the (mutated) side `sg` beside the oracle `so`, in stage order."""
    base = dict(step=0, kind=kind, lam=0.0, radius=0.0, closest=(1.0, 1.0, ST.INF), ok=1, n_out=0, flags_ok=1, case=0, dl_margin=ST.INF, n_low=0,
                s2_vs_prev=-1, s2_vs_first=-1)
    bad = []
    for rec in CF.records_of("lm-laser-visual", [dict(base, stages=so)], [dict(base, stages=sg)], dict(n_free_poses=0)):
        try:
            CF.check_record(rec, device=False)
        except AssertionError:
            bad.append(rec["stage"])
    return bad


def _dense_S(tr, npf):
    S = np.zeros((npf, 6, npf, 6))
    for (i, j), blk in zip(tr["keys"], tr["S"]):
        S[i, :, j, :] = blk.astype(np.float64); S[j, :, i, :] = blk.T.astype(np.float64)
    return S.reshape(-1)


def test_the_unmutated_oracle_passes_every_ceres_stage(lv_lm, lv_dl, clamp_lm):
    assert _refused("linearize", _clin(lv_lm), _clin(lv_lm)) == [] and _refused("trial", _ctrial(lv_lm), _ctrial(lv_lm)) == []
    assert _refused("dogleg", _cdog(lv_dl), _cdog(lv_dl)) == [] and _refused("trial", _ctrial(clamp_lm), _ctrial(clamp_lm)) == []
    assert lv_dl["res"]["A"] != 0 and lv_dl["res"]["B"] not in (0.0, 1.0)              # the dogleg trial is on the segment (case 3)


def test_criterion_rejects_the_jacobi_scale_without_the_square_root(lv_lm):
    s = lv_lm; lin = s["lin"]
    n6 = len(lin["bp"])
    q = 1.0 / (1.0 + lin["Hpp"].reshape(n6, n6).diagonal())
    assert _refused("linearize", _clin(s), _clin(s, s2p=q * q))[0] == "s2p"
    ql = 1.0 / (1.0 + lin["Hll"].reshape(-1, 6)[:, [0, 3, 5]])
    assert _refused("linearize", _clin(s), _clin(s, s2l=(ql * ql).reshape(-1)))[0] == "s2l"


def test_criterion_rejects_the_information_value_not_squared(lv_lm):
    s = lv_lm
    assert s["g"]["w_px"] == 0.5
    assert _refused("linearize", _clin(s), _clin(s, chi2=s["lin"]["chi2"] / s["g"]["w_px"]))[0] == "chi2"
    # one pass that squares it once too few: H_ll with rho' info in place of rho' info^2
    assert _refused("linearize", _clin(s), _clin(s, Hll=s["lin"]["Hll"] / s["g"]["w_px"]))[0] == "Hll"


def test_criterion_rejects_g2os_kernel_weight_in_place_of_huber_loss(lv_lm):
    """g2o's rho' is a function of ITS chi2 = e^T Omega e; HuberLoss's of ||info e||^2."""
    s = lv_lm; g = s["g"]
    w = np.asarray(ST.huber(s["lin"]["chi2"] / g["w_px"], g["delta"])[1], dtype=np.float64) * (s["lin"]["weight"] != 0)
    assert (w != s["lin"]["weight"]).sum() > 0
    assert _refused("linearize", _clin(s), _clin(s, weight=w))[0] == "weight"


def _wrong_multiplier_trial(s, mp, ml):
    lin = s["lin"]
    npf = len(lin["bp"]) // 6
    tr = ST.schur_truth(s["g"], s["lam"], lin["Hpp"], lin["bp"], lin["Hpl"], lin["Hll"], lin["bl"], lin["weight"], mp=mp, ml=ml)
    return dict(S=_dense_S(tr, npf), bs=tr["bs"].astype(np.float64).reshape(-1))


def test_criterion_rejects_the_lower_clamp_missing(clamp_lm):
    s = clamp_lm
    mp, ml, margin, n_low = ST.own_multipliers(s["g"], s["lin"])
    assert n_low == 3 * CF.CLAMP_FAR and margin > CF.MIN_CLOSEST
    npf = len(s["lin"]["bp"]) // 6
    dp, dl = ST._diagonals(s["lin"], npf, len(s["g"]["point_fixed"]))
    ml_wrong = np.where(dl > 0, dl, ml)                                                # m = H_ii s^2 / s^2, no clamp
    assert (ml_wrong != ml).sum() == n_low
    bad = _refused("trial", _ctrial(s), _ctrial(s, **_wrong_multiplier_trial(s, mp, ml_wrong)))
    assert bad[0] == "S", bad


def test_criterion_rejects_one_damping_term_taken_with_the_plain_lambda(lv_lm):
    s = lv_lm
    mp, ml, _, _ = ST.own_multipliers(s["g"], s["lin"])
    n6 = len(s["lin"]["bp"])
    i = n6 - 2
    S = s["tr"]["S"].copy().reshape(n6, n6)
    S[i, i] += s["lam"] * (1.0 - float(mp.reshape(-1)[i]))
    assert abs(float(mp.reshape(-1)[i]) - 1.0) > 1e-3
    assert _refused("trial", _ctrial(s), _ctrial(s, S=S.reshape(-1)))[0] == "S"


def test_criterion_rejects_one_partial_missing_from_s1(lv_dl):
    s = lv_dl; lin = s["lin"]
    mp, ml, _, _ = ST.own_multipliers(s["g"], lin)
    Nl = len(s["g"]["point_fixed"])
    used = np.nonzero(np.abs(s["tr"]["dx_point"].reshape(Nl, 3)).max(axis=1) > 0)[0]
    l = int(used[-1])                                                                   # the last landmark's share
    part = float((ST._ld(lin["bl"]).reshape(Nl, 3)[l] ** 2 / ml[l]).sum())
    assert part > 0
    assert _refused("dogleg", _cdog(s), _cdog(s, res=dict(s1=s["res"]["s1"] - part)))[0] == "s1"


def test_criterion_rejects_the_laser_blocks_missing_from_jv2(lv_dl):
    s = lv_dl; lin = s["lin"]
    mp, ml, _, _ = ST.own_multipliers(s["g"], lin)
    Nl = len(s["g"]["point_fixed"])
    used = np.abs(s["tr"]["dx_point"].reshape(Nl, 3)).max(axis=1) > 0
    P = ST.dogleg_products(s["g"], s["pose"], s["pt"], {**lin, **s["tr"]}, mp, ml, used, drop_laser=True)
    assert float(P["jv2"]) < s["res"]["jv2"]
    assert _refused("dogleg", _cdog(s), _cdog(s, res=dict(jv2=float(P["jv2"]))))[0] == "jv2"


def test_criterion_rejects_mu_missing_from_the_model_cost_change(lv_dl):
    s = lv_dl; r = s["res"]
    shs = r["A"] ** 2 * r["jv2"] + 2 * r["A"] * r["B"] * (-r["s1"]) + r["B"] ** 2 * (-r["s3"])
    mcc = -(r["A"] * r["s1"] + r["B"] * r["s3"] + 0.5 * shs)
    assert _refused("dogleg", _cdog(s), _cdog(s, res=dict(mcc=mcc)))[0] == "mcc"


def test_criterion_rejects_the_gradient_part_missing_from_the_landmark_step(lv_dl):
    s = lv_dl
    Nl = len(s["g"]["point_fixed"])
    pt = s["pt"].reshape(Nl, 3) + s["res"]["B"] * s["tr"]["dx_point"].reshape(Nl, 3)   # B dn alone, A v left out
    assert _refused("dogleg", _cdog(s), _cdog(s, point_trial=pt.reshape(-1)))[0] == "point_trial"
