"""Marginal covariances on the GPU (visfs_ba_graph_covariance / visfs_ba_window_covariance, ABI 9) against independent checks:

* small windows: the blocks of inv(H) of the test-side dense assembly (test_oracle_algebra.Dense, no Schur complement) at the GPU's
  final estimate with the GPU's outlier flags as edge levels;
* BASELINE sizes: the checker's Schur complement S, H_ll and H_pl at the same state (outlier edges left out), inverted in NumPy;
* the window layer against the graph layer mapped through visfs_ba_pose_cov_to_world; the call leaves every later result unchanged;
* the documented refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib
from helpers import graph_of, hard_window, ragged_window
from test_oracle_algebra import Dense
from visfs_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

_pd = C.POINTER(C.c_double)


def P(a):
    return a.ctypes.data_as(_pd)


def _solve_graph(olib, w, **kw):
    prm = abi.default_params(**kw)
    wb, gb, used, oref, mono = graph_of(olib.oracle_pack_window, prm, w)
    s = backend.Solver(prm)
    s.upload(gb)
    rc, _ = s.optimize()
    assert rc == abi.OK
    pose, pt, outl, _ = s.download()
    return prm, gb, s, pose, pt, outl


def _blk_err(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _check_special(gb, pose_cov, cross, pt_cov, pose_active, pt_active):
    """Zeros for fixed variables, NaN for free ones outside the active set, finite values elsewhere."""
    for i in range(gb.n_poses):
        if gb.pose_fixed[i]:
            assert not pose_cov[i].any()
        elif not pose_active[i]:
            assert np.isnan(pose_cov[i]).all()
        else:
            assert np.isfinite(pose_cov[i]).all()
    for i in range(gb.n_poses - 1):
        if gb.pose_fixed[i] or gb.pose_fixed[i + 1]:
            assert not cross[i].any()
        elif not (pose_active[i] and pose_active[i + 1]):
            assert np.isnan(cross[i]).all()
    for l in range(gb.n_points):
        if gb.point_fixed[l]:
            assert not pt_cov[l].any()
        elif not pt_active[l]:
            assert np.isnan(pt_cov[l]).all()
        else:
            assert np.isfinite(pt_cov[l]).all()


SMALL = {
    "C1": lambda: synth.make_window("C1"),
    "PROD": lambda: synth.make_window("PROD"),
    "RAGGED": lambda: ragged_window(),
    "HARD": lambda: hard_window(),
    "LASER": lambda: synth.make_laser_window(with_visual=True, n_points=400, seed=2),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_graph_covariance_matches_the_dense_inverse(olib, name):
    prm, gb, s, pose, pt, outl = _solve_graph(olib, SMALL[name](), iterations=10, solver=0)
    pose_cov, cross, pt_cov = s.covariance(points=True, cross=True)
    d = Dense(olib, prm, gb, level=outl.astype(np.uint8))
    H, _, _ = d.assemble(pose, pt)
    act = np.diag(H) != 0.0
    Ha = H[np.ix_(act, act)]
    Sig = np.full(H.shape, np.nan)
    Sig[np.ix_(act, act)] = np.linalg.inv(Ha)
    pose_active = np.array([d.col_pose(i) is not None and act[d.col_pose(i)].all() for i in range(d.Np)])
    pt_active = np.array([d.col_pt(l) is not None and act[d.col_pt(l)].all() for l in range(d.Nl)])
    _check_special(gb, pose_cov, cross, pt_cov, pose_active, pt_active)
    for i in range(d.Np):
        if pose_active[i]:
            c = d.col_pose(i)
            assert _blk_err(pose_cov[i], Sig[c, c]) <= 1e-8, (name, i)
    for i in range(d.Np - 1):
        if pose_active[i] and pose_active[i + 1]:
            a, b = d.col_pose(i), d.col_pose(i + 1)
            assert _blk_err(cross[i], Sig[a, b]) <= 1e-8, (name, i)
    for l in range(d.Nl):
        if pt_active[l]:
            c = d.col_pt(l)
            assert _blk_err(pt_cov[l], Sig[c, c]) <= 1e-8, (name, l)
    # a second call returns the same bytes
    again = s.covariance(points=True, cross=True)
    for x, y in zip((pose_cov, cross, pt_cov), again):
        assert np.array_equal(x, y, equal_nan=True)
    s.close()


def _schur_oracle(olib, prm, gb, pose, pt, outl):
    """The checker's S, H_ll and H_pl at the GPU's final state with the outlier edges left out (the same H)."""
    keep = outl == 0
    g2 = abi.GraphBuffers(pose, gb.pose_fixed, pt, gb.point_fixed, gb.obs_point[keep], gb.obs_pose[keep], gb.obs_uvr[keep],
                          gb.odo_from, gb.odo_to, gb.odo_tq, gb.struct.fx, gb.struct.fy, gb.struct.cx, gb.struct.cy, gb.struct.bf)
    o = oracle_lib.OracleSystem(olib, prm, g2)
    o.linearize()
    o.trial(0.0)
    n6 = 6 * o.npf
    S = o.fetch(abi.BUF_S).reshape(n6, n6)
    Hll = o.fetch(abi.BUF_HLL).reshape(-1, 6)
    Hpl = o.fetch(abi.BUF_HPL).reshape(-1, 6, 3)
    o.close()
    return g2, S, Hll, Hpl


def _check_schur_side(olib, w, prm, gb, pose, pt, outl, pose_cov, cross, pt_cov, n_points=300):
    g2, S, Hll, Hpl = _schur_oracle(olib, prm, gb, pose, pt, outl)
    Sig = np.linalg.inv(S)
    free = [i for i in range(gb.n_poses) if not gb.pose_fixed[i]]
    pf = {p: a for a, p in enumerate(free)}
    for a, i in enumerate(free):
        if np.isnan(pose_cov[i]).any():
            # outside the active set (every edge of the pose an outlier): the checker pins its block of S to I, uncoupled
            assert np.isnan(pose_cov[i]).all()
            row = S[6 * a:6 * a + 6].copy()
            row[:, 6 * a:6 * a + 6] -= np.eye(6)
            assert not row.any(), i
            continue
        assert _blk_err(pose_cov[i], Sig[6 * a:6 * a + 6, 6 * a:6 * a + 6]) <= 1e-8, i
    # the consecutive-pose cross blocks Sigma_{i,i+1}
    n_cross = 0
    for i in range(gb.n_poses - 1):
        if gb.pose_fixed[i] or gb.pose_fixed[i + 1]:
            assert not cross[i].any()
        elif np.isnan(pose_cov[i]).any() or np.isnan(pose_cov[i + 1]).any():
            assert np.isnan(cross[i]).all()
        else:
            a, b = pf[i], pf[i + 1]
            assert _blk_err(cross[i], Sig[6 * a:6 * a + 6, 6 * b:6 * b + 6]) <= 1e-8, i
            n_cross += 1
    assert n_cross > 0
    rng = np.random.default_rng(0)
    obs_pt = np.asarray(g2.obs_point); obs_pose = np.asarray(g2.obs_pose)
    cand = [l for l in range(gb.n_points) if not gb.point_fixed[l] and (obs_pt == l).any()]
    for l in rng.choice(cand, size=min(n_points, len(cand)), replace=False):
        h = Hll[l]
        D = np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])
        Di = np.linalg.inv(D)
        ks = [k for k in np.nonzero(obs_pt == l)[0] if obs_pose[k] in pf]
        E = {k: Hpl[k] @ Di for k in ks}
        ref = Di.copy()
        for ka in ks:
            for kb in ks:
                a, b = pf[obs_pose[ka]], pf[obs_pose[kb]]
                ref += E[ka].T @ Sig[6 * a:6 * a + 6, 6 * b:6 * b + 6] @ E[kb]
        assert _blk_err(pt_cov[l], ref) <= 1e-8, l


@pytest.mark.parametrize("cfg,solver", [("C2", 0), ("C2", 2), ("C3", 0), ("C4", 0)])
def test_graph_covariance_matches_the_schur_oracle_at_baseline_sizes(olib, cfg, solver):
    w = synth.make_window(cfg)
    prm, gb, s, pose, pt, outl = _solve_graph(olib, w, iterations=10, solver=solver)
    assert s.describe()["band_blocks" if solver == 0 else "n_free_poses"] >= 0
    pose_cov, cross, pt_cov = s.covariance(points=True, cross=True)
    _check_schur_side(olib, w, prm, gb, pose, pt, outl, pose_cov, cross, pt_cov)
    s.close()
    if cfg == "C2" and solver == 0:
        # the streaming form of the banded solver (VISFS_BA_BAND_ROWS=12) solves the same window bit for bit; the covariance kernels do
        # not read band_rows, so this leg checks that a second handle on that path returns the same covariance bytes end to end
        os.environ["VISFS_BA_BAND_ROWS"] = "12"
        try:
            _, _, s2, pose2, pt2, _ = _solve_graph(olib, w, iterations=10, solver=0)
        finally:
            del os.environ["VISFS_BA_BAND_ROWS"]
        assert np.array_equal(pose2, pose) and np.array_equal(pt2, pt)
        again = s2.covariance(points=True, cross=True)
        for x, y in zip((pose_cov, cross, pt_cov), again):
            assert np.array_equal(x, y, equal_nan=True)
        s2.close()


def _window_cov(s, n_poses, n_points):
    pose = np.zeros((n_poses, 6, 6)); pt = np.zeros((max(n_points, 1), 3, 3))
    rc = s.lib.visfs_ba_window_covariance(s.h, P(pose), P(pt))
    return rc, pose, pt[:n_points]


def test_window_covariance_is_the_graph_layer_result_in_world_form(olib, hiplib):
    w = ragged_window(seed=11)
    prm = abi.default_params(iterations=10, solver=0)
    s = backend.Solver(prm)
    wb = abi.WindowBuffers(w)
    rc, rb = s.solve_window(wb)
    assert rc == abi.OK
    n, m = wb.struct.n_poses, wb.struct.n_points
    rc, pose_wr, pt_cov = _window_cov(s, n, m)
    assert rc == abi.OK
    # the same handle's resident graph IS the window's: its graph-layer covariance, mapped
    pose_g = np.zeros((n, 6, 6)); pt_g = np.zeros((max(m, 1), 3, 3))
    assert s.lib.visfs_ba_graph_covariance(s.h, P(pose_g), None, P(pt_g)) == abi.OK
    tq = np.zeros((n, 7))
    assert s.lib.visfs_ba_graph_download(s.h, P(tq), None, None, None) == abi.OK
    Trc = np.array(list(wb.struct.Trc))
    for i in range(n):
        ref = np.zeros(36)
        hiplib.visfs_ba_pose_cov_to_world(P(np.ascontiguousarray(tq[i])), P(Trc), P(np.ascontiguousarray(pose_g[i])), P(ref))
        assert np.array_equal(pose_wr[i].reshape(36), ref, equal_nan=True)
    root = list(w["pose_ids"]).index(w["root_id"])
    assert not pose_wr[root].any()
    _, _, gb_used, _, _ = graph_of(olib.oracle_pack_window, prm, w)
    used = np.asarray(gb_used)[:m]
    assert (used == 0).any()
    for l in range(m):
        if not used[l]:
            assert np.isnan(pt_cov[l]).all()
        else:
            assert np.array_equal(pt_cov[l], pt_g[l], equal_nan=True)
    s.close()


def _soak_frames(n=5):
    rng = np.random.default_rng(2026)
    out = []
    for f in range(n):
        if f % 7 == 3:
            out.append(synth.make_window("PROD", window_index=f))
        else:
            n_kf = int(rng.integers(20, 61)); n_lm = int(rng.integers(2000, 6001))
            track = int(rng.integers(6, min(n_kf, 12) + 1))
            out.append(synth.make_window("custom", n_kf=n_kf, n_lm=n_lm, n_obs=n_lm * track, seed=1000 + f))
    return out


def test_covariance_calls_leave_the_next_solves_unchanged():
    frames = _soak_frames(5)
    prm = abi.default_params(iterations=10, solver=2)
    results = []
    for with_cov in (False, True):
        s = backend.Solver(prm)
        seq = []
        for w in frames:
            wb = abi.WindowBuffers(w)
            rc, rb = s.solve_window(wb)
            n = rb.struct.n_poses_out
            seq.append((rc, rb.pose_Twr_out[:n].copy(), rb.outliers(), wb.point_xyz.copy()))
            if with_cov:
                a = _window_cov(s, wb.struct.n_poses, wb.struct.n_points)
                b = _window_cov(s, wb.struct.n_poses, wb.struct.n_points)
                assert a[0] == b[0] == abi.OK
                assert np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)
        s.close()
        results.append(seq)
    for x, y in zip(*results):
        assert x[0] == y[0] and x[2] == y[2]
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[3], y[3], equal_nan=True)


def test_graph_covariance_leaves_the_estimate_and_levels_unchanged(olib):
    prm, gb, s, pose, pt, outl = _solve_graph(olib, synth.make_window("C1"), iterations=10, solver=0)
    s.covariance(points=True, cross=True)
    pose2, pt2, outl2, _ = s.download()
    assert np.array_equal(pose, pose2) and np.array_equal(pt, pt2) and np.array_equal(outl, outl2)
    s.reset(); s.optimize()
    pose3, pt3, outl3, _ = s.download()
    assert np.array_equal(pose, pose3) and np.array_equal(pt, pt3) and np.array_equal(outl, outl3)
    s.close()


def test_covariance_refusals():
    z = np.zeros(36 * 64)
    # before any solve
    s = backend.Solver(abi.default_params(iterations=10, solver=0))
    assert s.lib.visfs_ba_graph_covariance(s.h, P(z), None, None) == abi.ERR_NOT_LOADED
    assert s.lib.visfs_ba_window_covariance(s.h, P(z), None) == abi.ERR_NOT_LOADED
    # no fixed pose (a root id outside the window, Estimator.cpp:252)
    w = synth.make_window("PROD")
    w["root_id"] = int(max(w["pose_ids"])) + 100
    wb = abi.WindowBuffers(w)
    rc, _ = s.solve_window(wb)
    assert rc == abi.OK
    assert s.lib.visfs_ba_window_covariance(s.h, P(z), None) == abi.ERR_SINGULAR
    # a passthrough leaves nothing to report on
    s0 = backend.Solver(abi.default_params(iterations=0, solver=0))
    rc, _ = s0.solve_window(abi.WindowBuffers(synth.make_window("PROD")))
    assert rc == abi.PASSTHROUGH
    assert s0.lib.visfs_ba_window_covariance(s0.h, P(z), None) == abi.ERR_NOT_LOADED
    s0.close()
    # WB: block half-bandwidth 29, no band plan
    wbw = abi.WindowBuffers(synth.make_window("WB"))
    rc, _ = s.solve_window(wbw)
    assert rc == abi.OK
    zz = np.zeros(36 * 64)
    assert s.lib.visfs_ba_window_covariance(s.h, P(zz), None) == abi.ERR_UNSUPPORTED
    assert "band" in s.lib.visfs_ba_last_error(s.h).decode()
    # batch handle
    olib = oracle_lib.load()
    gbs = [graph_of(olib.oracle_pack_window, s.params, synth.make_window("PROD", window_index=k))[1] for k in range(2)]
    s.batch_upload(gbs)
    assert s.lib.visfs_ba_graph_covariance(s.h, P(z), None, None) == abi.ERR_UNSUPPORTED
    assert s.lib.visfs_ba_window_covariance(s.h, P(z), None) == abi.ERR_UNSUPPORTED
    s.close()
    # the Ceres branch
    sc = backend.Solver(abi.default_params(iterations=10, framework=1))
    rc, _ = sc.solve_window(abi.WindowBuffers(synth.make_window("PROD")))
    assert rc == abi.OK
    assert sc.lib.visfs_ba_window_covariance(sc.h, P(z), None) == abi.ERR_UNSUPPORTED
    assert sc.lib.visfs_ba_graph_covariance(sc.h, P(z), None, None) == abi.ERR_UNSUPPORTED
    sc.close()
