"""CPU tests of the marginal-covariance boundary (include/visfs_ba.h, ABI 9), no GPU needed:

* visfs_ba_hook_band_selinv — the block-banded factorisation and the selected inversion the kernels run (ba_cov.hpp, compiled for
  the host) — against numpy.linalg.inv on random SPD block-banded matrices, every block of the band;
* visfs_ba_pose_cov_to_world against a central finite-difference Jacobian of visfs_ba_unpack_pose o CameraPose::update;
* the ABI version and the export list."""
import ctypes as C

import numpy as np
import pytest

from test_oracle_algebra import _oplus
from visfs_amd import abi

_pd = C.POINTER(C.c_double)


def P(a):
    return a.ctypes.data_as(_pd)


def _random_band(n, B, rng, weak_rows=()):
    """A random SPD matrix of n 6x6 block rows with block half-bandwidth B: M0 = L L^T + I / 2, L block lower-banded; returned as
    (M = diag(s) M0 diag(s), s, M0) with s = 1e-4 on the block rows in `weak_rows` (a pose that sees few landmarks): cond(M) grows by ~1e8
    per such row while M0 stays well conditioned."""
    N = 6 * n
    L = np.zeros((N, N))
    for i in range(n):
        for d in range(min(B, i) + 1):
            j = i - d
            L[6 * i:6 * i + 6, 6 * j:6 * j + 6] = rng.standard_normal((6, 6)) * (1.0 if d == 0 else 0.3)
    M = L @ L.T + 0.5 * np.eye(N)
    # L L^T has block half-bandwidth B: L's band is B wide below the diagonal, the product's band is B wide as well
    s = np.ones(N)
    for r in weak_rows:
        s[6 * r:6 * r + 6] = 1e-4
    return (s[:, None] * M) * s[None, :], s, M


def _to_band(M, n, B):
    W = B + 1
    out = np.zeros((n, W, 6, 6))
    for I in range(n):
        for d in range(W):
            if I - d >= 0:
                out[I, d] = M[6 * I:6 * I + 6, 6 * (I - d):6 * (I - d) + 6]
    return out


def _selinv(hiplib, M, n, B):
    S = np.ascontiguousarray(_to_band(M, n, B))
    Sg = np.full_like(S, np.nan)
    rc = hiplib.visfs_ba_hook_band_selinv(n, B, P(S), P(Sg))
    return rc, Sg


@pytest.mark.parametrize("n,B,weak", [(1, 0, ()), (2, 1, ()), (7, 9, ()), (49, 9, ()), (60, 15, ()), (40, 21, ()),
                                      (49, 9, (17,)), (30, 5, (0, 29))])
def test_band_selinv_matches_the_dense_inverse(hiplib, n, B, weak):
    rng = np.random.default_rng(1000 * n + B + len(weak))
    Bm = min(B, n - 1)                                           # (B >= n: every block is in the band)
    M, sc, M0 = _random_band(n, Bm, rng, weak)
    rc, Sg = _selinv(hiplib, M, n, B)
    assert rc == abi.OK
    if weak:
        assert np.linalg.cond(M) > 1e8 and np.linalg.cond(M0) < 1e4
    # M^-1 = diag(1/s) M0^-1 diag(1/s) with M0 well conditioned: the reference carries no error of its own.  A block Cholesky is
    # insensitive to a diagonal scaling, so the check is made on the RESCALED blocks s_I Sigma_IJ s_J against those of M0^-1: every block
    # to 1e-10 relative Frobenius, the ill-conditioned cases included (a normwise bound against ||M^-1|| would say nothing about the
    # O(1) blocks outside the weak rows)
    M0inv = np.linalg.inv(M0)
    floor = 1e-3 * np.linalg.norm(M0inv, 2)
    for I in range(n):
        for d in range(B + 1):
            if I - d < 0:
                assert not Sg[I, d].any()                        # unused slots are written as zeros
                continue
            J = I - d
            ref = M0inv[6 * I:6 * I + 6, 6 * J:6 * J + 6]
            mine = sc[6 * I:6 * I + 6, None] * Sg[I, d] * sc[None, 6 * J:6 * J + 6]
            err = np.linalg.norm(mine - ref)
            assert err <= 1e-10 * max(np.linalg.norm(ref), floor), (I, d, err, np.linalg.norm(ref))


def test_band_selinv_refuses_an_indefinite_matrix(hiplib):
    rng = np.random.default_rng(7)
    n, B = 12, 3
    M = _random_band(n, B, rng)[0]
    M[6 * 5 + 2, 6 * 5 + 2] = -50.0                              # an indefinite pivot
    rc, _ = _selinv(hiplib, M, n, B)
    assert rc == abi.ERR_SINGULAR
    assert hiplib.visfs_ba_hook_band_selinv(0, 1, P(np.zeros(36)), P(np.zeros(36))) == abi.ERR_BAD_ARGUMENT


def _rand_quat(rng):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _log(R):
    """SO(3) logarithm (small angles: the finite differences below stay far from pi)."""
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    return v if th < 1e-8 else v * th / np.sin(th)


def _unpack(hiplib, tq, Trc):
    out = np.zeros(12)
    hiplib.visfs_ba_unpack_pose(P(np.ascontiguousarray(tq)), P(Trc), P(out))
    return out.reshape(3, 4)


@pytest.mark.parametrize("seed", range(6))
def test_pose_cov_to_world_matches_finite_differences(hiplib, seed):
    rng = np.random.default_rng(seed)
    tq = np.concatenate([rng.standard_normal(3) * 3.0, _rand_quat(rng)])
    Trc = np.concatenate([_quat_R(_rand_quat(rng)), rng.standard_normal((3, 1)) * 0.3], axis=1).reshape(12).copy()
    A = rng.standard_normal((6, 6))
    cov = A @ A.T * 1e-3
    T0 = _unpack(hiplib, tq, Trc)

    def f(d):
        T = _unpack(hiplib, _oplus(tq, d), Trc)
        return np.concatenate([T[:, 3] - T0[:, 3], _log(T[:, :3] @ T0[:, :3].T)])

    h = 1e-6
    J = np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6); e[k] = h
        J[:, k] = (f(e) - f(-e)) / (2 * h)
    ref = J @ cov @ J.T
    out = np.zeros(36)
    hiplib.visfs_ba_pose_cov_to_world(P(tq), P(Trc), P(np.ascontiguousarray(cov)), P(out))
    out = out.reshape(6, 6)
    assert np.abs(out - ref).max() <= 1e-7 * np.abs(ref).max(), np.abs(out - ref).max()
    # the first-order Jacobian as the header states it
    R_cw = _quat_R(tq[3:])
    p = T0[:, 3]
    px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
    Jh = np.block([[-R_cw.T, px @ R_cw.T], [np.zeros((3, 3)), -R_cw.T]])
    assert np.abs(Jh @ cov @ Jh.T - out).max() <= 1e-12 * np.abs(out).max()


def test_abi_version_and_error_code(hiplib):
    assert abi.ABI_VERSION == 10
    assert abi.ERR_SINGULAR == 10
    assert hiplib.visfs_ba_abi_version() == 10
    from visfs_amd import backend
    for name in ("visfs_ba_graph_covariance", "visfs_ba_window_covariance", "visfs_ba_pose_cov_to_world", "visfs_ba_hook_band_selinv"):
        assert name in backend.EXPORTS
        assert hasattr(hiplib, name)
