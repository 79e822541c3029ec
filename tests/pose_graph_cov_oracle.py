"""An independent NumPy checker of the pose graph's covariances (include/visfs_pose_graph_cov.h), written
from the definition: Sigma = numpy.linalg.inv of the dense H of pose_graph_oracle.linearize at the poses handed in, the joint
covariance of a pair read out of it (zero blocks for a fixed vertex), the relative covariance through the derivatives of
z = a^-1 o b written out here."""
import numpy as np

import pose_graph_oracle as po


def sigma(poses, fixed, edges):
    """(Sigma [3n][3n], row_of [N])"""
    L = po.linearize(poses, fixed, edges)
    row, _ = po.rows_of(fixed)
    return np.linalg.inv(L["H"]), row


def block(S, row, a, b):
    ra, rb = row[a], row[b]
    if ra < 0 or rb < 0:
        return np.zeros((3, 3))
    return S[3 * ra:3 * ra + 3, 3 * rb:3 * rb + 3]


def joint(S, row, a, b):
    return np.block([[block(S, row, a, a), block(S, row, a, b)], [block(S, row, b, a), block(S, row, b, b)]])


def relative_jacobian(pa, pb):
    """d z / d (x_a, y_a, yaw_a, x_b, y_b, yaw_b) of z = a^-1 o b = (R(yaw_a)^T (t_b - t_a), yaw_b - yaw_a)"""
    c, s = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    J = np.zeros((3, 6))
    # z_x = c dx + s dy, z_y = -s dx + c dy
    J[0] = [-c, -s, -s * dx + c * dy, c, s, 0.0]
    J[1] = [s, -c, -c * dx - s * dy, -s, c, 0.0]
    J[2] = [0.0, 0.0, -1.0, 0.0, 0.0, 1.0]
    return J


def query(poses, fixed, edges, queries):
    """(joint [Q][6][6], relative [Q][3][3])"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    S, row = sigma(poses, fixed, edges)
    js, rs = [], []
    for a, b in queries:
        Jt = joint(S, row, a, b)
        J = relative_jacobian(poses[a], poses[b])
        js.append(Jt)
        rs.append(J @ Jt @ J.T)
    return np.array(js), np.array(rs)


def dense_from_blocks(n, row, edges, edge_blocks):
    """H [3n][3n] from the per-edge blocks (H_ii, H_ij, H_jj) of the linearize hook"""
    H = np.zeros((3 * n, 3 * n))
    for e, B in zip(edges, edge_blocks):
        ri, rj = row[e[0]], row[e[1]]
        if ri >= 0:
            H[3 * ri:3 * ri + 3, 3 * ri:3 * ri + 3] += B[0]
        if rj >= 0:
            H[3 * rj:3 * rj + 3, 3 * rj:3 * rj + 3] += B[2]
        if ri >= 0 and rj >= 0:
            H[3 * ri:3 * ri + 3, 3 * rj:3 * rj + 3] += B[1]
            H[3 * rj:3 * rj + 3, 3 * ri:3 * ri + 3] += B[1].T
    return H


def apply_blocks(n, row, edges, edge_blocks, x):
    """H x [3n] with H applied edge by edge from the blocks of the linearize hook (no dense matrix)"""
    x = np.asarray(x, dtype=np.float64).reshape(n, 3)
    y = np.zeros((n, 3))
    ei = np.array([row[e[0]] for e in edges])
    ej = np.array([row[e[1]] for e in edges])
    B = np.asarray(edge_blocks)
    mi, mj, mb = ei >= 0, ej >= 0, (ei >= 0) & (ej >= 0)
    np.add.at(y, ei[mi], np.einsum("kab,kb->ka", B[mi, 0], x[ei[mi]]))
    np.add.at(y, ej[mj], np.einsum("kab,kb->ka", B[mj, 2], x[ej[mj]]))
    np.add.at(y, ei[mb], np.einsum("kab,kb->ka", B[mb, 1], x[ej[mb]]))
    np.add.at(y, ej[mb], np.einsum("kba,kb->ka", B[mb, 1], x[ei[mb]]))
    return y.reshape(-1)


def residual_inf(n, row, edges, edge_blocks, x, col):
    """|| H x - e_col ||_inf"""
    y = apply_blocks(n, row, edges, edge_blocks, x)
    y[col] -= 1.0
    return float(np.max(np.abs(y)))


def norm_inf(n, row, edges, edge_blocks):
    """an upper bound of || H ||_inf: the row sums of the blocks' absolute values"""
    return float(np.max(apply_blocks(n, row, edges, np.abs(np.asarray(edge_blocks)), np.ones((n, 3)))))
