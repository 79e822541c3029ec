"""An independent NumPy checker of the 2-D pose graph (include/visfs_pose_graph.h), written from the
semantics: numpy.cos / numpy.sin of the yaw itself, a dense H, numpy.linalg.solve for the step and for M^-1 r, and the same
Levenberg-Marquardt control.  Edges are tuples (i, j, z[3], information[3][3], huber_delta)."""
import numpy as np

TWO_PI = 2.0 * np.pi
REJECTED = 1.7976931348623157e308
ITERATIONS, NO_PROGRESS, TOLERANCE, ROTATION_BOUND, PCG_BUDGET = range(5)
MAX_ROTATION = 1.0


def rows_of(fixed):
    """row of every vertex (-1: fixed), in vertex order"""
    out, n = [], 0
    for f in fixed:
        out.append(-1 if f else n)
        n += 0 if f else 1
    return np.array(out), n


def edge_terms(poses, e):
    """(residual, Ji, Jj) of one edge"""
    i, j, z = e[0], e[1], np.asarray(e[2], dtype=np.float64)
    ti, tj = poses[i], poses[j]
    c, s = np.cos(ti[2]), np.sin(ti[2])
    Rt = np.array([[c, s], [-s, c]])
    u = Rt @ (tj[:2] - ti[:2])
    d = tj[2] - ti[2] - z[2]
    r = np.array([u[0] - z[0], u[1] - z[1], d - TWO_PI * np.rint(d / TWO_PI)])
    Ji = np.array([[-c, -s, u[1]], [s, -c, -u[0]], [0.0, 0.0, -1.0]])
    Jj = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return r, Ji, Jj


def robust(chi2, delta):
    """(weight, cost) of g2o's Huber kernel on sqrt(chi2); delta == 0: none"""
    sq = np.sqrt(max(chi2, 0.0))
    if delta > 0.0 and sq > delta:
        return delta / sq, 2.0 * delta * sq - delta * delta
    return 1.0, chi2


def cost_of(poses, edges):
    total, chi2s = 0.0, []
    for e in edges:
        r, _, _ = edge_terms(poses, e)
        chi2 = float(r @ np.asarray(e[3], dtype=np.float64).reshape(3, 3) @ r)
        chi2s.append(chi2)
        total += robust(chi2, e[4] if len(e) > 4 else 0.0)[1]
    return total, np.array(chi2s)


def linearize(poses, fixed, edges):
    """dense H [3n][3n] and g [3n] over the free rows, the cost, chi2 per edge, the per-edge blocks"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    row, n = rows_of(fixed)
    H, g = np.zeros((3 * n, 3 * n)), np.zeros(3 * n)
    cost, chi2s, blocks = 0.0, [], []
    for e in edges:
        W = np.asarray(e[3], dtype=np.float64).reshape(3, 3)
        r, Ji, Jj = edge_terms(poses, e)
        chi2 = float(r @ W @ r)
        w, rho = robust(chi2, e[4] if len(e) > 4 else 0.0)
        cost += rho
        chi2s.append(chi2)
        blocks.append(np.stack([w * Ji.T @ W @ Ji, w * Ji.T @ W @ Jj, w * Jj.T @ W @ Jj]))
        for a, Ja in ((row[e[0]], Ji), (row[e[1]], Jj)):
            if a < 0:
                continue
            g[3 * a:3 * a + 3] += w * Ja.T @ W @ r
            for b, Jb in ((row[e[0]], Ji), (row[e[1]], Jj)):
                if b >= 0:
                    H[3 * a:3 * a + 3, 3 * b:3 * b + 3] += w * Ja.T @ W @ Jb
    return {"H": H, "g": g, "cost": cost, "chi2": np.array(chi2s), "rows": n, "edge_blocks": np.array(blocks)}


def band(H, preconditioner=1):
    """the block-tridiagonal (1) or block-diagonal (0) part of H in 3 x 3 blocks"""
    n = H.shape[0] // 3
    M = np.zeros_like(H)
    for r in range(n):
        for c in range(max(0, r - preconditioner), min(n, r + preconditioner + 1)):
            M[3 * r:3 * r + 3, 3 * c:3 * c + 3] = H[3 * r:3 * r + 3, 3 * c:3 * c + 3]
    return M


def precondition(H, lam, r, preconditioner=1):
    M = band(H, preconditioner) + lam * np.eye(H.shape[0])
    return np.linalg.solve(M, np.asarray(r, dtype=np.float64).reshape(-1)).reshape(-1, 3)


def pcg_iterations(H, g, lam, tolerance, preconditioner, max_iterations=100000):
    """the iterations of PCG on (H + lam I) x = -g, M applied by a dense solve, stopped at r.z <= tolerance^2 r0.z0"""
    A = H + lam * np.eye(H.shape[0])
    M = band(H, preconditioner) + lam * np.eye(H.shape[0])
    x, r = np.zeros_like(g), -g.copy()
    z = np.linalg.solve(M, r)
    p, rz = z.copy(), float(r @ z)
    rz0, it = rz, 0
    while rz > tolerance * tolerance * rz0 and it < max_iterations:
        q = A @ p
        a = rz / float(p @ q)
        x += a * p
        r -= a * q
        z = np.linalg.solve(M, r)
        rzn = float(r @ z)
        p = z + (rzn / rz) * p
        rz, it = rzn, it + 1
    return it, x


def optimize(poses, fixed, edges, max_iterations=20, function_tolerance=1e-6):
    """The control of section 9p with a dense solve for every step.  Returns a dict: poses, iterations, trials, termination,
    initial_cost, final_cost, chi2 and trace rows (cost, lambda, accepted, rho)."""
    start = np.asarray(poses, dtype=np.float64).reshape(-1, 3).copy()
    x = start.copy()
    row, n = rows_of(fixed)
    free = np.array([i for i in range(len(x)) if row[i] >= 0])
    L = linearize(x, fixed, edges)
    cost = cost0 = before = L["cost"]
    lam, nu = 1e-5 * np.max(np.diag(L["H"])), 2.0
    it = trials = q = 0
    term, done, rot_seen, trace = ITERATIONS, not np.isfinite(cost), False, []
    if done:
        term = NO_PROGRESS
    while not done:
        H, g = L["H"], L["g"]
        temp, rot, dx, xt = REJECTED, False, np.zeros(3 * n), x
        try:
            A = H + lam * np.eye(3 * n)
            np.linalg.cholesky(A)
            dx = np.linalg.solve(A, -g)
            xt = x.copy()
            xt[free] += dx.reshape(-1, 3)
            if not np.all(np.isfinite(xt)):
                pass
            elif np.any(np.abs(xt[:, 2] - start[:, 2]) > MAX_ROTATION):
                rot = True
            else:
                temp = cost_of(xt, edges)[0]
                if not np.isfinite(temp):
                    temp = REJECTED
        except np.linalg.LinAlgError:
            pass
        rho = -1.0
        if temp != REJECTED:
            rho = (cost - temp) / (float(dx @ (lam * dx - g)) + 1e-3)
            if np.isnan(rho):
                rho = -1.0
        accepted = rho > 0.0
        trace.append((temp, lam, 1.0 if accepted else 0.0, rho))
        rot_seen = rot_seen or rot
        if accepted:
            lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            nu = 2.0
            before, cost, x = cost, temp, xt
            L = linearize(x, fixed, edges)
        else:
            lam *= nu
            nu *= 2.0
        q += 1
        trials += 1
        if not accepted and rho < 0.0 and q < 10 and np.isfinite(lam):
            continue
        it += 1
        if q == 10 or rho == 0.0 or not np.isfinite(lam):
            done, term = True, NO_PROGRESS
        elif function_tolerance > 0.0 and before - cost <= function_tolerance * before:
            done, term = True, TOLERANCE
        elif it >= max_iterations:
            done, term = True, ITERATIONS
        if done and term != ITERATIONS and rot_seen:
            term = ROTATION_BOUND
        q, rot_seen = 0, False
    return {"poses": x, "iterations": it, "trials": trials, "termination": term, "initial_cost": cost0, "final_cost": cost,
            "chi2": cost_of(x, edges)[1], "trace": np.array(trace).reshape(-1, 4)}


def compose(a, z):
    """the pose a o z"""
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * z[0] - s * z[1], a[1] + s * z[0] + c * z[1], a[2] + z[2]])


def between(a, b):
    """the pose of b in the frame of a"""
    c, s = np.cos(a[2]), np.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    d = b[2] - a[2]
    return np.array([c * dx + s * dy, -s * dx + c * dy, d - TWO_PI * np.rint(d / TWO_PI)])
