"""An independent NumPy checker of the scan refinement (include/visfs_scan_refine.h), written from the
stated semantics: numpy.cos and numpy.sin of the yaw itself, plain numpy sums, numpy.linalg.solve.  It imports nothing of
visfs_amd.

The cost is the sum of squares of: per return (w_occ / sqrt(n)) * bicubic(correspondence cost)(r, c); w_t * (x - target_x),
w_t * (y - target_y); w_r * (yaw - initial_yaw).  The control is the Levenberg-Marquardt of SURVEY section 3.4 on the 3 x 3 system.
"""
import numpy as np

PAD = 2147483647 // 4                                     # kGridPadding
MIN_P = 0.1
MAX_P = 1.0 - MIN_P
MIN_CC = 1.0 - MAX_P
MAX_CC = 1.0 - MIN_P
MAX_VALUE = 32767
REJECTED = np.finfo(np.float64).max
ITERATIONS, NO_PROGRESS, TOLERANCE = 0, 1, 2


def value_cost_table():
    """Grid2D's value -> correspondence cost as getCorrespondenceCost returns it: float32, widened."""
    v = np.arange(32768, dtype=np.float64)
    k = (MAX_CC - MIN_CC) / 32766.0
    t = v * k + (MIN_CC - k)
    t[0] = MAX_CC
    return t.astype(np.float32).astype(np.float64)


TABLE = value_cost_table()


def cost_of_cells(cells):
    """The float costs (as doubles) of a sub-map's cells [ny][nx] (the update marker is not part of the value)."""
    return TABLE[np.asarray(cells).astype(np.int64) & MAX_VALUE]


def cost_of_gains(p0):
    """The same from a stack's level 0 (32767 - value, 0 for unknown)."""
    g = np.asarray(p0).astype(np.int64)
    return TABLE[np.where(g == 0, 0, MAX_VALUE - g)]


def _sample(cost, rows, cols):
    ny, nx = cost.shape
    y, x = rows - PAD, cols - PAD
    inside = (y >= 0) & (x >= 0) & (y < ny) & (x < nx)
    out = np.full(rows.shape, MAX_CC)
    out[inside] = cost[y[inside], x[inside]]
    return out


def _hermite(p0, p1, p2, p3, x):
    a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3)
    b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3)
    c = 0.5 * (-p0 + p2)
    return p1 + x * (c + x * (b + x * a)), c + x * (2.0 * b + 3.0 * a * x)


def bicubic(cost, r, c):
    """ceres::BiCubicInterpolator::Evaluate over the padded grid: f, df/dr, df/dc."""
    row, col = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    fr, dfr = [], []
    for i in range(4):
        p = [_sample(cost, row - 1 + i, col - 1 + j) for j in range(4)]
        f, d = _hermite(p[0], p[1], p[2], p[3], c - col)
        fr.append(f); dfr.append(d)
    f, dfdr = _hermite(fr[0], fr[1], fr[2], fr[3], r - row)
    dfdc, _ = _hermite(dfr[0], dfr[1], dfr[2], dfr[3], r - row)
    return f, dfdr, dfdc


class Problem:
    def __init__(self, cost, limits, points, initial, target, occupied_space_weight=1.0, translation_weight=10.0, rotation_weight=40.0):
        self.cost = np.asarray(cost, dtype=np.float64)
        self.res, self.max_x, self.max_y = limits["resolution"], limits["max_x"], limits["max_y"]
        assert self.cost.shape == (limits["num_y_cells"], limits["num_x_cells"])
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        self.px, self.py, self.n = p[:, 0], p[:, 1], len(p)
        self.yaw0 = float(initial[2])
        self.tx, self.ty = float(target[0]), float(target[1])
        self.wo, self.wt, self.wr = occupied_space_weight, translation_weight, rotation_weight

    def linearise(self, x, y, yaw):
        """(residuals [n + 3], Jacobian [n + 3][3]) at the pose."""
        C, S = np.cos(yaw), np.sin(yaw)
        Xr, Yr = C * self.px - S * self.py, S * self.px + C * self.py
        r = (self.max_x - (Xr + x)) / self.res - 0.5 + PAD
        c = (self.max_y - (Yr + y)) / self.res - 0.5 + PAD
        ny, nx = self.cost.shape
        r = np.clip(r, PAD - 4, PAD + 4 + ny)               # beyond it every sample is the constant
        c = np.clip(c, PAD - 4, PAD + 4 + nx)
        f, dfdr, dfdc = bicubic(self.cost, r, c)
        s = self.wo / np.sqrt(self.n)
        e = np.concatenate([s * f, [self.wt * (x - self.tx), self.wt * (y - self.ty), self.wr * (yaw - self.yaw0)]])
        J = np.zeros((self.n + 3, 3))
        J[:self.n, 0] = -s * dfdr / self.res
        J[:self.n, 1] = -s * dfdc / self.res
        J[:self.n, 2] = s * (dfdr * Yr - dfdc * Xr) / self.res
        J[self.n, 0] = self.wt; J[self.n + 1, 1] = self.wt; J[self.n + 2, 2] = self.wr
        return e, J

    def system(self, x, y, yaw):
        e, J = self.linearise(x, y, yaw)
        return J.T @ J, J.T @ e, float(np.sum(e * e))


def refine(problem, initial, max_iterations=20, function_tolerance=1e-6, max_rotation=1.0):
    """The refinement of `problem` from `initial`: a dict with the record's fields and `trace`, a list of
    (cost, lambda, accepted, x, y, yaw - initial yaw) per trial."""
    x, y, yaw = (float(v) for v in initial)
    yaw0 = problem.yaw0
    H, g, cost = problem.system(x, y, yaw)
    cost0 = cost
    lam, nu = 1e-5 * max(H[0, 0], H[1, 1], H[2, 2]), 2.0
    trace, it, term = [], 0, ITERATIONS
    done = not np.isfinite(cost)
    if done:
        term = NO_PROGRESS
    while not done:
        q, rho, accepted, before = 0, -1.0, False, cost
        while True:
            A = H + lam * np.eye(3)
            trial, ok = (x, y, yaw), True
            dx = np.zeros(3)
            try:
                np.linalg.cholesky(A)
                dx = np.linalg.solve(A, -g)
                trial = (x + dx[0], y + dx[1], yaw + dx[2])
                ok = bool(np.all(np.isfinite(dx))) and abs(trial[2] - yaw0) <= max_rotation
            except np.linalg.LinAlgError:
                ok = False
            temp, rho = REJECTED, -1.0
            if ok:
                Ht, gt, ct = problem.system(*trial)
                if np.isfinite(ct):
                    temp = ct
                    rho = (cost - ct) / (float(dx @ (lam * dx - g)) + 1e-3)
            accepted = rho > 0
            trace.append((temp, lam, 1.0 if accepted else 0.0, trial[0], trial[1], trial[2] - yaw0))
            if accepted:
                alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); nu = 2.0
                before = cost
                (x, y, yaw), H, g, cost = trial, Ht, gt, ct
            else:
                lam *= nu; nu *= 2.0
            q += 1
            if accepted or not rho < 0 or q == 10 or not np.isfinite(lam):
                break
        it += 1
        if q == 10 or rho == 0 or not np.isfinite(lam):
            done, term = True, NO_PROGRESS
        elif function_tolerance > 0 and before - cost <= function_tolerance * before:
            done, term = True, TOLERANCE
        elif it >= max_iterations:
            done, term = True, ITERATIONS
    return dict(x=x, y=y, yaw=yaw, initial_cost=cost0, final_cost=cost, iterations=it, trials=len(trace), termination=term,
                information=H, trace=trace)
