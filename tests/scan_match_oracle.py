"""An independent plain-Python restatement of the correlative scan matcher, on submap_oracle.Grid.

It shares no code with the library: every candidate is scored from scratch, in generation order, with Python floats
(IEEE doubles) and math.* (the C library's acos, cos, sin, exp; hypot see `hypot`), each expression formed as section 9l
writes it.  The sum of a candidate is an exact integer, so there is no summation order to restate.
"""
import math

from submap_oracle import cell_index

KAPPA = 0.8 / 32766


def hypot(x, y):
    return math.hypot(x, y)


def eff(grid, x, y):
    """The value a match reads: unknown and outside cells as the maximal correspondence cost."""
    if not grid.contains(x, y):
        return 32767
    v = grid.cells[grid.nx * y + x]
    return 32767 if v == 0 else v & 32767


def search(grid, points, linear_window, angular_window):
    res = grid.res
    max_range = 3 * res
    for p in points:
        max_range = max(max_range, math.sqrt(p[0] * p[0] + p[1] * p[1]))
    step = (1 - 1e-3) * math.acos(1 - res * res / (2 * (max_range * max_range)))
    na = math.ceil(angular_window / step)
    nl = math.ceil(linear_window / res)
    return step, na, nl


def match(grid, guess, points, linear_window, angular_window, tw, rw):
    """Returns a dict: step, na, nl, cells [S][n] of (x, y), sums and scores as flat lists in generation order, the
    winner (k, xo, yo), its index, and the corrected pose."""
    gx, gy, gyaw = guess
    n = len(points)
    res = grid.res
    step, na, nl = search(grid, points, linear_window, angular_window)
    S = 2 * na + 1
    cells, sums, scores = [], [], []
    best, best_i, winner = None, None, None
    for k in range(S):
        theta = (k - na) * step
        a = gyaw + theta
        c, s = math.cos(a), math.sin(a)
        row = []
        for p in points:
            X = (c * p[0] - s * p[1]) + gx
            Y = (s * p[0] + c * p[1]) + gy
            row.append(cell_index(res, grid.max_x, grid.max_y, X, Y))
        cells.append(row)
        for xo in range(-nl, nl + 1):
            for yo in range(-nl, nl + 1):
                Q = 0
                for (x, y) in row:
                    Q += 32767 - eff(grid, x + xo, y + yo)
                cx = -yo * res
                cy = -xo * res
                t = hypot(cx, cy) * tw + abs(theta) * rw
                w = math.exp(-(t * t))
                score = (0.1 + (float(Q) * KAPPA) / float(n)) * w
                if best is None or score > best:          # max_element: the first of equal scores stays
                    best, best_i, winner = score, len(sums), (k, xo, yo)
                sums.append(Q)
                scores.append(score)
    k, xo, yo = winner
    return dict(step=step, na=na, nl=nl, S=S, cells=cells, sums=sums, scores=scores, winner=winner, index=best_i,
                score=best, sum=sums[best_i], x=gx + (-yo * res), y=gy + (-xo * res), yaw=gyaw + (k - na) * step)


def pretreat(points, T, origin, num_subdivisions, min_range, max_range, missing_ray_length):
    """Estimator::laserPretreatment (Estimator.cpp:116-157): a list of (origin, returns, misses)."""
    def tf(p):
        return [((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3] for r in range(3)]
    out = []
    n = len(points)
    if n == 0:
        return out
    for i in range(num_subdivisions):
        a, b = n * i // num_subdivisions, n * (i + 1) // num_subdivisions
        if a == b:
            continue
        o = tf(origin)
        ret, mis = [], []
        for p in points[a:b]:
            q = tf(p)
            d = [q[0] - o[0], q[1] - o[1], q[2] - o[2]]
            rng = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if rng >= min_range:
                if rng <= max_range:
                    ret.append(q)
                else:
                    f = missing_ray_length / rng
                    mis.append([o[0] + f * d[0], o[1] + f * d[1], o[2] + f * d[2]])
        out.append((o, ret, mis))
    return out
