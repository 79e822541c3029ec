"""An independent restatement of the branch-and-bound scan matcher's definitions, on
submap_oracle.Grid, with NumPy.

It shares no code with the library and knows nothing of pruning: the level arrays are window maxima taken from P_0 by
their definition (never level from level), and the winner is found by scoring every leaf.  Rotation and discretisation are
scan_match_oracle's (Python floats, math.*).
"""
import math

import numpy as np

from scan_match_oracle import KAPPA, search
from submap_oracle import cell_index


def base(grid):
    """P_0 [ny][nx] int64: 0 for unknown, otherwise 32767 - (v & 32767)."""
    v = np.asarray(grid.cells, dtype=np.int64).reshape(grid.ny, grid.nx)
    return np.where(v == 0, 0, 32767 - (v & 32767))


def level(grid, h):
    """(P_h over x in [-e, nx), y in [-e, ny) as uint16 [ny + e][nx + e], e): P_h(x, y) = max over 0 <= dx, dy < 2^h of
    P_0(x + dx, y + dy), P_0 reading 0 outside the grid."""
    p0 = base(grid)
    w = 1 << h
    e = w - 1
    pad = np.zeros((grid.ny + 2 * e, grid.nx + 2 * e), dtype=np.int64)     # x in [-e, nx + e), y likewise
    pad[e:e + grid.ny, e:e + grid.nx] = p0
    rows = np.zeros((grid.ny + 2 * e, grid.nx + e), dtype=np.int64)        # the maximum over dx
    for dx in range(w):
        rows = np.maximum(rows, pad[:, dx:dx + grid.nx + e])
    out = np.zeros((grid.ny + e, grid.nx + e), dtype=np.int64)             # ... and over dy
    for dy in range(w):
        out = np.maximum(out, rows[dy:dy + grid.ny + e, :])
    return out.astype(np.uint16), e


def match(grid, guess, points, linear_window, angular_window):
    """Every leaf scored: a dict with step, na, nl, S, Q [S][L][L] (scan, xo, yo), the winner (k, xo, yo), its
    generation-order index, sum, score and pose.  The winner: maximal Q, earliest in generation order."""
    gx, gy, gyaw = guess
    n = len(points)
    res = grid.res
    step, na, nl = search(grid, points, linear_window, angular_window)
    S, L = 2 * na + 1, 2 * nl + 1
    p0 = base(grid)
    off = np.arange(-nl, nl + 1, dtype=np.int64)
    Q = np.zeros((S, L, L), dtype=np.int64)
    for k in range(S):
        a = gyaw + (k - na) * step
        c, s = math.cos(a), math.sin(a)
        cells = [cell_index(res, grid.max_x, grid.max_y, (c * p[0] - s * p[1]) + gx, (s * p[0] + c * p[1]) + gy) for p in points]
        cx = np.asarray([q[0] for q in cells], dtype=np.int64)
        cy = np.asarray([q[1] for q in cells], dtype=np.int64)
        X = cx[:, None, None] + off[None, :, None]                         # [n][xo][1]
        Y = cy[:, None, None] + off[None, None, :]                         # [n][1][yo]
        ok = (X >= 0) & (X < grid.nx) & (Y >= 0) & (Y < grid.ny)
        vals = p0[np.clip(Y, 0, grid.ny - 1), np.clip(X, 0, grid.nx - 1)]
        Q[k] = np.where(ok, vals, 0).sum(axis=0)
    index = int(np.argmax(Q))                                              # the first of equal maxima, in generation order
    k, xi, yi = np.unravel_index(index, Q.shape)
    k, xo, yo = int(k), int(xi) - nl, int(yi) - nl
    q = int(Q[k, xi, yi])
    score = (0.1 + (float(q) * KAPPA) / float(n)) * 1.0
    return dict(step=step, na=na, nl=nl, S=S, L=L, Q=Q, winner=(k, xo, yo), index=index, sum=q, score=score,
                x=gx + (-yo * res), y=gy + (-xo * res), yaw=gyaw + (k - na) * step)
