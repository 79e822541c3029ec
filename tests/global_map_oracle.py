"""An independent NumPy checker of the global occupancy map (include/visfs_map.h), written from the
definition: no culling, `math.cos` / `math.sin` for every tile's yaw (as tests/scan_match_oracle.py forms its rotations), the
rounding restated, the inverse of the log-odds table by `argmin`.

A tile is a dict: `cells` ([ny][nx] uint16, markers allowed), `limits` (resolution, max_x, max_y, num_x_cells, num_y_cells) and
`pose` (x, y, yaw).  Every product and sum below is one NumPy operation on doubles, in the order of the definition, so nothing
is fused.
"""
import math

import numpy as np

ODDS, LATEST, OCCUPIED = 0, 1, 2
CLAMP = 1 << 30
MARGIN = 2


def round_index(v):
    """Half away from zero, saturating at +-2^30 (scan::round_index)."""
    v = np.asarray(v, dtype=np.float64)
    t = np.trunc(v)
    r = t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)
    return np.clip(r, -float(CLAMP), float(CLAMP)).astype(np.int64)


def odds_table_numpy(cost):
    """L from the correspondence-cost table by NumPy's own log (entry 0 unused)."""
    L = np.zeros(32768, dtype=np.int64)
    x = np.log((1.0 - cost[1:]) / cost[1:]) * 1048576.0
    L[1:] = (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)            # llround
    return L


def corners(tile):
    l = tile["limits"]
    x0, x1 = l["max_x"], l["max_x"] - float(l["num_y_cells"]) * l["resolution"]
    y0, y1 = l["max_y"], l["max_y"] - float(l["num_x_cells"]) * l["resolution"]
    c, s = math.cos(tile["pose"][2]), math.sin(tile["pose"][2])
    out = []
    for px, py in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        out.append(((c * px - s * py) + tile["pose"][0], (s * px + c * py) + tile["pose"][1]))
    return out


def limits_from_tiles(tiles, res):
    pts = [p for t in tiles for p in corners(t)]
    lo_x, hi_x = min(p[0] for p in pts), max(p[0] for p in pts)
    lo_y, hi_y = min(p[1] for p in pts), max(p[1] for p in pts)
    cx, fx, cy, fy = math.ceil(hi_x / res), math.floor(lo_x / res), math.ceil(hi_y / res), math.floor(lo_y / res)
    return dict(resolution=res, max_x=cx * res, max_y=cy * res, num_x_cells=cy - fy, num_y_cells=cx - fx)


def box(tile, limits):
    """The culling box (min_x, min_y, max_x, max_y) in output cells, or None when it misses the grid."""
    fx = [(limits["max_y"] - gy) / limits["resolution"] - 0.5 for _, gy in corners(tile)]
    fy = [(limits["max_x"] - gx) / limits["resolution"] - 0.5 for gx, _ in corners(tile)]
    out = []
    for f, n in ((fx, limits["num_x_cells"]), (fy, limits["num_y_cells"])):
        a, b = max(math.floor(min(f)) - MARGIN, 0), min(math.ceil(max(f)) + MARGIN, n - 1)
        if a > b:
            return None
        out.append((a, b))
    return (out[0][0], out[1][0], out[0][1], out[1][1])


def sample(tile, X, Y):
    """The tile's value at the map points (X, Y): 0 outside and for unknown cells."""
    l = tile["limits"]
    c, s = math.cos(tile["pose"][2]), math.sin(tile["pose"][2])
    dx, dy = X - tile["pose"][0], Y - tile["pose"][1]
    px, py = c * dx + s * dy, c * dy - s * dx
    jx = round_index((l["max_y"] - py) / l["resolution"] - 0.5)
    jy = round_index((l["max_x"] - px) / l["resolution"] - 0.5)
    inside = (jx >= 0) & (jy >= 0) & (jx < l["num_x_cells"]) & (jy < l["num_y_cells"])
    cells = np.asarray(tile["cells"], dtype=np.uint16).reshape(l["num_y_cells"], l["num_x_cells"]).astype(np.int64) & 32767
    v = cells[np.where(inside, jy, 0), np.where(inside, jx, 0)]
    return np.where(inside, v, 0)


def odds_inverse(L, S):
    """Per entry of S the v in 1 .. 32767 with the smallest |L[v] - S|, the smaller v of two equally near."""
    uniq, inv = np.unique(S, return_inverse=True)
    out = np.zeros(len(uniq), dtype=np.int64)
    for a in range(0, len(uniq), 256):
        out[a:a + 256] = np.abs(L[None, 1:] - uniq[a:a + 256, None]).argmin(axis=1) + 1
    return out[inv].reshape(S.shape)


def compose(tiles, L, combine=ODDS, resolution=0.05, limits=None):
    """(limits, cells [ny][nx] uint16, counts [ny][nx] uint8, drawn): drawn[k] is the boolean plane of the output cells tile k
    contributes to."""
    lim = dict(limits) if limits is not None else limits_from_tiles(tiles, resolution)
    nx, ny, res = lim["num_x_cells"], lim["num_y_cells"], lim["resolution"]
    iy, ix = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    X = lim["max_x"] - (iy + 0.5) * res
    Y = lim["max_y"] - (ix + 0.5) * res
    L = np.asarray(L, dtype=np.int64)
    count = np.zeros((ny, nx), dtype=np.int64)
    total = np.zeros((ny, nx), dtype=np.int64)
    latest = np.zeros((ny, nx), dtype=np.int64)
    least = np.full((ny, nx), 32768, dtype=np.int64)
    drawn = []
    for t in tiles:
        v = sample(t, X, Y)
        k = v > 0
        drawn.append(k)
        count += k
        total += np.where(k, L[v], 0)
        latest = np.where(k, v, latest)
        least = np.where(k, np.minimum(least, v), least)
    if combine == LATEST:
        value = latest
    elif combine == OCCUPIED:
        value = least
    else:
        assert combine == ODDS
        value = odds_inverse(L, np.clip(total, L[32767], L[1]))
    cells = np.where(count > 0, value, 0).astype(np.uint16)
    return lim, cells, np.minimum(count, 255).astype(np.uint8), drawn


def pose_from_anchor(frozen, now):
    """anchor_now o anchor_when_frozen^-1, written out with 3 x 3 homogeneous matrices."""
    def mat(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        return np.array([[c, -s, p[0]], [s, c, p[1]], [0.0, 0.0, 1.0]])
    T = mat(now) @ np.linalg.inv(mat(frozen))
    return np.array([T[0, 2], T[1, 2], math.atan2(T[1, 0], T[0, 0])])
