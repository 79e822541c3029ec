"""NumPy / plain-Python checker of the verified place query (include/visfs_place_verify.h).  It shares no code
with the library.

Stage 1 of a candidate is pnp_oracle.solve on the candidate's rows (stage1()).  Stage 2 is guided() on the model handed in, which is
the twin's stage-1 model (the way tracker_pnp_oracle stages a frame: what a later step starts from is the library's, so the step
itself can be held to exact equality), followed by pnp_oracle.after_winner on the guided rows from that model (stage2()).

guided(), as section 9x states it:
 2. every valid entry j with a finite point is projected in double (pnp_oracle.project); dropped when its depth is not positive or
    its pixel is not finite;
 3. a valid query i is in the window iff dx dx + dy dy <= r r in double, dx and dy from the query's float32 pixel, r the float32 radius;
 4. entry j picks the i in its window with Hamming distance D <= max_distance that minimises D * 1024 + i;
 5. query i keeps, among the entries that picked it, the one that minimises D * 1024 + j;
 6. the guided rows are the kept pairs in ascending query index.
"""
import numpy as np

import place_oracle as po
import pnp_oracle as pno

MAX_POINTS = 512
DEFAULTS = dict(guided=1, guided_radius=6.0, guided_max_distance=64)
F32 = np.float32


def in_window(pu, pv, qx, qy, radius):
    """The window test on scalars or arrays of queries."""
    dx = np.asarray(qx, dtype=F32).astype(np.float64) - pu
    dy = np.asarray(qy, dtype=F32).astype(np.float64) - pv
    r = float(F32(radius))
    return dx * dx + dy * dy <= r * r


def guided(R, t, K, slot, qset, radius, max_distance):
    """(pick int32 [512] per entry, keep int32 [512] per query, rows ROW_DTYPE [kept]); -1: none."""
    edesc, evalid = np.asarray(slot["desc"], dtype=np.uint8).reshape(-1, 32), np.asarray(slot["valid"])
    xyz = np.asarray(slot["xyz"], dtype=F32).reshape(-1, 3)
    qdesc, qvalid = np.asarray(qset["desc"], dtype=np.uint8).reshape(-1, 32), np.asarray(qset["valid"])
    qxy = np.asarray(qset["xy"], dtype=F32).reshape(-1, 2)
    ebits, qbits = np.unpackbits(edesc, axis=1), np.unpackbits(qdesc, axis=1)
    pick = np.full(MAX_POINTS, -1, dtype=np.int32)
    keep = np.full(MAX_POINTS, -1, dtype=np.int32)
    for j in range(len(edesc)):
        if not evalid[j] or not np.isfinite(xyz[j]).all():
            continue
        X = xyz[j].astype(np.float64)
        depth = float((R @ X + t)[2])
        if not depth > 0.0:
            continue
        pu, pv = pno.project(R, t, K, X[None, :])[0]
        if not (np.isfinite(pu) and np.isfinite(pv)):
            continue
        best = -1
        for i in np.flatnonzero(in_window(pu, pv, qxy[:, 0], qxy[:, 1], radius)) if len(qxy) else []:
            if not qvalid[i]:
                continue
            d = int((ebits[j] != qbits[i]).sum())
            if d <= max_distance and (best < 0 or d * 1024 + i < best):
                best = d * 1024 + int(i)
        pick[j] = best
    for i in range(len(qdesc)):
        best = -1
        for j in range(len(edesc)):
            if pick[j] >= 0 and (pick[j] & 1023) == i:
                key = (int(pick[j]) >> 10) * 1024 + j
                if best < 0 or key < best:
                    best = key
        keep[i] = best
    kept = np.flatnonzero(keep >= 0)
    rows = np.zeros(len(kept), dtype=po.ROW_DTYPE)
    for r, i in enumerate(kept):
        j = int(keep[i]) & 1023
        rows[r] = (i, j, int(keep[i]) >> 10, slot["ids"][j], xyz[j], qxy[i])
    return pick, keep, rows


def _to_xyz(query_xyz, rows):
    if query_xyz is None:
        return None
    return np.asarray(query_xyz, dtype=F32).reshape(-1, 3)[rows["query_index"]]


def stage1(params, K, Tir, rows, query_xyz=None):
    """pnp_oracle.solve on a candidate's rows."""
    return pno.solve(params, K, Tir, rows["from_xyz"], rows["to_xy"], _to_xyz(query_xyz, rows))


def stage2(params, K, Tir, R, t, rows, query_xyz=None):
    """The refinement of the guided rows from the model (R, t): dict(T, cov, inliers, passes, margin) of pnp_oracle.after_winner, or the
    sentinel with fewer than min_inliers rows."""
    if len(rows) < max(4, params["min_inliers"]):
        return {"T": np.zeros((4, 4)), "cov": np.eye(6), "inliers": [], "passes": [], "margin": np.inf}
    return pno.after_winner(R, t, K, Tir, np.ascontiguousarray(rows["from_xyz"]), np.ascontiguousarray(rows["to_xy"]), _to_xyz(query_xyz, rows), params)


def best(final_inliers, min_inliers):
    """final_inliers: per candidate the stage-2 count where stage 2 ran, else the stage-1 count."""
    out, most = -1, -1
    for c, n in enumerate(final_inliers):
        if n >= max(4, min_inliers) and n > most:
            out, most = c, n
    return out


def rt_of(tq):
    """(R, t) of a model given as t then the quaternion x y z w."""
    x, y, z, w = (float(v) for v in tq[3:])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(tq[:3], dtype=np.float64)


def closure_edge(T, cov):
    """(z, information, out_of_plane) of visfs_place_closure_edge."""
    T, cov = np.asarray(T, dtype=np.float64).reshape(4, 4), np.asarray(cov, dtype=np.float64).reshape(6, 6)
    ix = [0, 1, 5]
    S = cov[np.ix_(ix, ix)]
    info = np.linalg.inv(0.5 * (S + S.T))
    z = np.array([T[0, 3], T[1, 3], np.arctan2(T[1, 0], T[0, 0])])
    oop = np.array([T[2, 3], np.arctan2(T[2, 1], T[2, 2]), np.arctan2(-T[2, 0], np.hypot(T[0, 0], T[1, 0]))])
    return z, 0.5 * (info + info.T), oop
