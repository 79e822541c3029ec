"""NumPy checker of the fundamental-matrix cull (include/visfs_fund.h).  It shares no code with the library and
is the definition of record for the six steps:

1. rows: a row is kept when its four coordinates are finite, in input order; m kept rows.  m < 7: not applied, the status passes, mask
   and F zero.  m == 7: no search, the mask is 1 on every kept row, F the first model of rows 0..6
   (reported as the one hypothesis of the call, unscored).  m >= 8: the search.
2. conditioning: one Hartley transform per image (centroid, mean distance sqrt 2), serial double sums in kept-row order; a mean
   distance of zero gives scale 1.
3. samples: hypothesis h takes seven distinct rows, r_k = mix64(seed + 0x9E3779B97F4A7C15 (7h + k + 1)), j_k = r_k mod (m - k), stepped
   past the rows already taken in ascending order.
4. seven-point solver in conditioned coordinates.  Here the null space comes from numpy.linalg.svd and the roots of det(f1 + x f2)
   from numpy.roots; the library eliminates with full pivoting, bisects, deflates and polishes.  A sample is invalid when A has rank
   below 7 (here: sigma_7 < RANK_LIMIT sigma_1) or the cubic's leading coefficient is below LEAD_LIMIT of its largest.  Every real
   root gives F^ scaled to unit Frobenius norm with its largest-magnitude entry positive; the models are ordered by ascending
   F^[2][2]; F = T2^T F^ T1.
5. score: e_i = float32(max(d1^2 / (a1^2 + b1^2), d2^2 / (a2^2 + b2^2))) on the raw pixels in double, inlier iff e_i <= float32(thr thr);
   the largest count wins, ties to the lowest h and then the lowest model index; a winner needs 7; every hypothesis is evaluated.
6. result: the winner's inlier flags; with no winner mask and F are zero and applied is 1.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
F32 = np.float32
RANK_LIMIT = 1e-9          # sigma_7 / sigma_1 (the library: smallest pivot / first pivot of the full-pivot elimination)
LEAD_LIMIT = 1e-10         # |c3| / max |c_i|
REAL_LIMIT = 1e-7          # |imag| / (1 + |root|) below which a root of numpy.roots is real


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, h, m):
    taken, out = [], []
    for k in range(7):
        j = mix64((seed + 0x9E3779B97F4A7C15 * (7 * h + k + 1)) & MASK) % (m - k)
        for t in sorted(taken):
            if j >= t:
                j += 1
        taken.append(j)
        out.append(j)
    return out


def hartley(xy):
    """xy [m][2] double -> the 3x3 transform; serial sums in row order."""
    m = len(xy)
    sx = sy = 0.0
    for x, y in xy:
        sx += float(x); sy += float(y)
    cx, cy = sx / m, sy / m
    sd = 0.0
    for x, y in xy:
        sd += math.sqrt((float(x) - cx) ** 2 + (float(y) - cy) ** 2)
    mean = sd / m
    s = math.sqrt(2.0) / mean if mean > 0.0 else 1.0
    return np.array([[s, 0.0, -s * cx], [0.0, s, -s * cy], [0.0, 0.0, 1.0]])


def condition(T, xy):
    return np.stack([(xy[:, 0] + T[0, 2] / T[0, 0]) * T[0, 0], (xy[:, 1] + T[1, 2] / T[1, 1]) * T[1, 1]], axis=1)


def canonical(F):
    """Unit Frobenius norm, the largest-magnitude entry positive.  Returns (F^, gap between the two largest magnitudes of F^)."""
    F = F / np.linalg.norm(F)
    a = np.abs(F).ravel()
    k = int(np.argmax(a))
    if F.ravel()[k] < 0:
        F = -F
    top = np.sort(a)
    return F, float(top[-1] - top[-2])


def seven_point(p1, p2):
    """p1, p2 [7][2] conditioned (double).  Returns (list of F^ ordered by F^[2][2], diagnostics)."""
    diag = {"rank_ratio": 0.0, "lead_ratio": None, "max_real_imag": 0.0, "min_complex_imag": np.inf, "key_sep": np.inf, "sign_gap": np.inf}
    x1, y1, x2, y2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(7)], axis=1)
    if not np.isfinite(A).all():
        return [], diag
    _, sv, Vt = np.linalg.svd(A)
    diag["rank_ratio"] = float(sv[6] / sv[0]) if sv[0] > 0 else 0.0
    if not diag["rank_ratio"] >= RANK_LIMIT:
        return [], diag
    f1, f2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    # det(f1 + x f2) by interpolation-free polynomial arithmetic: each entry is the polynomial (f2, f1), highest power first
    P = [[np.array([f2[i, j], f1[i, j]]) for j in range(3)] for i in range(3)]

    def minor(a, b, c, d):
        return np.polysub(np.polymul(a, d), np.polymul(b, c))
    cubic = np.polyadd(np.polysub(np.polymul(P[0][0], minor(P[1][1], P[1][2], P[2][1], P[2][2])),
                                  np.polymul(P[0][1], minor(P[1][0], P[1][2], P[2][0], P[2][2]))),
                       np.polymul(P[0][2], minor(P[1][0], P[1][1], P[2][0], P[2][1])))
    cubic = np.concatenate([np.zeros(4 - len(cubic)), cubic])
    big = float(np.abs(cubic).max())
    diag["lead_ratio"] = float(abs(cubic[0]) / big) if big > 0 else 0.0
    if not diag["lead_ratio"] >= LEAD_LIMIT:
        return [], diag
    models = []
    for r in np.roots(cubic):
        rel = abs(r.imag) / (1.0 + abs(r))
        if rel < REAL_LIMIT:
            diag["max_real_imag"] = max(diag["max_real_imag"], rel)
            Fh, gap = canonical(f1 + r.real * f2)
            diag["sign_gap"] = min(diag["sign_gap"], gap)
            models.append(Fh)
        else:
            diag["min_complex_imag"] = min(diag["min_complex_imag"], rel)
    models.sort(key=lambda F: F[2, 2])
    for a, b in zip(models, models[1:]):
        diag["key_sep"] = min(diag["key_sep"], float(b[2, 2] - a[2, 2]))
    return models, diag


def errors(F, xy1, xy2):
    """FMEstimatorCallback::computeError on raw pixels [m][2] (double): float32 [m]."""
    x1, y1, x2, y2 = xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]
    with np.errstate(all="ignore"):
        a = F[0, 0] * x1 + F[0, 1] * y1 + F[0, 2]
        b = F[1, 0] * x1 + F[1, 1] * y1 + F[1, 2]
        c = F[2, 0] * x1 + F[2, 1] * y1 + F[2, 2]
        d2 = x2 * a + y2 * b + c
        e2 = d2 * d2 / (a * a + b * b)
        a = F[0, 0] * x2 + F[1, 0] * y2 + F[2, 0]
        b = F[0, 1] * x2 + F[1, 1] * y2 + F[2, 1]
        c = F[0, 2] * x2 + F[1, 2] * y2 + F[2, 2]
        d1 = x1 * a + y1 * b + c
        e1 = d1 * d1 / (a * a + b * b)
        return np.maximum(e1, e2).astype(F32)


def threshold(pixel_error):
    thr = F32(pixel_error) if pixel_error > 0 else F32(3.0)
    return F32(float(thr) * float(thr))


def score(models, T1, T2, xy1, xy2, thr2):
    """models [H][<=3] of F^ -> (counts [H][3], winner (h, k) or (-1, -1), the smallest |sqrt e - sqrt thr2| in px, ties)."""
    counts, best, win, margin = [], 6, (-1, -1), np.inf
    for h, ms in enumerate(models):
        row = [0, 0, 0]
        for k, Fh in enumerate(ms):
            e = errors(T2.T @ np.asarray(Fh) @ T1, xy1, xy2)
            row[k] = int((e <= thr2).sum())
            fin = e[np.isfinite(e)].astype(np.float64)
            if len(fin):
                margin = min(margin, float(np.abs(np.sqrt(fin) - math.sqrt(float(thr2))).min()))
            if row[k] > best:
                best, win = row[k], (h, k)
        counts.append(row)
    ties = sum(1 for row in counts for c in row if c == best) if win[0] >= 0 else 0
    return counts, win, margin, ties


def cull(params, from_xy, to_xy, status):
    """params: dict with pixel_error, iterations, seed.  Returns a dict of everything the library reports."""
    a = np.asarray(from_xy, dtype=F32).reshape(-1, 2)
    b = np.asarray(to_xy, dtype=F32).reshape(-1, 2)
    status = np.asarray(status, dtype=np.uint8)
    n = len(a)
    keep = np.nonzero(np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1))[0]
    m = len(keep)
    out = {"keep": keep, "m": m, "applied": 0, "mask": np.zeros(n, dtype=np.uint8), "status": (status != 0).astype(np.uint8), "F": np.zeros((3, 3)),
           "samples": [], "models": [], "counts": [], "winner": (-1, -1), "diags": [], "margin": np.inf, "ties": 0, "n_inliers": 0,
           "T1": np.zeros((3, 3)), "T2": np.zeros((3, 3))}
    if m < 7:
        return out
    out["applied"] = 1
    xy1, xy2 = a[keep].astype(np.float64), b[keep].astype(np.float64)
    T1, T2 = hartley(xy1), hartley(xy2)
    out["T1"], out["T2"] = T1, T2
    c1, c2 = condition(T1, xy1), condition(T2, xy2)
    if m == 7:
        models, diag = seven_point(c1, c2)
        out["diags"].append(diag)
        out["mask"][keep] = 1
        out["n_inliers"] = 7
        out["samples"], out["models"], out["counts"] = [list(range(7))], [models], [[0, 0, 0]]
        if models:
            out["F"] = T2.T @ models[0] @ T1
            out["winner"] = (0, 0)
        out["status"] = out["status"] & out["mask"]
        return out
    thr2 = threshold(params["pixel_error"])
    for h in range(params["iterations"]):
        s = sample(params["seed"], h, m)
        models, diag = seven_point(c1[s], c2[s])
        out["samples"].append(s); out["models"].append(models); out["diags"].append(diag)
    out["counts"], out["winner"], out["margin"], out["ties"] = score(out["models"], T1, T2, xy1, xy2, thr2)
    h, k = out["winner"]
    if h >= 0:
        F = T2.T @ out["models"][h][k] @ T1
        out["F"] = F
        out["mask"][keep] = (errors(F, xy1, xy2) <= thr2).astype(np.uint8)
        out["n_inliers"] = int(out["mask"].sum())
    out["status"] = out["status"] & out["mask"]
    return out
