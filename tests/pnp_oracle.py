"""NumPy checker of the PnP-RANSAC pose guess (include/visfs_pnp.h).  It shares no code with the library and is
the definition of record for the seven steps:

1. correspondences: the rows with a finite from_xyz, in input order; fewer than min_inliers (raised to 4): the zero transform.
2. samples: hypothesis h takes four distinct rows, r_k = mix64(seed + 0x9E3779B97F4A7C15 (4h + k + 1)), j_k = r_k mod (m - k), stepped
   past the rows already taken in ascending order.
3. minimal solver: P3P on rows 0-2 of the sample (every solution with three positive depths), the solution closest on row 3.  A triad
   whose world points are collinear within sin^2 < 1e-8 is invalid.  Here the quartic comes from polynomial arithmetic and
   numpy.roots, and the pose from the SVD (Kabsch) of the two triads; the library uses Ferrari and orthonormal frames.
4. score: e_i = float32(sqrt(dx^2 + dy^2)) of the double projection (iz = 1/z, or 1 for z == 0); inlier iff e_i <= float32(reproj_error);
   the largest count wins, ties to the lowest h; every hypothesis is evaluated.
5. refit: the least-squares pose on the winner's inliers from the winner's model (here: Gauss-Newton with an exponential-map update,
   run to convergence; the library: Levenberg-Marquardt, at most 20 iterations).
6. the refinement loop of MultiviewGeometry.cpp:241-313 as written.
7. transform (Tir pnp)^-1 and the covariance of :159-205.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
F32 = np.float32


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def sample(seed, h, m):
    taken, out = [], []
    for k in range(4):
        j = mix64((seed + 0x9E3779B97F4A7C15 * (4 * h + k + 1)) & MASK) % (m - k)
        for t in sorted(taken):
            if j >= t:
                j += 1
        taken.append(j)
        out.append(j)
    return out


def project(R, t, K, X):
    """X [n][3] double -> pixels [n][2] double, cv::projectPoints without distortion."""
    pc = X @ R.T + t
    z = pc[:, 2]
    iz = np.where(z != 0.0, 1.0 / np.where(z != 0.0, z, 1.0), 1.0)
    return np.stack([K[0] * pc[:, 0] * iz + K[2], K[1] * pc[:, 1] * iz + K[3]], axis=1)


def errors(R, t, K, X, uv):
    d = uv - project(R, t, K, X)
    return np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2).astype(F32)


def kabsch(P, Q):
    """The rotation and translation with Q_i = R P_i + t for two congruent triads."""
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, qc - R @ pc


def p3p(K, X, uv):
    """X [4][3], uv [4][2] (double).  Returns (best (R, t) or None, diagnostics)."""
    diag = {"sin2": None, "max_real_imag": 0.0, "min_complex_imag": np.inf, "root_sep": np.inf, "depth_margin": np.inf, "fourth_gap": np.inf, "n_solutions": 0}
    P = X[:3]
    d1, d2 = P[1] - P[0], P[2] - P[0]
    cr = np.cross(d1 / np.linalg.norm(d1), d2) if np.linalg.norm(d1) > 0 else np.zeros(3)
    sin2 = float(cr @ cr / (d2 @ d2)) if d2 @ d2 > 0 and np.linalg.norm(d1) > 0 else 0.0
    diag["sin2"] = sin2
    if not sin2 >= 1e-8:
        return None, diag
    j = np.stack([(uv[:3, 0] - K[2]) / K[0], (uv[:3, 1] - K[3]) / K[1], np.ones(3)], axis=1)
    j /= np.linalg.norm(j, axis=1)[:, None]
    a2, b2, c2 = ((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum()
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    # s2 = u s1, s3 = v s1;  b2 (u^2 + v^2 - 2 u v ca) = a2 Q,  b2 (1 + u^2 - 2 u cg) = c2 Q,  Q = 1 + v^2 - 2 v cb
    Q = np.array([1.0, -2.0 * cb, 1.0])                                  # highest power first
    N = np.polysub((a2 - c2) * Q, b2 * np.array([1.0, 0.0, -1.0]))       # the difference of the two: u D = N
    Dp = 2.0 * b2 * np.array([-ca, cg])
    quartic = np.polysub(b2 * np.polyadd(np.polyadd(np.polymul(Dp, Dp), np.polymul(N, N)), -2.0 * cg * np.polymul(N, Dp)),
                         c2 * np.polymul(Q, np.polymul(Dp, Dp)))
    roots = np.roots(quartic)
    real = []
    for r in roots:
        rel = abs(r.imag) / (1.0 + abs(r))
        if rel < 1e-7:
            real.append(r.real)
            diag["max_real_imag"] = max(diag["max_real_imag"], rel)
        else:
            diag["min_complex_imag"] = min(diag["min_complex_imag"], rel)
    real.sort()
    for x, y in zip(real, real[1:]):
        diag["root_sep"] = min(diag["root_sep"], abs(y - x) / (1.0 + abs(x)))
    sols = []
    for v in real:
        den = np.polyval(Dp, v)
        u = np.polyval(N, v) / den
        diag["depth_margin"] = min(diag["depth_margin"], abs(u), abs(v), abs(den) / (2.0 * b2))
        if not (u > 0 and v > 0):
            continue
        s1 = math.sqrt(b2 / np.polyval(Q, v))
        R, t = kabsch(P, np.stack([s1 * j[0], u * s1 * j[1], v * s1 * j[2]]))
        d = uv[3] - project(R, t, K, X[3:4])[0]
        sols.append((float(np.hypot(d[0], d[1])), R, t))
    diag["n_solutions"] = len(sols)
    if not sols:
        return None, diag
    sols.sort(key=lambda s: s[0])
    if len(sols) > 1:
        diag["fourth_gap"] = sols[1][0] - sols[0][0]
    return (sols[0][1], sols[0][2]), diag


def expm_so3(w):
    th = float(np.linalg.norm(w))
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + math.sin(th) / th * Kx + (1.0 - math.cos(th)) / th ** 2 * (Kx @ Kx)


def refit(R, t, K, X, uv, iterations=60):
    """Gauss-Newton on the pixel residual with R <- exp(w) R, t <- t + dt, run to convergence."""
    for _ in range(iterations):
        rx = X @ R.T
        pc = rx + t
        iz = 1.0 / pc[:, 2]
        e = uv - np.stack([K[0] * pc[:, 0] * iz + K[2], K[1] * pc[:, 1] * iz + K[3]], axis=1)
        n = len(X)
        J = np.zeros((n, 2, 6))
        A = np.zeros((n, 2, 3))
        A[:, 0, 0] = K[0] * iz; A[:, 0, 2] = -K[0] * pc[:, 0] * iz ** 2
        A[:, 1, 1] = K[1] * iz; A[:, 1, 2] = -K[1] * pc[:, 1] * iz ** 2
        J[:, :, :3] = A
        S = np.zeros((n, 3, 3))                                         # -[R X]x
        S[:, 0, 1] = rx[:, 2]; S[:, 0, 2] = -rx[:, 1]; S[:, 1, 0] = -rx[:, 2]; S[:, 1, 2] = rx[:, 0]; S[:, 2, 0] = rx[:, 1]; S[:, 2, 1] = -rx[:, 0]
        J[:, :, 3:] = A @ S
        d = np.linalg.lstsq(J.reshape(-1, 6), e.reshape(-1), rcond=None)[0]
        t = t + d[:3]
        R = expm_so3(d[3:]) @ R
        if np.abs(d).max() < 1e-14:
            break
    return R, t


def umean(e):
    buf = F32(0)
    for x in e:
        buf = F32(buf + x)
    return F32(buf / F32(len(e)))


def uvariance(e, mean):
    s = 0.0
    for x in e:
        d = F32(x - mean)
        s += float(F32(d * d))
    return F32(s / (len(e) - 1))


def select(R, t, K, X, uv, thr):
    e = errors(R, t, K, X, uv)
    keep = np.nonzero(e <= thr)[0]
    return e, keep.tolist()


def refine_loop(R, t, K, X, uv, L0, thr0, sigma, min_inliers, refine_iterations):
    """MultiviewGeometry.cpp:241-313.  Returns (returned list, R, t, passes); a pass: (R, t, threshold, errors of all rows, list)."""
    thr, it, changed = thr0, 0, False
    prev, new, sizes, passes = list(L0), [], [], []
    while True:
        R, t = refit(R, t, K, X[prev], uv[prev])
        sizes.append(len(prev))
        e, new = select(R, t, K, X, uv, thr)
        passes.append((R, t, thr, e, list(new)))
        if len(new) < min_inliers:
            it += 1
            if it >= refine_iterations:
                break
        else:
            err = e[new]
            mean = umean(err)
            var = uvariance(err, mean)
            thr = min(thr0, F32(F32(sigma) * F32(math.sqrt(float(var)))))
            changed = False
            prev, new = new, prev
            if len(new) != len(prev):
                if len(sizes) >= min_inliers and sizes[-1] == sizes[-3] and sizes[-2] == sizes[-4]:
                    break
                changed = True
            else:
                changed = prev != new
        if not changed:
            break
        it += 1
        if not it < refine_iterations:
            break
    return new, R, t, passes


def angle3d(a, b):
    a, b = a.astype(F32), b.astype(F32)
    na, nb = F32(np.sqrt(F32(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])), F32(np.sqrt(F32(b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]))
    ua, ub = (a / na).astype(F32), (b / nb).astype(F32)
    rad = F32(F32(ua[0] * ub[0] + ua[1] * ub[1]) + ua[2] * ub[2])
    return F32(math.acos(float(min(max(rad, F32(-1)), F32(1)))))


def finalize(R, t, K, Tir, X32, uv32, inliers, to_xyz):
    """(T [4][4], cov [6][6]) of :147-205; inliers index the kept rows, to_xyz is in kept-row order (or None)."""
    pnp = np.eye(4); pnp[:3, :3] = R; pnp[:3, 3] = t
    Ti = np.eye(4); Ti[:3] = np.asarray(Tir, dtype=np.float64).reshape(3, 4)
    T = np.linalg.inv(Ti @ pnp)
    cov = np.eye(6)
    if to_xyz is not None:
        d2, ang = [], []
        for i in inliers:
            q = to_xyz[i]
            if not np.isfinite(q).all():
                continue
            npt = (T[:3, :3] @ q.astype(np.float64) + T[:3, 3]).astype(F32)
            d = (X32[i] - npt).astype(F32)
            d2.append(F32(F32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            v1 = (X32[i].astype(np.float64) - T[:3, 3]).astype(F32)
            v2 = (npt.astype(np.float64) - T[:3, 3]).astype(F32)
            ang.append(angle3d(v1, v2))
        if d2:
            d2.sort(); ang.sort()
            cov[:3, :3] *= 2.1981 * float(d2[len(d2) >> 1])
            cov[3:, 3:] *= 2.1981 * float(ang[len(ang) >> 1])
    else:
        pr = project(R, t, K, X32.astype(np.float64)).astype(F32)
        err = F32(0)
        for i in inliers:
            dx, dy = F32(uv32[i, 0] - pr[i, 0]), F32(uv32[i, 1] - pr[i, 1])
            err = F32(err + F32(dx * dx + dy * dy))
        cov *= float(np.sqrt(F32(err / F32(len(inliers)))))
    return T, cov


def count_models(models, valid, K, X, uv, thr0):
    """Counts and the winner for given hypotheses (models [H][3][4]); also the distance of the nearest error to the threshold."""
    counts, margin = [], np.inf
    for M, ok in zip(models, valid):
        if not ok:
            counts.append(0)
            continue
        e = errors(M[:, :3], M[:, 3], K, X, uv)
        counts.append(int((e <= thr0).sum()))
        margin = min(margin, float(np.abs(e.astype(np.float64) - float(thr0)).min()))
    key = [(c, -h) for h, (c, ok) in enumerate(zip(counts, valid)) if ok]
    winner = -max(key)[1] if key else -1
    return counts, winner, margin


def after_winner(R, t, K, Tir, X32, uv32, to_xyz_kept, params):
    """Steps 4 (the winner's list) to 7 from the winner's model."""
    X, uv = X32.astype(np.float64), uv32.astype(np.float64)
    thr0 = F32(params["reproj_error"])
    min_inliers = max(4, params["min_inliers"])
    out = {"T": np.zeros((4, 4)), "cov": np.eye(6), "inliers": [], "passes": [], "refit": None, "margin": np.inf}
    e, L0 = select(R, t, K, X, uv, thr0)
    out["L0"] = L0
    if len(L0) < min_inliers or params["refine_iterations"] <= 0:
        return out
    R, t = refit(R, t, K, X[L0], uv[L0])
    out["refit"] = (R, t)
    inl, R, t, passes = refine_loop(R, t, K, X, uv, L0, thr0, params["refine_sigma"], min_inliers, params["refine_iterations"])
    out["passes"] = passes
    out["model"] = (R, t)
    for _, _, thr, e, _ in passes:
        out["margin"] = min(out["margin"], float(np.abs(e.astype(np.float64) - float(thr)).min()))
    if len(inl) < min_inliers:
        return out
    out["inliers"] = inl
    out["T"], out["cov"] = finalize(R, t, K, Tir, X32, uv32, inl, to_xyz_kept)
    return out


def solve(params, K, Tir, from_xyz, to_xy, to_xyz=None):
    """The whole call on the checker's own hypotheses.  params: dict of the visfs_pnp_params fields; K = (fx, fy, cx, cy)."""
    from_xyz = np.asarray(from_xyz, dtype=F32).reshape(-1, 3)
    to_xy = np.asarray(to_xy, dtype=F32).reshape(-1, 2)
    keep = np.nonzero(np.isfinite(from_xyz).all(axis=1))[0]
    X32, uv32 = from_xyz[keep], to_xy[keep]
    kept_to = np.asarray(to_xyz, dtype=F32).reshape(-1, 3)[keep] if to_xyz is not None else None
    m = len(keep)
    min_inliers = max(4, params["min_inliers"])
    res = {"matches": keep.astype(np.int32), "m": m, "T": np.zeros((4, 4)), "cov": np.eye(6), "inliers": np.zeros(0, dtype=np.int32),
           "samples": [], "valid": [], "models": [], "diags": [], "counts": [], "winner": -1, "ties": 0, "margin": np.inf, "after": None}
    if m < min_inliers:
        return res
    X, uv = X32.astype(np.float64), uv32.astype(np.float64)
    thr0 = F32(params["reproj_error"])
    for h in range(params["iterations"]):
        s = sample(params["seed"], h, m)
        best, diag = p3p(K, X[s], uv[s])
        res["samples"].append(s); res["valid"].append(best is not None); res["diags"].append(diag)
        M = np.zeros((3, 4))
        if best is not None:
            M[:, :3], M[:, 3] = best
        res["models"].append(M)
    res["counts"], res["winner"], res["margin"] = count_models(res["models"], res["valid"], K, X, uv, thr0)
    if res["winner"] < 0:
        return res
    res["ties"] = sum(1 for c, ok in zip(res["counts"], res["valid"]) if ok and c == res["counts"][res["winner"]])
    W = res["models"][res["winner"]]
    aft = after_winner(W[:, :3], W[:, 3], K, Tir, X32, uv32, kept_to, params)
    res["after"] = aft
    res["margin"] = min(res["margin"], aft["margin"])
    res["T"], res["cov"] = aft["T"], aft["cov"]
    res["inliers"] = keep[aft["inliers"]].astype(np.int32) if len(aft["inliers"]) else np.zeros(0, dtype=np.int32)
    return res
