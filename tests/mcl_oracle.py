"""An independent checker of the Monte-Carlo localisation, written from the definition: a brute-force distance
field over the occupied cells, Python integers or exact NumPy integers for every integer quantity, the adjacent-pair tree sum as
written, and IEEE + - * / sqrt element by element (NumPy never fuses them).  It takes nothing from the library."""
import bisect
import math

import numpy as np

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
TWO40 = float(1 << 40)
TWO32 = float(1 << 32)
PI = float.fromhex("0x1.921fb54442d18p+1")
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
P1 = float.fromhex("0x1.921fb54400000p+0")
P2 = float.fromhex("0x1.0b4611a600000p-34")
P3 = float.fromhex("0x1.3198a2e037073p-69")

FIELD_DEFAULTS = dict(occupied_probability=0.65, max_dist=2.0, z_hit=0.5, z_rand=0.5, sigma_hit=0.2, range_max=12.0)
FILTER_DEFAULTS = dict(alpha1=0.2, alpha2=0.2, alpha3=0.2, alpha4=0.2, n_eff_ratio=1.0, resample_interval=2, max_beams=0)


# ---------------------------------------------------------------- the field
def value_cost(v):
    """The correspondence cost of grid value v in 1 .. 32767 (ProbabilityValues.h)."""
    k_min_p = 0.1
    k_max_p = 1.0 - k_min_p
    lo, hi = 1.0 - k_max_p, 1.0 - k_min_p
    k = (hi - lo) / 32766.0
    return v * k + (lo - k)


def v_occ_of(occupied_probability):
    best = 0
    for v in range(1, 32768):
        if 1.0 - value_cost(v) >= occupied_probability:
            best = v
    return best


def llround(v):
    r = math.floor(v)
    return int(r) + (1 if v - r >= 0.5 else 0)          # v >= 0 here


def field(cells, res, **kw):
    """(t uint16 [ny][nx], q int64 [T + 1], v_occ, T, R) by brute force over the occupied cells."""
    p = dict(FIELD_DEFAULTS, **kw)
    cells = np.asarray(cells, dtype=np.uint16)
    ny, nx = cells.shape
    d = p["max_dist"] / res
    R, T = int(math.floor(d)), int(math.ceil(d * d))
    v_occ = v_occ_of(p["occupied_probability"])
    v = (cells & 32767).astype(np.int64)
    oy, ox = np.nonzero((v >= 1) & (v <= v_occ))
    t = np.full((ny, nx), T, dtype=np.int64)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for k in range(0, len(ox), 64):                      # min over every occupied cell, in chunks
        dx = xx[None, :, :] - ox[k:k + 64, None, None]
        dy = yy[None, :, :] - oy[k:k + 64, None, None]
        t = np.minimum(t, (dx * dx + dy * dy).min(axis=0))
    q = []
    for i in range(T + 1):
        z = res * math.sqrt(float(i)) if i < T else p["max_dist"]
        pz = p["z_hit"] * math.exp(-(z * z) / (2.0 * (p["sigma_hit"] * p["sigma_hit"]))) + p["z_rand"] / p["range_max"]
        q.append(llround((pz * pz * pz) * TWO40))
    return t.astype(np.uint16), np.array(q, dtype=np.int64), v_occ, T, R


# ---------------------------------------------------------------- numbers
def mix64(z):
    """The splitmix64 finaliser on a uint64 array (NumPy's unsigned arithmetic wraps)."""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mix64_int(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def key_int(seed, update, particle, draw):
    h = mix64_int(seed + GOLD * (update + 1))
    h = mix64_int(h + GOLD * (particle + 1))
    return mix64_int(h + GOLD * (draw + 1))


def normals(seed, update, n, draw):
    """g of particles 0 .. n - 1 for one draw."""
    with np.errstate(over="ignore"):
        h0 = np.uint64(mix64_int(seed + GOLD * (update + 1)))
        j = np.arange(1, n + 1, dtype=np.uint64)
        h = mix64(h0 + np.uint64(GOLD) * j)
        h = mix64(h + np.uint64((GOLD * (draw + 1)) & MASK))
        s = np.zeros(n, dtype=np.int64)
        for m in range(1, 7):
            r = mix64(h + np.uint64((GOLD * m) & MASK))
            s += (r >> np.uint64(32)).astype(np.int64) + (r & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return (s - 6 * 0xFFFFFFFF).astype(np.float64) / TWO32


def round_half_away(v):
    r = np.trunc(v)
    return r + np.where(np.abs(v - r) >= 0.5, np.sign(v), 0.0)


def sincos_poly(d):
    z = d * d
    p = 1.0 / 51090942171709440000.0
    for c in (-1.0 / 121645100408832000.0, 1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0,
              1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
        p = c + z * p
    q = 1.0 / 2432902008176640000.0
    for c in (-1.0 / 6402373705728000.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0,
              1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -1.0 / 2.0):
        q = c + z * q
    return d * p, 1.0 + z * q


def sincos_any(a):
    a = np.asarray(a, dtype=np.float64)
    k = round_half_away(a * TWO_OVER_PI)
    r = ((a - k * P1) - k * P2) - k * P3
    sr, cr = sincos_poly(r)
    quad = k.astype(np.int64) & 3
    s = np.select([quad == 0, quad == 1, quad == 2], [sr, cr, -sr], -cr)
    c = np.select([quad == 0, quad == 1, quad == 2], [cr, -sr, -cr], sr)
    return s, c


def wrap(yaw):
    yaw = np.asarray(yaw, dtype=np.float64)
    return np.where(yaw > PI, yaw - TWO_PI, np.where(yaw <= -PI, yaw + TWO_PI, yaw))


def tree_sum(a):
    a = np.asarray(a, dtype=np.float64)
    n = 1
    while n < len(a):
        n *= 2
    a = np.concatenate([a, np.zeros(n - len(a))])
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return float(a[0])


# ---------------------------------------------------------------- the filter
class Filter:
    """The filter on a field (t, q, T) with limits (res, max_x, max_y)."""

    def __init__(self, t, q, T, res, max_x, max_y, n_particles, seed):
        self.t, self.q, self.T = np.asarray(t), np.asarray(q, dtype=np.int64), T
        self.res, self.max_x, self.max_y = res, max_x, max_y
        self.N, self.seed = n_particles, seed
        self.init((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))

    def init(self, mean, sigma):
        N = self.N
        g = [normals(self.seed, 0, N, d) for d in range(3)]
        self.x = mean[0] + sigma[0] * g[0]
        self.y = mean[1] + sigma[1] * g[1]
        self.yaw = wrap(float(wrap(mean[2])) + sigma[2] * g[2])
        self.w = np.full(N, 1.0 / N)
        self.Q = np.zeros(N, dtype=np.int64)
        self.ancestors = np.arange(N, dtype=np.int32)
        self.update_count = 0

    def state(self):
        return dict(x=self.x, y=self.y, yaw=self.yaw, w=self.w, Q=self.Q, ancestors=self.ancestors)

    def update(self, odom_delta, points_xyz, **kw):
        p = dict(FILTER_DEFAULTS, **kw)
        N = self.N
        u = self.update_count + 1
        dx, dy, dyaw = (float(v) for v in odom_delta)
        # the host plan
        trans = math.sqrt(dx * dx + dy * dy)
        rot1 = 0.0 if trans < 0.01 else math.atan2(dy, dx)
        rot2 = dyaw - rot1
        w2 = abs(float(wrap(rot2)))
        a1, a2, a3, a4 = p["alpha1"], p["alpha2"], p["alpha3"], p["alpha4"]
        n1, n2 = min(abs(rot1), PI - abs(rot1)), min(w2, PI - w2)
        s_r1 = math.sqrt(a1 * (n1 * n1) + a2 * (trans * trans))
        s_t = math.sqrt((a3 * (trans * trans) + a4 * (n1 * n1)) + a4 * (n2 * n2))
        s_r2 = math.sqrt(a1 * (n2 * n2) + a2 * (trans * trans))
        assert abs(dyaw) <= TWO_PI and abs(rot1 + rot2) + 6.0 * (s_r1 + s_r2) <= TWO_PI
        pts = np.asarray(points_xyz, dtype=np.float64).reshape(-1, 3)
        n = len(pts)
        step = -(-n // p["max_beams"]) if p["max_beams"] > 0 else 1
        pts = pts[::max(step, 1)]
        # 1. motion
        g0, g1, g2 = (normals(self.seed, u, N, d) for d in range(3))
        r1 = rot1 - s_r1 * g0
        th = trans - s_t * g1
        r2 = rot2 - s_r2 * g2
        s, c = sincos_any(self.yaw + r1)
        moved = th != 0.0
        x = np.where(moved, self.x + th * c, self.x)
        y = np.where(moved, self.y + th * s, self.y)
        dyw = r1 + r2
        yaw = np.where(dyw != 0.0, wrap(self.yaw + dyw), self.yaw)
        # 2. weights
        s, c = sincos_any(yaw)
        Q = np.zeros(N, dtype=np.int64)
        ny, nx = self.t.shape
        chunk = max(1, (1 << 18) // N)                     # beams per pass: [chunk][N] element by element, the integer sum has no order
        for b in range(0, len(pts), chunk):
            px, py = pts[b:b + chunk, 0][:, None], pts[b:b + chunk, 1][:, None]
            ex = x[None, :] + (c[None, :] * px - s[None, :] * py)
            ey = y[None, :] + (s[None, :] * px + c[None, :] * py)
            ix = round_half_away((self.max_y - ey) / self.res - 0.5)
            iy = round_half_away((self.max_x - ex) / self.res - 0.5)
            inside = (ix >= 0) & (iy >= 0) & (ix < nx) & (iy < ny)
            jx = np.where(inside, ix, 0).astype(np.int64)
            jy = np.where(inside, iy, 0).astype(np.int64)
            tt = np.where(inside, self.t[jy, jx].astype(np.int64), self.T)
            Q += self.q[tt].sum(axis=0)
        w = self.w * (1.0 + Q.astype(np.float64) / TWO40)
        # 3. sums
        wx, wy = w * x, w * y
        S = [tree_sum(v) for v in (w, w * w, wx, wy, w * c, w * s, wx * x, wx * y, wy * y)]
        W = S[0]
        best = int(np.argmax(w))                           # the first of equals
        res = dict(status=0, best=best, n_beams=len(pts), update=u, W=W, best_pose=[float(x[best]), float(y[best]), float(yaw[best])],
                   best_weight=float(w[best]) / W)
        mx, my, mc, ms = S[2] / W, S[3] / W, S[4] / W, S[5] / W
        res["mean"] = [mx, my, math.atan2(S[5], S[4])]
        cov = [0.0] * 9
        cov[0] = S[6] / W - mx * mx
        cov[1] = cov[3] = S[7] / W - mx * my
        cov[4] = S[8] / W - my * my
        ln = math.sqrt(mc * mc + ms * ms)
        cov[8] = (-2.0 * math.log(ln) if ln > 0.0 else math.inf) if ln < 1.0 else 0.0
        res["covariance"] = cov
        res["n_eff"] = (W * W) / S[1]
        w = w / W
        # 4. resampling
        anc = list(range(N))
        resampled = u % p["resample_interval"] == 0 and res["n_eff"] < p["n_eff_ratio"] * float(N)
        if resampled:
            k = [int(math.floor(v * TWO40)) for v in w.tolist()]
            C = [0] * N
            for j in range(1, N):
                C[j] = C[j - 1] + k[j - 1]
            K = C[-1] + k[-1]
            r0 = key_int(self.seed, u, N, 0) % K
            anc = []
            for i in range(N):
                uu = (i * K + r0) // N
                a = bisect.bisect_right(C, uu) - 1
                assert C[a] <= uu < C[a] + k[a]
                anc.append(a)
            ia = np.array(anc, dtype=np.int64)
            x, y, yaw, w = x[ia], y[ia], yaw[ia], np.full(N, 1.0 / N)
        res["resampled"] = 1 if resampled else 0
        self.x, self.y, self.yaw, self.w, self.Q = x, y, yaw, w, Q
        self.ancestors = np.array(anc, dtype=np.int32)
        self.update_count = u
        return res
