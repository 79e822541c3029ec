"""Independent NumPy statement of the pyramidal Lucas-Kanade arithmetic of include/visfs_flow.h, and the
synthetic scenes the flow tests run on.  It shares no code with the library: whole-array operations, np.int64 sums, and the scalar
tail in np.float32 written one operation per line.  This file is the definition of record of the arithmetic.

The pass restates OpenCV's published calcOpticalFlowPyrLK from memory ([opencv-upstream], unpinned: OpenCV is not available where
the tests run).  Deliberate deviations: the window sums are exact integers (OpenCV adds the same integer-valued products in
float), the step divides by D where OpenCV multiplies by 1/D, and the stopping tests are float32 throughout.
"""
import functools

import numpy as np

F = np.float32
W_BITS = 14
FLT_EPSILON = F(np.finfo(np.float32).eps)


class Params:
    def __init__(self, **kw):
        self.win_size = 21; self.max_level = 3; self.iterations = 30; self.eps = F(0.01); self.flow_back = 1
        self.min_eig_threshold = F(1e-4); self.back_gate_track = F(1.5); self.back_gate_stereo = F(0.5)
        self.min_depth = F(0.2); self.max_depth = F(10.0)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


# ------------------------------------------------------------------------------------------------ pyramid and derivative
def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img):
    h, w = img.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    k = (1, 4, 6, 4, 1)
    a = img.astype(np.int64)
    xs, ys = 2 * np.arange(dw), 2 * np.arange(dh)
    rows = sum(k[i] * a[:, reflect101(xs + i - 2, w)] for i in range(5))
    out = sum(k[j] * rows[reflect101(ys + j - 2, h), :] for j in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def scharr(img):
    """(h, w, 2) int16: unnormalised Scharr Ix, Iy, image border REFLECT_101."""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    c = lambda dy, dx: p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx]
    ix = 3 * (c(-1, 1) - c(-1, -1)) + 10 * (c(0, 1) - c(0, -1)) + 3 * (c(1, 1) - c(1, -1))
    iy = 3 * (c(1, -1) - c(-1, -1)) + 10 * (c(1, 0) - c(-1, 0)) + 3 * (c(1, 1) - c(-1, 1))
    return np.stack([ix, iy], -1).astype(np.int16)


def build_pyramid(img, max_level):
    """[(uint8 level, int16 derivative)] for levels 0 .. max_level."""
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(max_level):
        out.append(pyr_down(out[-1]))
    return [(l, scharr(l)) for l in out]


# ------------------------------------------------------------------------------------------------ one LK pass
def _weights(fx, fy, ix, iy):
    a = fx - ix.astype(F)
    b = fy - iy.astype(F)
    one = F(1.0)
    s = F(1 << W_BITS)
    iw00 = np.rint(((one - a) * (one - b)) * s).astype(np.int64)
    iw01 = np.rint((a * (one - b)) * s).astype(np.int64)
    iw10 = np.rint(((one - a) * b) * s).astype(np.int64)
    iw11 = (1 << W_BITS) - iw00 - iw01 - iw10
    return [w[:, None, None] for w in (iw00, iw01, iw10, iw11)]


def _corner(pt, win, w, h):
    """floor of the window corner, and whether it stays in [-win, cols) x [-win, rows) (decided on the floats: NaN is outside)."""
    fl = np.floor(pt)
    ok = (fl[:, 0] >= F(-win)) & (fl[:, 0] < F(w)) & (fl[:, 1] >= F(-win)) & (fl[:, 1] < F(h))
    ip = np.where(ok[:, None], fl, F(0)).astype(np.int64)
    return ip, ok


def _patch_px(img, ip, win):
    """(n, win + 1, win + 1) pixels at the corners ip, REFLECT_101 outside the level."""
    h, w = img.shape
    k = np.arange(win + 1)
    X = reflect101(ip[:, 0, None] + k, w)
    Y = reflect101(ip[:, 1, None] + k, h)
    return img[Y[:, :, None], X[:, None, :]].astype(np.int64)


def _patch_der(der, ip, win):
    """(n, win + 1, win + 1, 2) derivatives, 0 outside the level."""
    h, w = der.shape[:2]
    k = np.arange(win + 1)
    X = ip[:, 0, None] + k
    Y = ip[:, 1, None] + k
    okx = (X >= 0) & (X < w)
    oky = (Y >= 0) & (Y < h)
    v = der[np.clip(Y, 0, h - 1)[:, :, None], np.clip(X, 0, w - 1)[:, None, :]].astype(np.int64)
    return v * (oky[:, :, None] & okx[:, None, :])[..., None]


def _bilinear(p, iw, bits):
    v = p[:, :-1, :-1] * iw[0] + p[:, :-1, 1:] * iw[1] + p[:, 1:, :-1] * iw[2] + p[:, 1:, 1:] * iw[3]
    return (v + (1 << (bits - 1))) >> bits


def lk_pass(pyrI, pyrJ, pts, init, prm):
    """One calcOpticalFlowPyrLK: template pyramid pyrI, moving pyramid pyrJ, points pts (n, 2) float32, init (n, 2) float32 or None
    (OPTFLOW_USE_INITIAL_FLOW).  Returns (next (n, 2) float32, status uint8, err float32)."""
    pts = np.asarray(pts, dtype=F).reshape(-1, 2)
    n = len(pts)
    win = prm.win_size
    half = F((win - 1) * 0.5)
    status = np.ones(n, dtype=np.uint8)
    err = np.zeros(n, dtype=F)
    nxt = np.zeros((n, 2), dtype=F)
    scale_tail = F(2.0 ** -20)
    eps2 = F(prm.eps) * F(prm.eps)
    for level in range(prm.max_level, -1, -1):
        imgI, derI = pyrI[level]
        imgJ, _ = pyrJ[level]
        h, w = imgI.shape
        sc = F(2.0 ** -level)
        prev = pts * sc
        if level == prm.max_level:
            nxt = (np.asarray(init, dtype=F).reshape(-1, 2) * sc) if init is not None else prev.copy()
        else:
            nxt = nxt * F(2.0)
        prev = prev - half
        ip, ok = _corner(prev, win, w, h)
        if level == 0:
            status[~ok] = 0
            err[~ok] = F(0)
        idx = np.nonzero(ok)[0]
        if len(idx) == 0:
            continue
        iw = _weights(prev[idx, 0], prev[idx, 1], ip[idx, 0], ip[idx, 1])
        I = _bilinear(_patch_px(imgI, ip[idx], win), iw, W_BITS - 5)
        d = _patch_der(derI, ip[idx], win)
        Ix = _bilinear(d[..., 0], iw, W_BITS)
        Iy = _bilinear(d[..., 1], iw, W_BITS)
        A11 = (Ix * Ix).sum((1, 2)).astype(F) * scale_tail
        A12 = (Ix * Iy).sum((1, 2)).astype(F) * scale_tail
        A22 = (Iy * Iy).sum((1, 2)).astype(F) * scale_tail
        t0 = A11 * A22
        t1 = A12 * A12
        D = t0 - t1
        df = A11 - A22
        df2 = df * df
        q = F(4.0) * A12
        q2 = q * A12
        rad = np.sqrt(df2 + q2)
        tr = A22 + A11
        num = tr - rad
        min_eig = num / F(2 * win * win)
        err[idx] = min_eig
        bad = (min_eig < F(prm.min_eig_threshold)) | (D < FLT_EPSILON)
        if level == 0:
            status[idx[bad]] = 0
        good = ~bad
        idx, I, Ix, Iy, A11, A12, A22, D = idx[good], I[good], Ix[good], Iy[good], A11[good], A12[good], A22[good], D[good]
        # the iteration, every point of the level in lock-step
        cur = nxt[idx] - half                        # window corner of the moving patch
        out = nxt[idx].copy()
        pd = np.zeros((len(idx), 2), dtype=F)
        live = np.ones(len(idx), dtype=bool)
        for j in range(prm.iterations):
            jp, ok = _corner(cur, win, w, h)
            ok |= ~live
            if level == 0:
                status[idx[~ok]] = 0
            live &= ok
            r = np.nonzero(live)[0]
            if len(r) == 0:
                break
            iwj = _weights(cur[r, 0], cur[r, 1], jp[r, 0], jp[r, 1])
            J = _bilinear(_patch_px(imgJ, jp[r], win), iwj, W_BITS - 5)
            diff = J - I[r]
            b1 = (diff * Ix[r]).sum((1, 2)).astype(F) * scale_tail
            b2 = (diff * Iy[r]).sum((1, 2)).astype(F) * scale_tail
            u0 = A12[r] * b2
            u1 = A22[r] * b1
            dx = (u0 - u1) / D[r]
            v0 = A12[r] * b1
            v1 = A11[r] * b2
            dy = (v0 - v1) / D[r]
            delta = np.stack([dx, dy], -1)
            cur[r] = cur[r] + delta
            out[r] = cur[r] + half
            dxx = dx * dx
            dyy = dy * dy
            conv = (dxx + dyy) <= eps2
            osc = np.zeros(len(r), dtype=bool)
            if j > 0:
                osc = ~conv & (np.abs(dx + pd[r, 0]) < F(0.01)) & (np.abs(dy + pd[r, 1]) < F(0.01))
                out[r[osc]] = out[r[osc]] - delta[osc] * F(0.5)
            pd[r] = delta
            live[r[conv | osc]] = False
        nxt[idx] = out
    return nxt, status, err


def l2(a, b):
    dx = a[:, 0] - b[:, 0]
    dy = a[:, 1] - b[:, 1]
    return np.sqrt(dx * dx + dy * dy)


def lk_gated(pyrI, pyrJ, pts, guess, prm, gate, detail=False):
    """Forward pass and, when flow_back, the reverse pass started from the points, with the gate on the round trip."""
    pts = np.asarray(pts, dtype=F).reshape(-1, 2)
    to, st, err = lk_pass(pyrI, pyrJ, pts, guess, prm)
    if not prm.flow_back:
        return (to, st, err, None) if detail else (to, st, err)
    back, rst, _ = lk_pass(pyrJ, pyrI, to, pts, prm)
    dist = l2(back, pts)
    with np.errstate(invalid="ignore"):
        keep = (st != 0) & (rst != 0) & (dist <= F(gate))
    out = keep.astype(np.uint8)
    if detail:
        return to, out, err, dict(forward=st, reverse=rst, dist=dist)
    return to, out, err


# ------------------------------------------------------------------------------------------------ triangulation
class Camera:
    def __init__(self, fx=435.2, fy=435.2, cx=367.4, cy=252.2, cx_right=367.4, baseline=0.11, Tir=None):
        self.fx, self.fy, self.cx, self.cy, self.cx_right, self.baseline = F(fx), F(fy), F(cx), F(cy), F(cx_right), F(baseline)
        self.Tir = np.asarray(Tir if Tir is not None else [0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0], dtype=np.float64).reshape(12)


def triangulate(left, right, status, cam, prm):
    """generateKeyPoints3DStereo for the points with status 1; NaN triples elsewhere.  float32 as projectDisparityTo3D writes it,
    then the image -> robot transform in double (row by row, left to right) rounded to float32."""
    left = np.asarray(left, dtype=F).reshape(-1, 2)
    right = np.asarray(right, dtype=F).reshape(-1, 2)
    n = len(left)
    out = np.full((n, 3), np.nan, dtype=F)
    T = cam.Tir
    for i in range(n):
        if not status[i]:
            continue
        disp = left[i, 0] - right[i, 0]
        if not (disp != F(0)):
            continue
        if not (disp > F(0) and cam.baseline > F(0) and cam.fx > F(0)):
            continue
        c = F(0)
        if cam.cx > F(0) and cam.cx_right > F(0):
            c = cam.cx_right - cam.cx
        den = disp + c
        with np.errstate(divide="ignore", invalid="ignore"):
            W = cam.baseline / den
            ux = left[i, 0] - cam.cx
            uy = left[i, 1] - cam.cy
            x = ux * W
            y = uy * W
            z = cam.fx * W
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            continue
        if not ((prm.min_depth < F(0) or z > F(prm.min_depth)) and (prm.max_depth <= F(0) or z <= F(prm.max_depth))):
            continue
        p = np.array([x, y, z], dtype=np.float64)
        for r in range(3):
            out[i, r] = F(((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3])
    return out


class Tracker:
    """The library's object, restated: resident pyramids of the previous and current stereo pair."""

    def __init__(self, prm, width, height):
        self.prm, self.w, self.h = prm, width, height
        self.prev = None
        self.cur = None

    def push_frame(self, left, right):
        assert left.shape == right.shape == (self.h, self.w)
        self.prev = self.cur
        self.cur = (build_pyramid(left, self.prm.max_level), build_pyramid(right, self.prm.max_level))

    def track(self, from_xy, guess_xy=None, detail=False):
        return lk_gated(self.prev[0], self.cur[0], from_xy, guess_xy, self.prm, self.prm.back_gate_track, detail)

    def stereo(self, left_xy, cam):
        to, st, _ = lk_gated(self.cur[0], self.cur[1], left_xy, None, self.prm, self.prm.back_gate_stereo)
        return to, st, triangulate(left_xy, to, st, cam, self.prm)


# ------------------------------------------------------------------------------------------------ synthetic scenes
class Texture:
    """A smooth random texture: a sum of sinusoids (wavelengths 6-60 px, amplitude proportional to the wavelength) evaluated
    analytically, so a warped frame is sampled, never interpolated."""

    def __init__(self, seed, n_waves=200, lo=6.0, hi=60.0, sigma=40.0):
        rng = np.random.default_rng(seed)
        lam = np.exp(rng.uniform(np.log(lo), np.log(hi), n_waves))
        th = rng.uniform(0, 2 * np.pi, n_waves)
        self.kx = 2 * np.pi / lam * np.cos(th)
        self.ky = 2 * np.pi / lam * np.sin(th)
        self.ph = rng.uniform(0, 2 * np.pi, n_waves)
        self.amp = lam * (sigma / np.sqrt(0.5 * np.sum(lam * lam)))

    def value(self, X, Y):
        X = np.asarray(X, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        acc = np.zeros(np.broadcast(X, Y).shape)
        for k in range(len(self.kx)):
            acc += self.amp[k] * np.cos(self.kx[k] * X + self.ky[k] * Y + self.ph[k])
        return acc

    def image(self, X, Y):
        return np.clip(np.rint(128.0 + self.value(X, Y)), 0, 255).astype(np.uint8)


class Motion:
    """p -> zoom * R(rot) (p - c) + c + t: where a point of the first frame lies in the second."""

    def __init__(self, width, height, t=(9.0, -7.5), rot=0.01, zoom=1.01):
        self.c = np.array([0.5 * (width - 1), 0.5 * (height - 1)])
        cs, sn = np.cos(rot), np.sin(rot)
        self.A = zoom * np.array([[cs, -sn], [sn, cs]])
        self.t = np.asarray(t, dtype=np.float64)

    def forward(self, p):
        p = np.asarray(p, dtype=np.float64)
        return (p - self.c) @ self.A.T + self.c + self.t

    def inverse(self, q):
        q = np.asarray(q, dtype=np.float64)
        return (q - self.c - self.t) @ np.linalg.inv(self.A).T + self.c


def grid(width, height):
    return np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def motion_pair(width=752, height=480, seed=1, t=(9.0, -7.5), rot=0.01, zoom=1.01):
    """(first frame, second frame, Motion): second(q) = first(inverse(q))."""
    tex = Texture(seed)
    X, Y = grid(width, height)
    m = Motion(width, height, t, rot, zoom)
    p = m.inverse(np.stack([X, Y], -1))
    return tex.image(X, Y), tex.image(p[..., 0], p[..., 1]), m


class Disparity:
    """A disparity field stated over the right image: the right pixel (xr, y) shows the left pixel (xr + d(xr, y), y).
    kind 'plane' (fronto-parallel, depth z0), 'slant' (depth z0 at the left edge to z1 at the right edge) or 'step'
    (depth z0 left of the right-image column xs, the nearer z1 from it on: the left columns between are occluded)."""

    def __init__(self, kind, width, fx=435.2, baseline=0.11, z0=5.0, z1=3.5, xs=None):
        self.kind, self.w = kind, width
        self.fb = float(F(fx)) * float(F(baseline))
        self.d0, self.d1 = self.fb / z0, self.fb / z1
        self.xs = xs if xs is not None else width // 2
        assert kind in ("plane", "slant", "step") and (kind != "step" or self.d1 > self.d0)
        self.g = (self.d1 - self.d0) / (width - 1)                  # slant: d = d0 + g * xr (disparity, not depth, is linear on a plane)

    def left_of_right(self, xr):
        xr = np.asarray(xr, dtype=np.float64)
        if self.kind == "plane":
            return xr + self.d0
        if self.kind == "slant":
            return xr + self.d0 + self.g * xr
        return np.where(xr < self.xs, xr + self.d0, xr + self.d1)

    def right_of_left(self, xl):
        """True right x of the left points xl, their disparity, and whether they are seen by the right camera."""
        xl = np.asarray(xl, dtype=np.float64)
        if self.kind == "plane":
            xr = xl - self.d0
        elif self.kind == "slant":
            xr = (xl - self.d0) / (1.0 + self.g)
        else:
            xr = np.where(xl < self.xs + self.d0, xl - self.d0, xl - self.d1)
        seen = np.ones(xl.shape, dtype=bool)
        if self.kind == "step":
            seen = (xl < self.xs + self.d0) | (xl >= self.xs + self.d1)
        return xr, xl - xr, seen

    def window_clear(self, xl, half=11.0):
        """Whether the window around the left points xl (and around their right images) stays on one side of the depth step."""
        if self.kind != "step":
            return np.ones(np.shape(xl), dtype=bool)
        xl = np.asarray(xl, dtype=np.float64)
        return (xl + half < self.xs + self.d0) | (xl - half >= self.xs + self.d1 + 1.0)


@functools.lru_cache(maxsize=None)
def stereo_pair(kind, width=752, height=480, seed=1, **kw):
    """(left, right, Disparity) of one textured surface."""
    tex = Texture(seed)
    X, Y = grid(width, height)
    d = Disparity(kind, width, **dict(kw))
    return tex.image(X, Y), tex.image(d.left_of_right(X), Y), d


def random_points(n, width, height, margin, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, width - 1 - margin, n), rng.uniform(margin, height - 1 - margin, n)], -1).astype(F)
