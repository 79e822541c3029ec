"""NumPy definition of record of the corner extraction (include/visfs_corners.h).  Shares no code with the
library: the tests compare the host twin with this byte for byte, and the device with the host twin.

goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask) with OpenCV's defaults (blockSize 3, gradientSize 3,
minimum-eigenvalue response), restated from OpenCV's published algorithm; parity with OpenCV itself is not pinned.  The one deliberate
deviation: the box sums of the derivative products are exact integers (OpenCV scales to float first and adds floats).
"""
import numpy as np

F = np.float32
K = F(1.0 / (3060.0 * 3060.0))


def reflect(i, n):
    """BORDER_REFLECT_101 of an index array."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _padded(m):
    h, w = m.shape
    return m[reflect(np.arange(-1, h + 1), h)][:, reflect(np.arange(-1, w + 1), w)]


def sobel(img):
    """(dx, dy) int64 [h][w]: unnormalised 3 x 3 Sobel, the image border reflected."""
    p = _padded(img.astype(np.int64))
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return dx, dy


def box3(m):
    """3 x 3 sums of an integer map, a neighbour outside the map taking the value at the reflected place."""
    h, w = m.shape
    p = _padded(m)
    s = np.zeros((h, w), dtype=np.int64)
    for a in range(3):
        for b in range(3):
            s += p[a:a + h, b:b + w]
    return s


def response(img):
    """float32 [h][w]: the minimum eigenvalue, one rounded float32 operation per step."""
    dx, dy = sobel(img)
    sxx, sxy, syy = box3(dx * dx), box3(dx * dy), box3(dy * dy)
    assert max(sxx.max(), syy.max(), np.abs(sxy).max()) < 2 ** 24
    a = (sxx.astype(F) * K) * F(0.5)
    b = sxy.astype(F) * K
    c = (syy.astype(F) * K) * F(0.5)
    d = a - c
    d2 = d * d
    b2 = b * b
    root = np.sqrt(d2 + b2)
    out = (a + c) - root
    assert out.dtype == F
    return out


def halfwidth(radius):
    """hw[0 .. radius] of cv::circle(..., thickness = -1)'s midpoint walk."""
    hw = np.full(radius + 1, -1, dtype=np.int32)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        m = (1 if err <= 0 else 0) - 1
        err -= minus & m
        dx += m
        minus -= m & 2
    return hw


def centre(v):
    """cv::Point(Point2f): lrintf, round half to even."""
    return int(np.rint(F(v)))


def draw_mask(width, height, discs):
    """(mask uint8 [h][w] with 255 = free, drawn uint8 [n]): Tracker::getMask's loop over (x, y, radius) in the order given."""
    mask = np.full((height, width), 255, dtype=np.uint8)
    drawn = np.zeros(len(discs), dtype=np.uint8)
    for k, (x, y, r) in enumerate(discs):
        cx, cy, r = centre(x), centre(y), int(r)
        if 0 <= cx < width and 0 <= cy < height and mask[cy, cx] != 255:
            continue
        drawn[k] = 1
        hw = halfwidth(r)
        for yy in range(max(cy - r, 0), min(cy + r, height - 1) + 1):
            half = int(hw[abs(yy - cy)])
            lo, hi = max(cx - half, 0), min(cx + half, width - 1)
            if lo <= hi:
                mask[yy, lo:hi + 1] = 0
    return mask, drawn


def good_features(img, max_corners=300, quality_level=0.01, min_distance=40.0, discs=None):
    """dict(xy float32 [n][2], eig, mask, disc_drawn, n_candidates, max_val, exhausted): exhausted says the candidate list ran out
    before max_corners was reached."""
    h, w = img.shape
    eig = response(img)
    mask, drawn = draw_mask(w, h, discs if discs is not None else [])
    free = mask != 0
    max_val = eig[free].max() if free.any() else F(0.0)
    t = F(np.float64(max_val) * np.float64(quality_level))
    thr = np.where(eig > t, eig, F(0.0))
    pad = np.full((h + 2, w + 2), -np.inf, dtype=F)
    pad[1:-1, 1:-1] = thr
    dil = pad[0:h, 0:w].copy()
    for a in range(3):
        for b in range(3):
            dil = np.maximum(dil, pad[a:a + h, b:b + w])
    ok = (thr != 0) & (thr == dil) & free
    ok[0] = ok[-1] = False
    ok[:, 0] = ok[:, -1] = False
    idx = np.flatnonzero(ok)
    val = thr.ravel()[idx]
    order = np.lexsort((-idx, -val.astype(np.float64)))           # value descending, then raster index descending
    idx = idx[order]
    xs, ys = idx % w, idx // w
    if min_distance < 1:
        keep = np.arange(min(len(idx), max_corners))
    else:
        d2 = np.float64(min_distance) * np.float64(min_distance)
        ax = np.zeros(max_corners, dtype=np.int64); ay = np.zeros(max_corners, dtype=np.int64)
        keep = []
        for k in range(len(idx)):
            n = len(keep)
            if n and (((ax[:n] - xs[k]) ** 2 + (ay[:n] - ys[k]) ** 2) < d2).any():
                continue
            ax[n], ay[n] = xs[k], ys[k]
            keep.append(k)
            if len(keep) == max_corners:
                break
        keep = np.array(keep, dtype=np.int64)
    xy = np.stack([xs[keep], ys[keep]], -1).astype(F).reshape(-1, 2)
    return dict(xy=xy, eig=eig, mask=mask, disc_drawn=drawn, n_candidates=len(idx), max_val=F(max_val),
                exhausted=len(xy) < max_corners, order_values=val[order])
