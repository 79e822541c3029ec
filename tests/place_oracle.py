"""An independent NumPy checker of visual place recognition (include/visfs_place.h): the pattern, the
descriptor with its bin and valid flag, and the whole query result, written from the definition and sharing nothing with the
library.  Distances come from np.unpackbits, ranks from plain sorts, the cross-check from a Python loop."""
import numpy as np

MAX_POINTS, MAX_KEYFRAMES, MAX_CANDIDATES, NO_SECOND = 512, 1024, 8, 257
_M64 = (1 << 64) - 1

# rint(16384 cos(2 pi k / 32)) and rint(16384 sin(2 pi k / 32)), written out
COS = [16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069,
       -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069]
SIN = [0, 3196, 6270, 9102, 11585, 13623, 15137, 16069, 16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196,
       0, -3196, -6270, -9102, -11585, -13623, -15137, -16069, -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196]

ROW_DTYPE = np.dtype([("query_index", "<i4"), ("db_index", "<i4"), ("distance", "<i4"), ("id", "<i4"), ("from_xyz", "<f4", 3),
                      ("to_xy", "<f4", 2)])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_slots", "<i4"), ("n_candidates", "<i4"), ("first_slot", "<i4"),
                         ("candidate", np.dtype([("slot", "<i4"), ("count", "<i4"), ("key", "<i8")]), MAX_CANDIDATES),
                         ("count", "<i4", MAX_KEYFRAMES), ("row", ROW_DTYPE, (MAX_CANDIDATES, MAX_POINTS))])

DEFAULTS = dict(first_slot=0, last_slot=1024, max_distance=64, ratio_num=4, ratio_den=5, min_matches=40, cross_check=1)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def base_points():
    """The first 512 kept points of the counter hash."""
    pts, c = [], 0
    while len(pts) < 512:
        h = mix64((0x9E3779B97F4A7C15 * (c + 1)) & _M64)
        x, y = (h & 31) - 16, ((h >> 8) & 31) - 16
        if x * x + y * y <= 169:
            pts.append((x, y))
        c += 1
    return pts


def pattern():
    """int8 [32][512][2]: the points rotated into every bin."""
    base = base_points()
    out = np.zeros((32, 512, 2), dtype=np.int8)
    for k in range(32):
        for p, (x, y) in enumerate(base):
            out[k, p, 0] = (x * COS[k] - y * SIN[k] + 8192) >> 14      # Python's >> on a negative int is the arithmetic shift
            out[k, p, 1] = (x * SIN[k] + y * COS[k] + 8192) >> 14
    return out


_PATTERN = None
_DY, _DX = np.mgrid[-15:16, -15:16]
_DISC = (_DX * _DX + _DY * _DY <= 225)


def centre(x, y, w, h):
    """(cx, cy) or None.  np.rint rounds half to even, as lrintf does."""
    x, y = np.float32(x), np.float32(y)
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    cx, cy = int(np.rint(np.float64(x))), int(np.rint(np.float64(y)))
    if not (15 <= cx <= w - 16 and 15 <= cy <= h - 16):
        return None
    return cx, cy


def moments(img, cx, cy):
    patch = img[cy - 15:cy + 16, cx - 15:cx + 16].astype(np.int64)
    return int((_DX * patch)[_DISC].sum()), int((_DY * patch)[_DISC].sum())


def describe(img, xy):
    """dict(desc uint8 [n][32], valid uint8 [n], bin uint8 [n]) of the key-points xy on the uint8 image."""
    global _PATTERN
    if _PATTERN is None:
        _PATTERN = pattern().astype(np.int64)
    h, w = img.shape
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    n = len(xy)
    desc = np.zeros((n, 32), dtype=np.uint8); valid = np.zeros(n, dtype=np.uint8); bins = np.zeros(n, dtype=np.uint8)
    # B(u, v): the sum of the 5 x 5 pixels about (u, v), from an integral image; defined 2 pixels inside the border
    ii = np.zeros((h + 1, w + 1), dtype=np.int64)
    ii[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    box = np.zeros((h, w), dtype=np.int64)
    box[2:h - 2, 2:w - 2] = ii[5:, 5:] - ii[:-5, 5:] - ii[5:, :-5] + ii[:-5, :-5]
    cos, sin = np.array(COS, dtype=np.int64), np.array(SIN, dtype=np.int64)
    for i in range(n):
        c = centre(xy[i, 0], xy[i, 1], w, h)
        if c is None:
            continue
        cx, cy = c
        m10, m01 = moments(img, cx, cy)
        k = int(np.argmax(m10 * cos + m01 * sin))          # the first of equals
        pts = _PATTERN[k]
        a, b = pts[0::2], pts[1::2]
        bits = box[cy + a[:, 1], cx + a[:, 0]] < box[cy + b[:, 1], cx + b[:, 0]]
        desc[i] = np.packbits(bits, bitorder="little")
        valid[i] = 1; bins[i] = k
    return dict(desc=desc, valid=valid, bin=bins)


def distances(a, b):
    """Hamming distances int64 [len(a)][len(b)] of uint8 [.][32] descriptors."""
    ba = np.unpackbits(np.asarray(a, dtype=np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    bb = np.unpackbits(np.asarray(b, dtype=np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return np.rint(ba @ (1 - bb).T + (1 - ba) @ bb.T).astype(np.int64)      # exact: at most 256


def match_slot(qdesc, qvalid, edesc, evalid, prm):
    """The accepted matches of one slot: a list of (i, j1, d1), ascending i."""
    vq, ve = np.flatnonzero(qvalid), np.flatnonzero(evalid)
    if len(vq) == 0 or len(ve) == 0:
        return []
    D = distances(qdesc[vq], edesc[ve])
    keys = np.sort(D * 1024 + ve[None, :], axis=1)
    out = []
    for r, i in enumerate(vq):
        j1, d1 = int(keys[r, 0] & 1023), int(keys[r, 0] >> 10)
        d2 = int(keys[r, 1] >> 10) if len(ve) > 1 else NO_SECOND
        if d1 > prm["max_distance"] or not (d1 * prm["ratio_den"] < d2 * prm["ratio_num"]):
            continue
        if prm["cross_check"]:
            col = D[:, int(np.searchsorted(ve, j1))]
            if min((int(col[rr]) * 1024 + int(ii)) for rr, ii in enumerate(vq)) != d1 * 1024 + int(i):
                continue
        out.append((int(i), j1, d1))
    return out


def query(qset, slots, **params):
    """qset: dict(xy, desc, valid); slots: a list of dict(desc, valid, ids, xyz, key) -> a RESULT_DTYPE scalar array, every byte of
    the result block of the library."""
    prm = dict(DEFAULTS); prm.update(params)
    first = min(prm["first_slot"], len(slots))
    n_slots = min(prm["last_slot"], len(slots)) - first
    R = np.zeros((), dtype=RESULT_DTYPE)
    R["n_slots"], R["first_slot"] = n_slots, first
    matches = []
    for k in range(n_slots):
        s = slots[first + k]
        m = match_slot(np.asarray(qset["desc"]), np.asarray(qset["valid"]), np.asarray(s["desc"]), np.asarray(s["valid"]), prm)
        matches.append(m)
        R["count"][k] = len(m)
    order = sorted((k for k in range(n_slots) if len(matches[k]) >= prm["min_matches"]), key=lambda k: (-len(matches[k]), k))
    order = order[:MAX_CANDIDATES]
    R["n_candidates"] = len(order)
    xy = np.asarray(qset["xy"], dtype=np.float32).reshape(-1, 2)
    for c, k in enumerate(order):
        s = slots[first + k]
        R["candidate"][c] = (first + k, len(matches[k]), s["key"])
        for r, (i, j1, d1) in enumerate(matches[k]):
            R["row"][c, r] = (i, j1, d1, s["ids"][j1], np.asarray(s["xyz"], dtype=np.float32)[j1], xy[i])
    return R
