"""An independent checker of the laser pretreatment with its voxel filters (include/visfs_scan_filter.h),
written from the definition in plain Python / NumPy: IEEE doubles combined in the stated order, voxels as a dict keyed by integer
tuples.  It shares no code and no hashing scheme with the library."""
import numpy as np

OK, ERR_UNSUPPORTED = 0, 7
DROPPED, RETURN, MISS = 0, 1, 2
MAX_VOXEL = (1 << 20) - 1

DEFAULTS = dict(num_subdivisions=1, min_range=0.1, max_range=30.0, missing_ray_length=5.0, voxel_size=0.025,
                adaptive_max_length=0.5, adaptive_min_num_points=200, adaptive_max_range=50.0)


def round_away(v):
    """round(v) with ties away from zero, exactly (v: float64 array)."""
    a = np.abs(v)
    f = np.floor(a)
    f = f + ((a - f) >= 0.5)
    return np.copysign(f, v)


def transform(T, p):
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def voxels(p, length):
    """(integer triples as a list of tuples, all in range)."""
    with np.errstate(all="ignore"):
        r = round_away(np.asarray(p, dtype=np.float64).reshape(-1, 3) / np.float64(length))
    ok = bool(np.all(np.abs(r) <= MAX_VOXEL)) if len(r) else True          # a NaN compares false
    if not ok:
        return None, False
    return [tuple(int(c) for c in row) for row in r.astype(np.int64)], True


def voxel_filter(p, length):
    """Indices of the points of p (in order) whose voxel no earlier point has, or None when a voxel index is out of range."""
    vox, ok = voxels(p, length)
    if not ok:
        return None
    seen, keep = {}, []
    for i, v in enumerate(vox):
        if v not in seen:
            seen[v] = i
            keep.append(i)
    return keep


def pretreat(points, T, origin, prm):
    """Per input point: class, subdivision, the point it becomes; and the transformed origin."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n, S = len(pts), prm["num_subdivisions"]
    o = transform(T, origin)[0]
    q = transform(T, pts)
    d = q - o
    with np.errstate(all="ignore"):
        rng = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        cls = np.where(~(rng >= prm["min_range"]), DROPPED, np.where(rng <= prm["max_range"], RETURN, MISS)).astype(np.uint8)
        f = np.float64(prm["missing_ray_length"]) / rng
        mis = o + f[:, None] * d
    out = np.where((cls == MISS)[:, None], mis, q)
    sub = np.zeros(n, dtype=np.uint8)
    for s in range(S):
        sub[n * s // S: n * (s + 1) // S] = s
    return cls, sub, out, o


def adaptive(cloud, prm):
    """(status ok, match cloud, length, trace) of Cartographer 1.0's AdaptivelyVoxelFiltered in double."""
    L, M = np.float64(prm["adaptive_max_length"]), prm["adaptive_min_num_points"]
    trace = []

    class OutOfRange(Exception):
        pass

    def filt(length):
        keep = voxel_filter(cloud, length)
        if keep is None:
            raise OutOfRange()
        trace.append((float(length), len(keep)))
        return keep

    try:
        if not L > 0.0 or len(cloud) <= M:
            return True, cloud, 0.0, trace
        result, length = filt(L), L
        if len(result) >= M:
            return True, cloud[result], float(length), trace
        high = L
        while high > np.float64(1e-2) * L:
            low = high / np.float64(2.0)
            result, length = filt(low), low
            if len(result) >= M:
                while (high - low) / low > np.float64(1e-1):
                    mid = (low + high) / np.float64(2.0)
                    cand = filt(mid)
                    if len(cand) >= M:
                        low, result, length = mid, cand, mid
                    else:
                        high = mid
                return True, cloud[result], float(length), trace
            high = high / np.float64(2.0)
        return True, cloud[result], float(length), trace
    except OutOfRange:
        return False, None, 0.0, []


def process(points, T, origin, params):
    """One scan.  dict(record, range_data [(origin, returns, misses)], match, cls, sub, kept, trace)."""
    prm = dict(DEFAULTS, **params)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n, S = len(pts), prm["num_subdivisions"]
    cls, sub, out, o = pretreat(pts, T, origin, prm)
    bad = dict(record=dict(status=ERR_UNSUPPORTED, n_range_data=0, n_returns=0, n_misses=0, n_in_range=0, n_match=0, passes=0, match_length=0.0),
               range_data=[], match=np.zeros((0, 3)), cls=np.zeros(n, np.uint8), sub=np.zeros(n, np.uint8), kept=np.zeros(n, np.uint8), trace=[])
    kept = np.zeros(n, dtype=np.uint8)
    range_data = []
    for s in range(S):
        a, b = n * s // S, n * (s + 1) // S
        if a == b:
            continue
        lists = []
        for c in (RETURN, MISS):
            idx = np.arange(a, b)[cls[a:b] == c]
            if prm["voxel_size"] > 0.0:
                keep = voxel_filter(out[idx], prm["voxel_size"])
                if keep is None:
                    return bad
                idx = idx[keep]
            kept[idx] = 1
            lists.append(out[idx].reshape(-1, 3))
        range_data.append(([float(v) for v in o], lists[0], lists[1]))
    returns = np.concatenate([r for _, r, _ in range_data], axis=0) if range_data else np.zeros((0, 3))
    with np.errstate(all="ignore"):
        norm = np.sqrt((returns[:, 0] * returns[:, 0] + returns[:, 1] * returns[:, 1]) + returns[:, 2] * returns[:, 2])
    cloud = returns[norm <= prm["adaptive_max_range"]]
    ok, match, length, trace = adaptive(cloud, prm)
    if not ok:
        return bad
    rec = dict(status=OK, n_range_data=len(range_data), n_returns=len(returns), n_misses=sum(len(m) for _, _, m in range_data),
               n_in_range=len(cloud), n_match=len(match), passes=len(trace), match_length=length)
    return dict(record=rec, range_data=range_data, match=match, cls=cls, sub=sub, kept=kept, trace=trace)
