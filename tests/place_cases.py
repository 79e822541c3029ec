"""Inputs the place-recognition tests share (host twin against the NumPy checker, device against host twin).  Everything is generated;
nothing is read from disk.  The checker's results are computed once, cached and never written to."""
import functools

import numpy as np

import flow_oracle as fo
import place_oracle as po

F = np.float32
FLOW = dict(max_level=1)     # the flow objects under the tests: 160 x 120 is too small for the default four pyramid levels

# ------------------------------------------------------------------------------------------------ describe
DESCRIBE_SIZES = [(160, 120), (161, 121)]
DESCRIBE_COUNTS = [0, 1, 63, 64, 65, 511, 512]
CONSTANT_AT = (40, 40)          # centre of a 31 x 31 patch of one grey value
SYMMETRIC_AT = (100, 60)        # centre of a patch equal to its own point reflection: both moments vanish


@functools.lru_cache(maxsize=None)
def describe_image(w, h):
    X, Y = fo.grid(w, h)
    img = fo.Texture(5).image(X, Y).copy()
    cx, cy = CONSTANT_AT
    img[cy - 15:cy + 16, cx - 15:cx + 16] = 77
    cx, cy = SYMMETRIC_AT
    p = img[cy - 15:cy + 16, cx - 15:cx + 16].astype(np.int32)
    img[cy - 15:cy + 16, cx - 15:cx + 16] = ((p + p[::-1, ::-1]) // 2).astype(np.uint8)
    img.setflags(write=False)
    return img


def special_points(w, h):
    """Valid and invalid one pixel apart at every edge, the half-even rule, what is not finite, and the two planted patches."""
    mx, my = w // 2, h // 2
    pts = [CONSTANT_AT, SYMMETRIC_AT]
    for x in (14, 15, w - 16, w - 15):
        pts.append((x, my))
        for y in (14, 15, h - 16, h - 15):
            pts.append((x, y))
    for y in (14, 15, h - 16, h - 15):
        pts.append((mx, y))
    # x.5: 14.5 -> 14 (out), 15.5 -> 16 (in), w - 15.5 -> w - 16 (in) for an even w and w - 15 (out) for an odd one; likewise in y
    pts += [(14.5, my), (15.5, my), (w - 15.5, my), (w - 16.5, my), (mx, 14.5), (mx, 15.5), (mx, h - 15.5), (mx, h - 16.5), (mx + 0.5, my + 0.5),
            (mx + 1.5, my + 1.5), (14.49, my), (14.51, my)]
    pts += [(np.nan, my), (mx, np.nan), (np.inf, my), (mx, -np.inf), (-np.inf, np.inf), (1e9, my), (mx, -1e9), (-3.0, -3.0), (3e38, 3e38)]
    return np.array(pts, dtype=F)


@functools.lru_cache(maxsize=None)
def describe_points(w, h, n):
    sp = special_points(w, h)
    rng = np.random.default_rng(100 + w)
    rest = np.stack([rng.uniform(8, w - 9, 512), rng.uniform(8, h - 9, 512)], -1).astype(F)       # some of them inside the margin
    rest[::7] = np.rint(rest[::7]) + F(0.5)
    pts = np.concatenate([sp, rest])[:n].copy()
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def describe_checked(w, h, n):
    out = po.describe(describe_image(w, h), describe_points(w, h, n))
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ query: descriptors made to order
def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(rng, desc, bits):
    """A copy with `bits` distinct bits of every row flipped."""
    out = desc.copy()
    for r in range(len(out)):
        for b in rng.choice(256, bits, replace=False):
            out[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _slot(rng, desc, valid=None, key=0):
    n = len(desc)
    return dict(desc=desc, valid=np.ones(n, dtype=np.uint8) if valid is None else valid,
                ids=rng.integers(0, 1 << 30, n).astype(np.int32), xyz=rng.normal(0, 3, (n, 3)).astype(F), key=key)


def _qset(rng, desc, valid=None):
    n = len(desc)
    return dict(desc=desc, valid=np.ones(n, dtype=np.uint8) if valid is None else valid, xy=rng.uniform(20, 300, (n, 2)).astype(F))


def _many_slots(n_slots):
    """40 queries (three of them invalid) against n_slots slots of 12 entries.  Every fifth slot holds near copies of queries 0-5
    (count 6 each: with 63 slots or more that is more than eight equal counts), the last slot near copies of queries 10-19, and a
    slot in the middle, if there is one, near copies of queries 20-29 with two invalid entries among them (count 7)."""
    rng = np.random.default_rng(1000 + n_slots)
    q = _rand_desc(rng, 40)
    qv = np.ones(40, dtype=np.uint8); qv[[7, 23, 33]] = 0
    q[qv == 0] = 0
    slots = []
    for s in range(n_slots):
        d = _rand_desc(rng, 12)
        v = np.ones(12, dtype=np.uint8)
        if s == n_slots - 1:
            d[:10] = _flip(rng, q[10:20], 9)
        elif n_slots > 2 and s == n_slots // 2:
            d[2:12] = _flip(rng, q[20:30], 5)
            v[[4, 11]] = 0
            d[v == 0] = 0
        elif s % 5 == 0:
            d[3:9] = _flip(rng, q[0:6], 12)
        slots.append(_slot(rng, d, v, key=(1 << 40) + 7 * s))
    variants = [dict(min_matches=3), dict(min_matches=3, cross_check=0), dict(min_matches=7), dict(min_matches=0, max_distance=256)]
    if n_slots > 2:
        variants += [dict(min_matches=3, first_slot=1, last_slot=n_slots - 1),        # leaves out the best slot
                     dict(min_matches=3, first_slot=n_slots // 2, last_slot=n_slots // 2 + 1), dict(first_slot=2, last_slot=2)]
    return dict(qset=_qset(rng, q, qv), slots=slots, variants=variants)


def _entry_counts():
    """512 queries against slots of 0, 1 and 512 entries (the last a shuffled near copy of the queries, some entries invalid)."""
    rng = np.random.default_rng(77)
    q = _rand_desc(rng, 512)
    perm = rng.permutation(512)
    full = _flip(rng, q[perm], 10)
    fv = np.ones(512, dtype=np.uint8); fv[rng.choice(512, 30, replace=False)] = 0
    full[fv == 0] = 0
    one = _flip(rng, q[5:6], 3)
    slots = [_slot(rng, _rand_desc(rng, 0), key=-1), _slot(rng, one, key=11), _slot(rng, full, fv, key=12), _slot(rng, _rand_desc(rng, 512), key=13)]
    return dict(qset=_qset(rng, q), slots=slots,
                variants=[dict(min_matches=1), dict(min_matches=1, cross_check=0), dict(min_matches=1, max_distance=9), dict(min_matches=1, max_distance=10)])


def _no_valid_query():
    rng = np.random.default_rng(78)
    q = np.zeros((20, 32), dtype=np.uint8)
    return dict(qset=_qset(rng, q, np.zeros(20, dtype=np.uint8)), slots=[_slot(rng, _rand_desc(rng, 30)), _slot(rng, np.zeros((4, 32), dtype=np.uint8))],
                variants=[dict(min_matches=0), dict(min_matches=1)])


def _empty_set():
    rng = np.random.default_rng(79)
    return dict(qset=_qset(rng, _rand_desc(rng, 0)), slots=[_slot(rng, _rand_desc(rng, 30))], variants=[dict(min_matches=0)])


def _duplicates():
    """Every entry twice: d1 = d2, nothing is accepted, not even at distance 0 (0 < 0 is false)."""
    rng = np.random.default_rng(80)
    q = _rand_desc(rng, 16)
    near = _flip(rng, q, 4)
    exact = q.copy()
    return dict(qset=_qset(rng, q), slots=[_slot(rng, np.concatenate([near, near])), _slot(rng, np.concatenate([exact, exact])), _slot(rng, near)],
                variants=[dict(min_matches=1), dict(min_matches=1, ratio_num=1, ratio_den=1), dict(min_matches=1, ratio_num=1024, ratio_den=1)])


def _equal_queries():
    """Queries 2 and 9 carry the same descriptor: both are nearest to entry 0, the lower wins the cross-check; without it both pass."""
    rng = np.random.default_rng(81)
    q = _rand_desc(rng, 12)
    q[9] = q[2]
    e = _rand_desc(rng, 6)
    e[0] = _flip(rng, q[2:3], 6)[0]
    e[3] = _flip(rng, q[4:5], 2)[0]
    return dict(qset=_qset(rng, q), slots=[_slot(rng, e, key=5)], variants=[dict(min_matches=1), dict(min_matches=1, cross_check=0)])


def _distance_bounds():
    """Exact copies (distance 0) and far entries: max_distance 0 keeps the exact ones only, 256 with an open ratio takes every row."""
    rng = np.random.default_rng(82)
    q = _rand_desc(rng, 24)
    e = _rand_desc(rng, 24)
    e[:8] = q[:8]
    e[8:12] = _flip(rng, q[8:12], 1)
    return dict(qset=_qset(rng, q), slots=[_slot(rng, e)],
                variants=[dict(min_matches=1, max_distance=0), dict(min_matches=1, max_distance=1), dict(min_matches=1, max_distance=256),
                          dict(min_matches=1, max_distance=256, ratio_num=1024, ratio_den=1, cross_check=0)])


QUERY_CASES = {
    "slots_1": functools.partial(_many_slots, 1), "slots_2": functools.partial(_many_slots, 2), "slots_63": functools.partial(_many_slots, 63),
    "slots_64": functools.partial(_many_slots, 64), "slots_65": functools.partial(_many_slots, 65), "slots_1024": functools.partial(_many_slots, 1024),
    "entries_0_1_512": _entry_counts, "no_valid_query": _no_valid_query, "empty_set": _empty_set, "duplicates": _duplicates,
    "equal_queries": _equal_queries, "distance_bounds": _distance_bounds,
}


@functools.lru_cache(maxsize=None)
def query_case(name):
    return QUERY_CASES[name]()


@functools.lru_cache(maxsize=None)
def query_checked(name):
    """The checker's result block of every variant of a case, as bytes."""
    case = query_case(name)
    return tuple(po.query(case["qset"], case["slots"], **v).tobytes() for v in case["variants"])


# ------------------------------------------------------------------------------------------------ descriptor behaviour and places
SCENE_W, SCENE_H = 320, 240
VIEWS = [dict(t=(3.0, -2.0), rot=0.0, zoom=1.0), dict(t=(4.0, 3.0), rot=0.1, zoom=1.02), dict(t=(-5.0, 2.0), rot=0.5, zoom=1.05),
         dict(t=(2.0, -6.0), rot=1.3, zoom=0.97), dict(t=(-3.0, -3.0), rot=3.0, zoom=1.04)]
PLACE_SEEDS = list(range(20, 28))
PLACE_QUERIES = [(3, dict(t=(6.0, -4.0), rot=0.7, zoom=1.03)), (6, dict(t=(6.0, -4.0), rot=2.5, zoom=1.03))]


@functools.lru_cache(maxsize=None)
def scene_points():
    p = fo.random_points(200, SCENE_W, SCENE_H, 40, 7)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def scene(seed):
    X, Y = fo.grid(SCENE_W, SCENE_H)
    img = fo.Texture(seed).image(X, Y)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def moved_scene(seed, t, rot, zoom):
    """(the scene seen after the motion, where scene_points() lie in it)"""
    X, Y = fo.grid(SCENE_W, SCENE_H)
    m = fo.Motion(SCENE_W, SCENE_H, t, rot, zoom)
    p = m.inverse(np.stack([X, Y], -1))
    img = fo.Texture(seed).image(p[..., 0], p[..., 1])
    pts = m.forward(scene_points()).astype(F)
    img.setflags(write=False); pts.setflags(write=False)
    return img, pts


def as_slot(desc, key, n=None):
    """A described frame as a slot of the checker: word ids 1000 + i, 3-D points made from the index."""
    n = len(desc["desc"]) if n is None else n
    ids = (1000 + np.arange(n)).astype(np.int32)
    xyz = np.stack([np.arange(n) * 0.01, np.arange(n) * -0.02 + 1.0, np.full(n, 2.0)], -1).astype(F)
    return dict(desc=desc["desc"], valid=desc["valid"], ids=ids, xyz=xyz, key=key)
