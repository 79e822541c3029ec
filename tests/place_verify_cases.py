"""Inputs the verified-place-query tests share (host twin against the checker and against the staged calls, device against host twin).
Everything is generated; nothing is read from disk.

A case: a key-frame store whose slots carry the 3-D words of a pnp_cases scene (the bench camera, 752 x 480, 0.3 px of pixel noise)
with random 256-bit descriptors, and a query set whose key-points are the words' pixels after the scene's motion, in shuffled order,
with the descriptors of their words at a few flipped bits.  So the place matcher pairs them, the PnP stage finds the motion and the
guided stage finds the pairs again by projection.  dict(qset, slots, query_xyz, variants); a variant: dict(place=, pnp=, verify=,
xyz=) of place parameters, visfs_pnp_params fields, guided fields and whether query_xyz is passed."""
import functools

import numpy as np

import flow_oracle as fo
import place_cases as pc
import pnp_cases as pnc
from visfs_amd import flow, place, pnp
from visfs_amd import place_verify as pv

F = np.float32
K, TIR = pnc.K, pnc.TIR


def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(rng, desc, bits):
    out = desc.copy()
    for r in range(len(out)):
        for b in rng.choice(256, bits, replace=False):
            out[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def pnp_model(truth):
    """The camera-frame model (4 x 4) of a scene: x_cam = P x_before, from T_out = (Tir pnp)^-1."""
    Ti = np.eye(4); Ti[:3] = np.array(TIR).reshape(3, 4)
    return np.linalg.inv(Ti) @ np.linalg.inv(truth)


def _base(n, seed, outliers=0.0, flips=6):
    """(scene, slot, qset, query_xyz, perm): query i is word perm[i]."""
    s = pnc.scene(n, outliers, seed)
    rng = np.random.default_rng(5000 + seed)
    edesc = _rand_desc(rng, n)
    perm = rng.permutation(n)
    slot = dict(desc=edesc, valid=np.ones(n, dtype=np.uint8), ids=(2000 + np.arange(n)).astype(np.int32), xyz=s["from_xyz"].copy(), key=seed)
    qset = dict(desc=_flip(rng, edesc[perm], flips), valid=np.ones(n, dtype=np.uint8), xy=s["to_xy"][perm].copy())
    return s, slot, qset, s["to_xyz"][perm].copy(), perm, rng


base = _base                                     # for tools/place_verify_timing.py


def _partial(slot, rng, n_match):
    """A copy of the slot in which only the first n_match entries are the scene's: the others get other descriptors and points."""
    out = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in slot.items()}
    n = len(out["desc"])
    out["desc"][n_match:] = _rand_desc(rng, n - n_match)
    out["xyz"][n_match:] = rng.normal(0, 3, (n - n_match, 3)).astype(F)
    out["key"] = 100 + n_match
    return out


V_DEFAULT = dict(place=dict(min_matches=1), pnp={}, verify={}, xyz=False)


def _v(**kw):
    out = dict(V_DEFAULT)
    out.update(kw)
    return out


def _kept_rows():
    """Five slots with 65, 64, 63, 12 and 11 matching entries of one scene (12 is min_inliers): five candidates in that order."""
    s, slot, qset, qxyz, perm, rng = _base(65, 3)
    slots = [_partial(slot, rng, n) for n in (11, 63, 65, 12, 64)]
    return dict(qset=qset, slots=slots, query_xyz=qxyz, truth=s["truth"], variants=[_v(), _v(xyz=True), _v(verify=dict(guided=0))])


def _rows_512():
    s, slot, qset, qxyz, perm, rng = _base(512, 4, outliers=0.1)
    return dict(qset=qset, slots=[slot], query_xyz=qxyz, truth=s["truth"], variants=[_v(), _v(xyz=True)])


def _nan_points():
    """80 entries, nine of them with a point that is not finite: 80 rows, 71 kept, a match index that is not the identity."""
    s, slot, qset, qxyz, perm, rng = _base(80, 41, outliers=0.2)
    bad = rng.permutation(80)[:9]
    slot["xyz"][bad[:3], 0] = np.nan
    slot["xyz"][bad[3:6], 1] = np.inf
    slot["xyz"][bad[6:], 2] = -np.inf
    return dict(qset=qset, slots=[slot], query_xyz=qxyz, truth=s["truth"], bad=bad, variants=[_v(), _v(xyz=True)])


def _ten_equal():
    """Ten slots of the same 30 entries: more than eight equal counts, eight candidates by slot; no candidate; one candidate."""
    s, slot, qset, qxyz, perm, rng = _base(30, 7)
    slots = []
    for k in range(10):
        c = {k2: (v.copy() if hasattr(v, "copy") else v) for k2, v in slot.items()}
        c["key"] = 50 + k
        slots.append(c)
    return dict(qset=qset, slots=slots, query_xyz=qxyz, truth=s["truth"],
                variants=[_v(), _v(place=dict(min_matches=31)), _v(place=dict(min_matches=1, first_slot=3, last_slot=4), xyz=True)])


def _collinear():
    """Every word on one line: no sample is valid, stage 1 leaves no pose and stage 2 does not run."""
    s, slot, qset, qxyz, perm, rng = _base(40, 9)
    a = np.linspace(1.0, 6.0, 40)
    slot["xyz"] = np.stack([a, 0.2 * a - 0.1, 0.1 * a + 0.3], -1).astype(F)
    return dict(qset=qset, slots=[slot], query_xyz=qxyz, truth=s["truth"], variants=[_v(), _v(xyz=True)])


def _geometry():
    """60 words and what the guided stage has to tell apart.
      - entries 60-62: words 0-2 mirrored through the camera centre, with their descriptors: the same pixel, a negative depth;
      - entry 63: a copy of word 5 (point and descriptor): two entries project onto one query at equal D, the lower j is kept;
      - query 60: a copy of the query of word 8, 1.5 px to the right: two queries at equal D in one window, the lower i is picked;
      - words 10-19: descriptors in pairs of equal ones (10 = 11, ...): the ratio test drops their queries, the window tells them apart.
    Variants: the defaults, without the guided stage, radius 0, a radius of 0.5 px inside the pixel noise, max_distance 0 (no guided row:
    stage 2 runs and leaves no pose) and 256, refine_iterations 0 (the sentinel, stage 2 does not run), min_inliers above the guided rows."""
    s, slot, qset, qxyz, perm, rng = _base(60, 21)
    order = np.argsort(perm)                         # word j is query order[j]
    for a in range(10, 20, 2):                       # equal descriptors in pairs; their queries follow
        slot["desc"][a + 1] = slot["desc"][a]
        qset["desc"][order[a + 1]] = qset["desc"][order[a]]
    P = pnp_model(s["truth"])
    X = np.concatenate([slot["xyz"][:3].astype(np.float64), np.ones((3, 1))], axis=1)
    pc = P @ X.T
    pc[:3] = -pc[:3]
    mirrored = (np.linalg.inv(P) @ pc).T[:, :3]
    slot = dict(desc=np.concatenate([slot["desc"], slot["desc"][:3], slot["desc"][5:6]]), valid=np.ones(64, dtype=np.uint8),
                ids=(2000 + np.arange(64)).astype(np.int32), xyz=np.concatenate([slot["xyz"], mirrored.astype(F), slot["xyz"][5:6]]).astype(F),
                key=21)
    i8 = order[8]
    qset = dict(desc=np.concatenate([qset["desc"], qset["desc"][i8:i8 + 1]]), valid=np.ones(61, dtype=np.uint8),
                xy=np.concatenate([qset["xy"], qset["xy"][i8:i8 + 1] + np.array([[1.5, 0.0]], dtype=F)]).astype(F))
    qxyz = np.concatenate([qxyz, qxyz[i8:i8 + 1]])
    variants = [_v(), _v(xyz=True), _v(verify=dict(guided=0)), _v(verify=dict(guided_radius=0.0)), _v(verify=dict(guided_radius=0.5)),
                _v(verify=dict(guided_max_distance=0)), _v(verify=dict(guided_max_distance=256), xyz=True), _v(pnp=dict(refine_iterations=0)),
                _v(pnp=dict(min_inliers=30, seed=5), verify=dict(guided_radius=0.25))]
    return dict(qset=qset, slots=[slot], query_xyz=qxyz, truth=s["truth"], order=order, variants=variants)


CASES = {"kept_rows": _kept_rows, "rows_512": _rows_512, "nan_points": _nan_points, "ten_equal": _ten_equal, "collinear": _collinear,
         "geometry": _geometry}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for d in [c["qset"]] + c["slots"]:
        for v in d.values():
            if hasattr(v, "setflags"):
                v.setflags(write=False)
    c["query_xyz"].setflags(write=False)
    return c


def pnp_dict(variant):
    return pnc.params_dict(**variant["pnp"])


# ------------------------------------------------------------------------------------------------ what the test files share
HOOK_KEYS = ("samples", "valid", "models", "counts", "refit_tq", "pass_tq", "pass_threshold", "pass_count", "pass_inliers")


def load(case, f, solver=None):
    """The case's query set and store: on host twins, or on the device of `solver`."""
    s = place.DescriptorSet(f, 512)
    db = place.KeyFrameStore(solver, max(len(case["slots"]), 1))
    for k, sl in enumerate(case["slots"]):
        s.upload(np.zeros((len(sl["desc"]), 2), np.float32), sl["desc"], sl["valid"])
        assert db.add(s, sl["ids"], sl["xyz"], sl["key"]) == k
    q = case["qset"]
    s.upload(q["xy"], q["desc"], q["valid"])
    return s, db


def params(variant):
    return pv.default_params(camera=pnp.camera(*K, Tir=TIR), pnp=variant["pnp"], **variant["verify"])


def chain_scene(seed, solver=None):
    """The chain scene of section 9w: a stereo_pair wall, 320 x 240, 200 words, seen again under Motion(t=(6, -4), rot=0.7).
    (flow object, set, store, moved key-points, 3-D points)"""
    w, h = pc.SCENE_W, pc.SCENE_H
    left, right, _ = fo.stereo_pair("plane", width=w, height=h, seed=seed)
    pts = pc.scene_points()
    f = flow.Flow(flow.default_params(**pc.FLOW), w, h, solver=solver) if solver is not None else flow.Flow(flow.default_params(**pc.FLOW), w, h)
    f.push_frame(left, right)
    _, _, xyz = f.stereo(pts, flow.camera(cx=0.5 * (w - 1), cy=0.5 * (h - 1), cx_right=0.5 * (w - 1)))
    s = place.DescriptorSet(f, 200)
    db = place.KeyFrameStore(solver, 2)
    s.describe(pts)
    assert db.add(s, np.arange(200, dtype=np.int32), xyz, seed) == 0
    m = fo.Motion(w, h, (6.0, -4.0), 0.7, 1.0)
    X, Y = fo.grid(w, h)
    back = m.inverse(np.stack([X, Y], -1))
    img = fo.Texture(seed).image(back[..., 0], back[..., 1])
    moved = m.forward(pts).astype(np.float32)
    f.push_frame(img, img)
    s.describe(moved)
    return f, s, db, moved, xyz


def chain_camera():
    return pnp.camera(cx=0.5 * (pc.SCENE_W - 1), cy=0.5 * (pc.SCENE_H - 1))
