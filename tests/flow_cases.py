"""Inputs the flow tests share (host twin against the NumPy checker, device against host twin), built from the synthetic scenes
of flow_oracle.py.  Everything is generated; nothing is read from disk."""
import functools

import numpy as np

import flow_oracle as fo

SEED = 1
MARGIN = 40          # ground truth is asked of points at least this far from the border
N_POINTS = 300

# name -> (width, height, with guess, flow_back, max_level)
CASES = {
    "plain": (752, 480, False, 1, 3),
    "guess": (752, 480, True, 1, 3),
    "no_back": (752, 480, False, 0, 3),
    "one_level": (752, 480, True, 1, 0),
    "one_level_no_guess": (752, 480, False, 1, 0),
    "odd_size": (641, 479, True, 1, 3),
}


@functools.lru_cache(maxsize=None)
def base_image(width, height, seed=SEED):
    X, Y = fo.grid(width, height)
    return fo.Texture(seed).image(X, Y)


@functools.lru_cache(maxsize=None)
def moved_pair(width, height, kind="step", seed=SEED):
    """(second left, second right, Motion, Disparity): the first left is base_image; the second left is it moved by the Motion, the
    second right shows the second left through the Disparity."""
    tex = fo.Texture(seed)
    X, Y = fo.grid(width, height)
    m = fo.Motion(width, height)
    d = fo.Disparity(kind, width)
    p = m.inverse(np.stack([X, Y], -1))
    q = m.inverse(np.stack([d.left_of_right(X), Y], -1))
    return tex.image(p[..., 0], p[..., 1]), tex.image(q[..., 0], q[..., 1]), m, d


@functools.lru_cache(maxsize=None)
def still_pair(width, height, kind, seed=SEED):
    """(left, right, Disparity) of the unmoved texture."""
    X, Y = fo.grid(width, height)
    d = fo.Disparity(kind, width)
    return base_image(width, height, seed), fo.Texture(seed).image(d.left_of_right(X), Y), d


def case(name):
    """dict: params keywords, the two pushed stereo pairs, the points (a few of them near and beyond the border) and the guess."""
    width, height, with_guess, flow_back, max_level = CASES[name]
    first = base_image(width, height)
    left, right, m, d = moved_pair(width, height)
    pts = fo.random_points(N_POINTS - 8, width, height, 4, seed=3)
    edge = np.array([[-40.0, 100.0], [width + 25.0, 100.0], [100.0, -35.5], [100.0, height + 30.0], [2.25, 3.5], [width - 1.5, height - 2.0],
                     [-11.5, 200.0], [300.0, -10.75]], dtype=np.float32)
    pts = np.concatenate([pts, edge]).astype(np.float32)
    guess = None
    if with_guess:
        rng = np.random.default_rng(11)
        guess = (m.forward(pts) + rng.normal(0.0, 1.5, pts.shape)).astype(np.float32)
    return dict(width=width, height=height, prm=dict(flow_back=flow_back, max_level=max_level), frames=[(first, first), (left, right)],
                pts=pts, guess=guess, motion=m, disparity=d)


# ------------------------------------------------------------------------------------------------ edge cases
# The shapes at which the device code takes another path than at the defaults.  A wavefront holds window cell s * 64 + lane in slot s
# of 7, so win_size decides which slots are full: 3, 4, 5, 7 end inside slot 0, 8 and 16 end exactly on a slot boundary (64 and 256
# cells), 9 and 17 one row of cells past it, 15 and 20 inside slots 3 and 6, and the even sizes have a half-pixel `half`.
# name -> dict(size, prm, scene, points, need):
#   scene   "texture" (sequence(2)), "noise" and "quadrant" (0 / 255 pixels only: the largest products the int32 partial sums of a
#           lane can meet), "texture_cheap" (fewer waves, for the one large image), "texture_band" (the texture with a constant band
#           of columns: without an iteration nothing moves and every point comes back to its start, so the texture alone drops only
#           the three rows that are not finite)
#   points  number of random points in front of FIXED_ROWS, or "lattice" (9 x 9 at 2.5 px around the quadrants' junction)
#   need    what the checker alone must give in track() so that the comparison is not one of empty outcomes: "both" at least 4 kept
#           and at least 4 dropped, "kept" at least 4 kept, None bytes only
EDGE_SIZES = ((160, 120), (161, 121))
SLOT_WINDOWS = (3, 4, 5, 7, 8, 9, 15, 16, 17, 20, 21)
SATURATION_WINDOWS = (21, 16, 8, 3)
JUNCTION, JUNCTION_MOVED = (80, 60), (82, 61)
BAND = (40, 75)        # columns of the constant band of "texture_band": a window of 21 wholly inside it has no gradient at all
STEREO_SHIFT = 3
EDGE_BASELINE = 0.05   # of the camera the edge cases triangulate with: a disparity of STEREO_SHIFT px is 7.25 m, inside the depth gates


def _edge_cases():
    out = {}
    for k, win in enumerate(SLOT_WINDOWS):
        out[f"win_{win}"] = dict(size=EDGE_SIZES[k % 2], prm=dict(win_size=win, max_level=2), scene="texture", points=120, need="both")
    for win in (8, 9):
        size = out[f"win_{win}"]["size"]
        out[f"win_{win}_back0"] = dict(size=size, prm=dict(win_size=win, max_level=2, flow_back=0), scene="texture", points=120, need="both")
    for k, win in enumerate(SATURATION_WINDOWS):
        out[f"saturated_noise_win_{win}"] = dict(size=EDGE_SIZES[k % 2], prm=dict(win_size=win, max_level=2), scene="noise", points=120,
                                                 need="both")
        # at window 21 every lattice point sees the junction and the checker keeps all 81: nothing is dropped there
        out[f"saturated_quadrant_win_{win}"] = dict(size=EDGE_SIZES[0], prm=dict(win_size=win, max_level=2), scene="quadrant",
                                                    points="lattice", need="kept" if win == 21 else "both")
    # the 8-level Layout: 513 -> 257 -> 129 -> 65 -> 33 -> 17 -> 9 -> 5, the top level exactly win_size + 2
    out["levels_8_top_5x5"] = dict(size=(513, 513), prm=dict(win_size=3, max_level=7), scene="texture_cheap", points=40, need="kept")
    out["levels_2_win_21"] = dict(size=(160, 120), prm=dict(win_size=21, max_level=1), scene="texture", points=120, need="kept")
    # the smallest accepted images: every window reflects at both borders.  The checker keeps nothing at 5 x 5 (and nothing in the
    # stereo call at 23 x 23), so those compare bytes only.
    out["smallest_23x23_win_21"] = dict(size=(23, 23), prm=dict(win_size=21, max_level=0), scene="texture", points=120, need=None)
    out["smallest_5x5_win_3"] = dict(size=(5, 5), prm=dict(win_size=3, max_level=0), scene="texture", points=120, need=None)
    out["smallest_92x92_top_23x23"] = dict(size=(92, 92), prm=dict(win_size=21, max_level=2), scene="texture", points=120, need=None)
    out["iterations_0_win_21"] = dict(size=(160, 120), prm=dict(win_size=21, max_level=2, iterations=0), scene="texture_band", points=120, need="both")
    out["iterations_1_win_9"] = dict(size=(161, 121), prm=dict(win_size=9, max_level=2, iterations=1), scene="texture", points=120, need="both")
    return out


EDGE_CASES = _edge_cases()


def fixed_rows(width, height):
    """Points beyond and on the border, and the values no window corner can be taken from."""
    return np.array([[-3.0, 5.0], [width + 2.0, 4.0], [0.0, 0.0], [width - 1.0, height - 1.0], [np.nan, 3.0], [np.inf, 2.0], [1e30, 1.0]],
                    dtype=np.float32)


def _right_of(left):
    """The right image of a fronto-parallel scene: disparity STEREO_SHIFT everywhere (the columns wrap around)."""
    return np.ascontiguousarray(np.roll(left, -STEREO_SHIFT, axis=1))


def _quadrants(width, height, junction):
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    return np.where((x < junction[0]) == (y < junction[1]), 255, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def edge_frames(scene, width, height):
    """The two stereo pairs of a scene; the motion between them is (2.5, -1.25) px for the textures, (2, 1) px for the others."""
    if scene == "texture":
        return sequence(2, width, height)
    if scene == "texture_cheap":
        return sequence(2, width, height, n_waves=24)
    if scene == "texture_band":
        frames = [tuple(img.copy() for img in pair) for pair in sequence(2, width, height)]
        for pair in frames:
            for img in pair:
                img[:, BAND[0]:BAND[1]] = 128
        return frames
    if scene == "noise":
        first = np.random.default_rng(42).integers(0, 2, (height, width)).astype(np.uint8) * 255
        second = np.ascontiguousarray(np.roll(first, (1, 2), axis=(0, 1)))
    elif scene == "quadrant":
        first, second = _quadrants(width, height, JUNCTION), _quadrants(width, height, JUNCTION_MOVED)
    else:
        raise KeyError(scene)
    return [(first, _right_of(first)), (second, _right_of(second))]


@functools.lru_cache(maxsize=None)
def _edge_case(name):
    spec = EDGE_CASES[name]
    width, height = spec["size"]
    frames = edge_frames(spec["scene"], width, height)
    if spec["points"] == "lattice":
        g = 2.5 * (np.arange(9) - 4.0)
        gx, gy = np.meshgrid(JUNCTION[0] + g, JUNCTION[1] + g)
        pts = np.stack([gx.ravel(), gy.ravel()], -1).astype(np.float32)
    else:
        pts = np.concatenate([fo.random_points(spec["points"], width, height, 1, seed=17), fixed_rows(width, height)]).astype(np.float32)
    step = (2.5, -1.25) if spec["scene"].startswith("texture") else (2.0, 1.0)
    guess = (pts + np.asarray(step, dtype=np.float32) + np.random.default_rng(19).normal(0.0, 0.75, pts.shape)).astype(np.float32)
    guess[1] = np.nan                               # one guess that no window can start from
    for a in (pts, guess) + tuple(img for pair in frames for img in pair):
        a.setflags(write=False)
    return dict(name=name, width=width, height=height, prm=dict(spec["prm"]), frames=frames, pts=pts, guess=guess, need=spec["need"])


def edge_case(name):
    return dict(_edge_case(name))


def check_not_vacuous(name, status, what="track"):
    """Prints the checker's kept and dropped counts of a call and holds them to the case's `need`."""
    kept, dropped = int((status == 1).sum()), int((status == 0).sum())
    print(f"{name} {what}: the checker keeps {kept} and drops {dropped} of {len(status)}")
    need = EDGE_CASES[name]["need"]
    if need in ("both", "kept"):
        assert kept >= 4, (name, what, kept)
    if need == "both":
        assert dropped >= 4, (name, what, dropped)
    return kept, dropped


def sequence(n_frames=20, width=320, height=240, seed=5, n_waves=200):
    """A sequence of stereo pairs of a texture drifting and turning a little more each frame, and the per-frame Motion."""
    tex = fo.Texture(seed, n_waves)
    X, Y = fo.grid(width, height)
    d = fo.Disparity("slant", width)
    frames = []
    for k in range(n_frames):
        m = fo.Motion(width, height, t=(2.5 * k, -1.25 * k), rot=0.004 * k, zoom=1.0 + 0.002 * k)
        p = m.inverse(np.stack([X, Y], -1))
        q = m.inverse(np.stack([d.left_of_right(X), Y], -1))
        frames.append((tex.image(p[..., 0], p[..., 1]), tex.image(q[..., 0], q[..., 1])))
    return frames


def truth_points(width, height, n=N_POINTS, seed=7):
    return fo.random_points(n, width, height, MARGIN, seed)


def constant_patch_pair(width=752, height=480):
    """Two frames with the same constant 64 x 64 patch; the point at its centre has a zero minimum eigenvalue."""
    a = base_image(width, height).copy()
    b = moved_pair(width, height)[0].copy()
    a[200:264, 300:364] = 128
    b[200:264, 300:364] = 128
    return a, b, np.array([[331.5, 231.5]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def replaced_region_pair(width=752, height=480):
    """The moved pair with a region of the second frame replaced by a differently seeded texture, and a lattice of points over and
    around it: the forward pass lands somewhere on the foreign texture, and the round trip does not come back."""
    a = base_image(width, height)
    b = moved_pair(width, height)[0].copy()
    X, Y = fo.grid(width, height)
    other = fo.Texture(SEED + 100).image(X, Y)
    b[170:330, 280:480] = other[170:330, 280:480]
    gx, gy = np.meshgrid(np.arange(250.0, 500.0, 9.0), np.arange(150.0, 350.0, 9.0))
    return a, b, np.stack([gx.ravel(), gy.ravel()], -1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ ground truth
# The bounds are the reference's own acceptance gates (Tracker.cpp:268, :364), not measurements: a kept point lies within 1.5 px
# (track) / 0.5 px (stereo) of the truth, its depth within what 0.5 px of disparity changes at that depth, and at most 10 % of the
# qualifying points come back with status 0.
TRACK_GATE, STEREO_GATE, MAX_DROPPED = 1.5, 0.5, 0.10


def check_track_truth(track, width=752, height=480):
    """track(from_xy) -> (to_xy, status, err) on the frames (base_image, moved_pair).  Returns (kept, n, max error, median error)."""
    m = moved_pair(width, height)[2]
    pts = truth_points(width, height)
    to, st, _ = track(pts)
    e = np.linalg.norm(to.astype(np.float64) - m.forward(pts), axis=1)
    kept = st == 1
    print(f"track truth {width}x{height}: kept {kept.sum()} of {len(pts)}, error max {e[kept].max():.4f} px, median {np.median(e[kept]):.4f} px")
    assert (e[kept] <= TRACK_GATE).all(), e[kept].max()
    assert (~kept).sum() <= MAX_DROPPED * len(pts), (~kept).sum()
    return int(kept.sum()), len(pts), float(e[kept].max()), float(np.median(e[kept]))


def check_stereo_truth(stereo, kind, cam_fb, width=752, height=480):
    """stereo(left_xy) -> (right_xy, status, xyz) on still_pair(kind), with the default camera (robot x = optical z)."""
    d = still_pair(width, height, kind)[2]
    pts = truth_points(width, height)
    rt, st, xyz = stereo(pts)
    xr, disp, seen = d.right_of_left(pts[:, 0])
    q = seen & d.window_clear(pts[:, 0])
    e = np.hypot(rt[:, 0].astype(np.float64) - xr, rt[:, 1].astype(np.float64) - pts[:, 1])
    kept = (st == 1) & q
    z = cam_fb / disp
    tol = cam_fb / (disp - STEREO_GATE) - z
    ez = np.abs(xyz[:, 0].astype(np.float64) - z)
    print(f"stereo truth {kind}: {q.sum()} qualify, kept {kept.sum()}, error max {e[kept].max():.4f} px, median {np.median(e[kept]):.4f} px, "
          f"depth error max {ez[kept].max():.4f} m (allowed there {tol[kept][np.argmax(ez[kept])]:.4f} m)")
    assert (e[kept] <= STEREO_GATE).all(), e[kept].max()
    assert np.isfinite(xyz[kept]).all()
    assert (ez[kept] <= tol[kept]).all()
    assert (q & (st == 0)).sum() <= MAX_DROPPED * q.sum(), (q & (st == 0)).sum()
    return int(kept.sum()), int(q.sum()), float(e[kept].max()), float(np.median(e[kept])), float(ez[kept].max())
