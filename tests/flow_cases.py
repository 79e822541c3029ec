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


def sequence(n_frames=20, width=320, height=240, seed=5):
    """A sequence of stereo pairs of a texture drifting and turning a little more each frame, and the per-frame Motion."""
    tex = fo.Texture(seed)
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
