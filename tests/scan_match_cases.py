"""The scenes the scan-match tests share (CPU: twin against checker; GPU: device against twin), so both see the same inputs.

A case is a dict: `limit` (LocalMap/NumRangeDataLimit), `frames` (the insertions: (Twr, [range data])), `index` (the sub-map
matched), `truth` and `guess` (x, y, yaw), `points` ([n][3], robot frame) and `prm` (linear window, angular window, tw, rw).
Everything is generated from fixed seeds.
"""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# An asymmetric room: a 5 m x 3.5 m outline with a 1.0 m x 0.8 m notch in one corner, and a 0.5 m pillar.
OUTLINE = [(-2.25, -1.75), (2.75, -1.75), (2.75, 0.95), (1.75, 0.95), (1.75, 1.75), (-2.25, 1.75)]
PILLAR = [(-1.35, 0.5), (-0.85, 0.5), (-0.85, 1.0), (-1.35, 1.0)]


def _segments():
    seg = []
    for poly in (OUTLINE, PILLAR):
        for i in range(len(poly)):
            seg.append((poly[i], poly[(i + 1) % len(poly)]))
    return np.asarray(seg, dtype=np.float64)          # [m][2][2]


SEGMENTS = _segments()


def cast(pose, n, rng, noise=0.005, max_range=None, fov=2 * math.pi, extra=()):
    """n returns of a planar laser at `pose` (x, y, yaw), in the robot frame ([n][3], z = 0): the nearest wall along each
    ray plus range noise; max_range caps the range; `extra` appends returns at the given (angle, range)."""
    x, y, yaw = pose
    ang = (np.arange(n) + 0.5) / n * fov - fov / 2
    d = np.stack([np.cos(ang + yaw), np.sin(ang + yaw)], -1)                     # world directions
    a, b = SEGMENTS[:, 0], SEGMENTS[:, 1]
    e = b - a
    r = np.full(n, np.inf)
    for j in range(len(SEGMENTS)):
        den = d[:, 0] * e[j, 1] - d[:, 1] * e[j, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a[j, 0] - x) * e[j, 1] - (a[j, 1] - y) * e[j, 0]) / den
            u = ((a[j, 0] - x) * d[:, 1] - (a[j, 1] - y) * d[:, 0]) / den
        ok = (np.abs(den) > 1e-12) & (t > 1e-9) & (u >= 0) & (u <= 1)
        r = np.where(ok & (t < r), t, r)
    assert np.all(np.isfinite(r)), "a ray left the room"
    r = r + noise * rng.normal(size=n)
    if max_range is not None:
        r = np.minimum(r, max_range)
    ang = list(ang) + [e_[0] for e_ in extra]
    r = list(r) + [e_[1] for e_ in extra]
    return np.stack([np.asarray(r) * np.cos(ang), np.asarray(r) * np.sin(ang), np.zeros(len(r))], -1)


def pose_T(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return [c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, 0.0]


def arc_frames(n_frames, n_returns, rng, **kw):
    """Insertions along a short arc from the origin."""
    out = []
    for f in range(n_frames):
        p = (0.08 * f, 0.03 * f * f / max(n_frames - 1, 1), 0.07 * f)
        out.append((pose_T(*p), [([0.0, 0.0, 0.0], cast(p, n_returns, rng, **kw), np.zeros((0, 3)))]))
    return out


TRUTH = (0.35, 0.10, 0.33)
BASE_PRM = (0.3, 0.2, 0.1, 0.1)
BASE_ERRORS = [(0.12, -0.09, 0.06), (-0.2, 0.15, -0.1), (0.0, 0.0, 0.0), (0.25, 0.25, 0.12), (-0.25, 0.1, -0.15)]


def _guess(err):
    return (TRUTH[0] + err[0], TRUTH[1] + err[1], TRUTH[2] + err[2])


def _base_parts():
    rng = np.random.default_rng(20)
    frames = arc_frames(6, 240, rng)
    scan = cast(TRUTH, 200, rng)
    return frames, scan


def base_cases():
    """The base scene: six insertions of 240 returns, a 200-return scan, windows 0.3 m / 0.2 rad, five guess errors."""
    frames, scan = _base_parts()
    return [dict(name=f"base{i}", limit=50, frames=frames, index=0, truth=TRUTH, guess=_guess(e), points=scan, prm=BASE_PRM)
            for i, e in enumerate(BASE_ERRORS)]


def chunk_size():
    """kChunk of visfs_amd/csrc/ba_scan.hpp: the points one workgroup stages in LDS at a time."""
    src = open(os.path.join(ROOT, "visfs_amd", "csrc", "ba_scan.hpp")).read()
    return int(re.search(r"constexpr\s+int\s+kChunk\s*=\s*(\d+)\s*;", src).group(1))


def edge_cases():
    frames, scan = _base_parts()
    rng = np.random.default_rng(21)
    err = BASE_ERRORS[0]
    small = (0.05, 0.03, 0.1, 0.1)                       # nl = 1, a handful of rotations: cheap for the checker
    out = []

    def add(name, **kw):
        c = dict(name=name, limit=50, frames=frames, index=0, truth=TRUTH, guess=_guess(err), points=scan, prm=small)
        c.update(kw)
        out.append(c)

    for n in (1, 63, 65, chunk_size() + 1):
        add(f"n{n}", points=cast(TRUTH, n, rng))
    add("nl0", prm=(0.0, 0.1, 0.1, 0.1))
    add("nl10", prm=(0.5, 0.03, 0.1, 0.1))
    add("one_scan", prm=(0.1, 0.0, 0.1, 0.1))
    # 12 m returns (through a doorway, as it were) make the angular step small: about 170 rotations in 0.35 rad
    far = [(-0.4 + 0.04 * i, 12.0) for i in range(20)]
    add("many_scans", points=cast(TRUTH, 80, rng, extra=far), prm=(0.05, 0.35, 0.1, 0.1))
    add("outside", guess=(12.0, 0.5, 0.2))                                       # every cell read lies outside the grid
    add("grid_edge", guess=(4.95, -4.95, 0.2), prm=(0.2, 0.03, 0.1, 0.1))       # negative indices and indices >= nx among inside ones
    # a match right after an insertion that grew the grid: a short-range frame keeps the first 100 x 100 cells, the next one doubles them
    near = (pose_T(0.0, 0.0, 0.0), [([0.0, 0.0, 0.0], cast((0.0, 0.0, 0.0), 120, rng, max_range=1.2), np.zeros((0, 3)))])
    add("after_growth", frames=[near, frames[0]], prm=(0.1, 0.05, 0.1, 0.1))
    # limit 3, six insertions: the front is finished and cropped (its walls lie on the grid's border), a second sub-map is active
    add("cropped_front", limit=3, prm=(0.2, 0.03, 0.1, 0.1))
    add("second_submap", limit=3, index=1)
    return out


def unknown_case(tw, rw):
    """A sub-map whose grid is all unknown (one empty range data): every candidate has Q = 0."""
    _, scan = _base_parts()
    empty = (pose_T(0.0, 0.0, 0.0), [([0.0, 0.0, 0.0], np.zeros((0, 3)), np.zeros((0, 3)))])
    return dict(name="unknown", limit=50, frames=[empty], index=0, truth=TRUTH, guess=TRUTH, points=scan[:40], prm=(0.1, 0.05, tw, rw))


def fill(sub, case):
    """The case's insertions into a submap.Submaps (either flavour)."""
    for T, rds in case["frames"]:
        assert sub.insert(T, rds) == 0, sub.last_error()
