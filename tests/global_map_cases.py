"""The tiles and compositions the global-map tests share (CPU: twin against checker; GPU: device against twin), all tiny and
generated from fixed seeds.

A case is a dict: `name`, `tiles` (dicts of `cells` [ny][nx] uint16, `limits`, `pose`), and the compose arguments `resolution`
and `limits` (None: limits from the tiles' extents).  Every case is composed in the three modes.
"""
import math

import numpy as np

PALETTE = np.array([0, 0, 1, 900, 9000, 16384, 16385, 24000, 32000, 32767], dtype=np.uint16)


def limits(nx, ny, res=0.05, max_x=None, max_y=None):
    """Limits of nx x ny cells; by default centred on the origin."""
    return dict(resolution=res, max_x=ny * res / 2 if max_x is None else max_x, max_y=nx * res / 2 if max_y is None else max_y,
                num_x_cells=nx, num_y_cells=ny)


def tile(rng, nx, ny, pose=(0.0, 0.0, 0.0), res=0.05, max_x=None, max_y=None, palette=False, unknown=0.3):
    if palette:
        cells = PALETTE[rng.integers(0, len(PALETTE), size=(ny, nx))]
    else:
        cells = rng.integers(1, 32768, size=(ny, nx)).astype(np.uint16)
        cells[rng.random((ny, nx)) < unknown] = 0
    return dict(cells=cells, limits=limits(nx, ny, res, max_x, max_y), pose=tuple(float(v) for v in pose))


def _stack256():
    """256 tiles of 4 x 4 on one spot.  Row 0: all value 1, row 1: all 32767 (both clamps); row 2: v beside 32768 - v, which sum
    to zero (16384); row 3: anything.  Column 3 of row 3 is unknown in the last tile: the count saturates at 255 either way."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(256):
        c = np.zeros((4, 4), dtype=np.uint16)
        c[0, :] = 1
        c[1, :] = 32767
        v = np.array([5, 1000, 16384, 30000])
        c[2, :] = v if k % 2 == 0 else 32768 - v
        c[3, :] = rng.integers(1, 32768, size=4)
        if k == 255:
            c[3, 3] = 0
        out.append(dict(cells=c, limits=limits(4, 4), pose=(0.0, 0.0, 0.0)))
    return out


def _ring64():
    """64 tiles of 64 x 64 cells (3.2 m) around a ring of 4 m radius, each turned along the ring: about 250 output cells a side."""
    rng = np.random.default_rng(8)
    out = []
    for k in range(64):
        a = 2 * math.pi * k / 64
        out.append(tile(rng, 64, 64, pose=(4.0 * math.cos(a), 4.0 * math.sin(a), a + 0.5 * math.pi), palette=True))
    return out


def cases():
    rng = np.random.default_rng(5)
    out = []

    def add(name, tiles, resolution=0.05, lim=None):
        out.append(dict(name=name, tiles=tiles, resolution=resolution, limits=lim))

    add("one_3x5", [tile(rng, 3, 5, pose=(0.1, -0.2, 0.4))])
    add("two_overlapping", [tile(rng, 12, 9), tile(rng, 12, 9, pose=(0.025, 0.025, 0.3))])
    # explicit output grids at the edges of the 64 x 4 block, cut out of two tiles that cover them
    wide = [tile(rng, 80, 12, unknown=0.1), tile(rng, 80, 12, pose=(0.01, -0.03, 0.05), unknown=0.1)]
    for nx, ny in ((1, 1), (63, 1), (64, 1), (65, 1), (1, 3), (1, 4), (1, 5), (65, 5)):
        add(f"out_{nx}x{ny}", wide, lim=limits(nx, ny, max_x=0.125, max_y=1.625))
    add("tile_outside", [tile(rng, 6, 6), tile(rng, 6, 6, pose=(3.0, 3.0, 0.2))], lim=limits(10, 10))
    add("tile_partly_outside", [tile(rng, 6, 6), tile(rng, 8, 8, pose=(0.3, -0.25, 0.7))], lim=limits(10, 10))
    add("all_outside", [tile(rng, 6, 6, pose=(3.0, 3.0, 0.2))], lim=limits(10, 10))
    add("mixed_resolutions", [tile(rng, 20, 16, res=0.025, pose=(0.0, 0.1, -0.2)), tile(rng, 6, 5, res=0.1, pose=(0.05, 0.0, 0.6)),
                              tile(rng, 9, 9)])
    marked = tile(rng, 7, 6, pose=(0.0, 0.0, 1.2))
    marked["cells"] = marked["cells"] | np.where(rng.random((6, 7)) < 0.5, 32768, 0).astype(np.uint16)
    add("markers", [marked, tile(rng, 7, 6)])
    add("coarse_output", [tile(rng, 30, 20, pose=(0.2, 0.1, 2.0)), tile(rng, 30, 20)], resolution=0.13)
    add("stack256", _stack256())
    add("ring64", _ring64())
    return out


def scan_of(rng, n=40, radius=0.25):
    """A scan's returns (robot frame, [n][3]) within `radius` of the origin."""
    p = np.zeros((n, 3))
    p[:, :2] = rng.uniform(-radius, radius, size=(n, 2))
    return p
