"""Inputs of the CLAHE tests (tests/test_clahe_host.py, tests/test_gpu_clahe.py), built from numpy.random.default_rng seeds.

Sizes: 64 x 48 divides into 8 x 8 tiles (8 x 6 pixels, clip 1); 70 x 52 divides on neither side; 64 x 50 fails on the height alone, so
eight more columns come with the rows; 256 x 128 has 32 x 16 tiles and clip 6.  Contents: a sum-of-sinusoids texture over the full
range, the same squeezed into grey levels 100 .. 131, a constant image and uniform noise.  One variation of the parameters at
256 x 128: no clipping, and 4 x 2 tiles.  Left and right of a case differ.  EDGE holds the shapes the device code splits on; its
cases stand beside cases(), so what is asserted over every case of cases() is unchanged.
"""
import functools

import numpy as np

import clahe_oracle

SIZES = [(64, 48), (70, 52), (64, 50), (256, 128)]
CONTENTS = ["texture", "low_contrast", "constant", "noise"]
DEFAULT = dict(clip_limit=3.0, tiles_x=8, tiles_y=8)
VARIATIONS = [dict(clip_limit=0.0, tiles_x=8, tiles_y=8), dict(clip_limit=3.0, tiles_x=4, tiles_y=2)]
# the flow object under the small images: visfs_flow_create wants the top level wider than the window + 2
FLOW_PARAMS = dict(max_level=1, win_size=5)


def _texture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    s = np.zeros((h, w))
    for _ in range(6):
        fx, fy = rng.uniform(0.02, 0.45, 2)
        s += rng.uniform(0.4, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
    s = (s - s.min()) / (s.max() - s.min())
    return s


def image(content, w, h, seed):
    if content == "texture":
        return np.rint(_texture(w, h, seed) * 255.0).astype(np.uint8)
    if content == "low_contrast":
        return (100 + np.rint(_texture(w, h, seed) * 31.0)).astype(np.uint8)
    if content == "constant":
        return np.full((h, w), 57 + seed % 100, dtype=np.uint8)
    if content == "noise":
        return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)
    raise KeyError(content)


# The shapes at which the device code takes another path than the host loops (tag, width, height, tiles_x, tiles_y, clip_limit), noise
# content.  k_clahe_lut steps through a tile by dq = 256 / tile_w rows and dr = 256 - dq * tile_w columns: dq == 0 above 256 columns,
# dr == 0 at exactly 256.  k_clahe_apply handles four pixels a thread and the last thread byte by byte when the area is no multiple
# of 4.  One tile on an axis clamps both of its blend tiles to 0.  The tile widths in the tags are the checker's geometry: a side that
# does not divide adds tiles - side % tiles columns to BOTH sides, so 256 x 37 in 1 x 3 tiles has tiles 257 wide.
EDGE = [
    ("tile_w_300_one_tile", 300, 40, 1, 1, 3.0),
    ("tile_w_256", 512, 40, 2, 1, 3.0),
    ("tile_w_258_clip_40", 257, 37, 1, 3, 40.0),
    ("tile_w_257", 256, 37, 1, 3, 3.0),
    ("area_mod4_3", 71, 53, 8, 8, 3.0),
    ("tiles_32x32", 33, 33, 32, 32, 3.0),
    ("width_tiles_plus_1", 9, 7, 8, 6, 3.0),
    ("no_clip", 6, 6, 5, 5, 0.0),
    ("one_tile", 5, 5, 1, 1, 3.0),
    ("narrowest", 5, 5, 4, 4, 3.0),
]
EDGE_TILE_W = {"tile_w_300_one_tile": 300, "tile_w_256": 256, "tile_w_258_clip_40": 258, "tile_w_257": 257}
# the flow object under them: one level and the smallest window, so that 5 x 5 is accepted
EDGE_FLOW_PARAMS = dict(max_level=0, win_size=3)


def _case(content, w, h, params, k, tag=None, flow_params=None):
    name = f"{content}_{w}x{h}_c{params['clip_limit']:g}_t{params['tiles_x']}x{params['tiles_y']}"
    return dict(name=name if tag is None else f"{tag}_{name}", tag=tag, content=content, w=w, h=h, params=dict(params),
                flow=dict(FLOW_PARAMS if flow_params is None else flow_params),
                left=image(content, w, h, 1000 + 2 * k), right=image(content, w, h, 1001 + 2 * k))


@functools.lru_cache(maxsize=None)
def cases():
    out, k = [], 0
    for w, h in SIZES:
        for content in CONTENTS:
            out.append(_case(content, w, h, DEFAULT, k)); k += 1
    for prm in VARIATIONS:
        for content in CONTENTS:
            out.append(_case(content, 256, 128, prm, k)); k += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_cases():
    return tuple(_case("noise", w, h, dict(clip_limit=clip, tiles_x=tx, tiles_y=ty), 500 + k, tag, EDGE_FLOW_PARAMS)
                 for k, (tag, w, h, tx, ty, clip) in enumerate(EDGE))


NAMES = [c["name"] for c in cases()]
EDGE_NAMES = [c["name"] for c in edge_cases()]


def case(name):
    return next(c for c in cases() + edge_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, image_index):
    """The checker's result for one image of a case: computed once, shared, never written to."""
    c = case(name)
    out = clahe_oracle.clahe(c["right" if image_index else "left"], **c["params"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def big_pair(w=752, h=480):
    return image("texture", w, h, 77), image("low_contrast", w, h, 78)
