"""Inputs the corner tests share (host twin against the NumPy checker, device against host twin), built from the synthetic
texture of flow_oracle.py / flow_cases.py.  Everything is generated; nothing is read from disk."""
import functools

import numpy as np

import clahe_cases
import corners_oracle as co
import flow_cases as fc

SIZES = [(752, 480), (641, 479), (320, 240)]
MIN_DISTANCES = [40.0, 20.0, 7.0, 0.0]
MAX_CORNERS = [300, 20]

# The device sorts through LDS tiles of this many keys and selects in chunks of this many candidates: the "many candidates" inputs
# must need several of each.
DEVICE_TILE = 1024


# The images at which k_corner_response's 32 x 8 tile with its 2-pixel apron meets both borders in one workgroup, and the parameter
# values at which the selection takes another path.  name -> (width, height, corner keywords); the image is edge_image(width, height).
EDGE_FLOW_PARAMS = dict(max_level=0, win_size=3)           # the flow object under them: 5 x 5 must be accepted


def _edge():
    out = {}
    for tag, (w, h) in (("narrower_than_a_tile", (31, 7)), ("exactly_a_tile", (32, 8)), ("one_past_a_tile", (33, 9)), ("smallest", (5, 5))):
        for md in (2.0, 0.0):
            out[f"{tag}_{w}x{h}_md{md:g}"] = (w, h, dict(max_corners=100, quality_level=0.01, min_distance=md))
    out["every_candidate_200x100"] = (200, 100, dict(max_corners=4096, quality_level=1e-6, min_distance=1.0))
    out["one_corner_64x48"] = (64, 48, dict(max_corners=1, quality_level=0.01, min_distance=40.0))
    out["quality_0.999_64x48"] = (64, 48, dict(max_corners=300, quality_level=0.999, min_distance=40.0))
    out["quality_1.5_64x48"] = (64, 48, dict(max_corners=300, quality_level=1.5, min_distance=40.0))
    return out


EDGE = _edge()
SMALL_TILE_CASES = [n for n in EDGE if n.split("_md")[0].endswith(("31x7", "32x8", "33x9"))]


@functools.lru_cache(maxsize=None)
def edge_image(width, height):
    img = clahe_cases.image("texture", width, height, 3)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def edge_checked(name):
    """The checker's result of an EDGE case: computed once, shared, never written to."""
    w, h, kw = EDGE[name]
    out = co.good_features(edge_image(w, h), kw["max_corners"], kw["quality_level"], kw["min_distance"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def tiled_image():
    """Copies of one 64 x 64 patch: equal responses at different raster indices, so the tie rule decides the order."""
    return np.ascontiguousarray(np.tile(fc.base_image(320, 240)[:64, :64], (4, 5)))


def noise_image(width=752, height=480, seed=12):
    return np.random.default_rng(seed).integers(0, 256, (height, width), dtype=np.uint8)


def flat_image(width=320, height=240, value=77):
    return np.full((height, width), value, dtype=np.uint8)


def squares_image(width=752, height=480, seed=4):
    """(image, true corners [n][2]): bright axis-aligned squares (200 on 90), sides 30 .. 49, one per 80 x 80 cell.  A square over
    the pixels [ox, ox + s) has its corners between pixels, at ox - 0.5 and ox + s - 0.5."""
    rng = np.random.default_rng(seed)
    img = np.full((height, width), 90, dtype=np.uint8)
    truth = []
    for gy in range(40, height - 80, 80):
        for gx in range(40, width - 80, 80):
            s = 30 + int(rng.integers(0, 20)); ox = gx + int(rng.integers(0, 10)); oy = gy + int(rng.integers(0, 10))
            img[oy:oy + s, ox:ox + s] = 200
            truth += [(ox - 0.5, oy - 0.5), (ox + s - 0.5, oy - 0.5), (ox - 0.5, oy + s - 0.5), (ox + s - 0.5, oy + s - 0.5)]
    return img, np.array(truth, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def checked(width, height, max_corners, min_distance, quality_level=0.01):
    """The checker's result on base_image (cached: the same extraction seeds several scenarios)."""
    return co.good_features(fc.base_image(width, height), max_corners, quality_level, min_distance)


def mask_scenario(width=752, height=480):
    """The disc list of a frame in mid-run: 90 tracked points (corners of a first extraction, jittered by up to half a pixel), 6
    more tracked points that have drifted to (25, 10) from another one, so that their centres lie inside an earlier disc, and 20 blocked
    points at half the radius."""
    first = checked(width, height, 300, 40.0)["xy"]
    rng = np.random.default_rng(21)
    keep = rng.permutation(len(first))
    tracked = first[keep[:90]] + rng.uniform(-0.5, 0.5, (90, 2)).astype(np.float32)
    blocked = first[keep[90:110]]
    extra = tracked[:6] + np.array([[25.0, 10.0]], dtype=np.float32)
    extra[:, 0] = np.clip(extra[:, 0], 0, width - 1); extra[:, 1] = np.clip(extra[:, 1], 0, height - 1)
    return [(float(x), float(y), 40) for x, y in np.concatenate([tracked, extra])] + [(float(x), float(y), 20) for x, y in blocked]


def special_discs(width=752, height=480):
    """Named discs whose draw decision is known by construction: name -> (disc list, expected drawn flags)."""
    return {
        # hw_40[0] = 40 covers a centre exactly 40 px along the row; the undrawn second disc does not cover the third
        "row_40_apart": ([(200.0, 100.0, 40), (240.0, 100.0, 40), (281.0, 100.0, 40)], [1, 0, 1]),
        "row_41_apart": ([(200.0, 100.0, 40), (241.0, 100.0, 40)], [1, 1]),
        # half to even: 100.5 -> 100 (inside the first disc's reach of 20), 101.5 -> 102 (outside it: 102 - 81 = 21)
        "half_to_even": ([(81.0, 50.0, 20), (100.5, 50.0, 3), (101.5, 50.0, 3)], [1, 0, 1]),
        # outside the image: drawn without the test, clipped; the second lies wholly outside
        "outside": ([(-10.0, 30.0, 40), (float(width) + 500.0, -700.0, 40), (5.0, 30.0, 40), (float(width) - 1.0, float(height) - 1.0, 0)],
                    [1, 1, 0, 1]),
    }


def full_cover_discs(width, height):
    return [(width / 2.0, height / 2.0, 2 * max(width, height))]
