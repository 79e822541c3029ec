"""The equalised frame push on the host twin (include/visfs_clahe.h) against the NumPy checker tests/clahe_oracle.py, byte for byte:
geometry, final histograms, look-up tables and the equalised level 0 of every case of tests/clahe_cases.py, both images; the pyramids
and derivatives behind it; properties that need no checker; the argument checks."""
import numpy as np
import pytest

import clahe_cases as cc
import clahe_oracle as co
from visfs_amd import abi, backend, clahe, flow


def _flow(w, h, solver=None, params=cc.FLOW_PARAMS):
    return flow.Flow(flow.default_params(**params), w, h, solver=solver)


def _pushed(c):
    f = _flow(c["w"], c["h"], params=c["flow"])
    clahe.push_frame(f, clahe.default_params(**c["params"]), c["left"], c["right"])
    return f


@pytest.mark.parametrize("name", cc.NAMES + cc.EDGE_NAMES)
def test_case_equals_the_checker(name):
    c = cc.case(name)
    assert not np.array_equal(c["left"], c["right"])
    left0, right0 = c["left"].copy(), c["right"].copy()
    f = _pushed(c)
    assert np.array_equal(c["left"], left0) and np.array_equal(c["right"], right0)      # the caller's buffers are not written
    prm = clahe.default_params(**c["params"])
    for image in (clahe.IMAGE_LEFT, clahe.IMAGE_RIGHT):
        want = cc.expected(name, image)
        assert clahe.hook_geometry(prm, c["w"], c["h"]) == want["geometry"]
        st = clahe.download(f, image)
        assert st["hist"].tobytes() == want["hist"].tobytes()
        assert st["lut"].tobytes() == want["lut"].tobytes()
        px, _ = f.download_level(flow.SLOT_CURRENT, image, 0)
        assert px.tobytes() == want["dst"].tobytes()
    f.close()


def test_cases_reach_every_branch_of_the_checker():
    """From the checker's own per-tile figures, so that a later change of the cases cannot hollow the tests out."""
    geo = {(c["w"], c["h"]): cc.expected(c["name"], 0)["geometry"] for c in cc.cases() if c["params"] == cc.DEFAULT}
    assert (geo[(64, 48)]["ext_w"], geo[(64, 48)]["ext_h"], geo[(64, 48)]["tile_w"], geo[(64, 48)]["tile_h"], geo[(64, 48)]["clip"]) == (64, 48, 8, 6, 1)
    assert (geo[(70, 52)]["ext_w"], geo[(70, 52)]["ext_h"]) == (72, 56)
    assert (geo[(64, 50)]["ext_w"], geo[(64, 50)]["ext_h"]) == (72, 56)             # eight more columns although 64 divides
    assert (geo[(256, 128)]["tile_w"], geo[(256, 128)]["tile_h"], geo[(256, 128)]["clip"]) == (32, 16, 6)
    def tiles(content, cond, params=cc.DEFAULT):
        n = 0
        for c in cc.cases():
            if c["content"] == content and (c["w"], c["h"]) == (256, 128) and c["params"] == params:
                for image in (0, 1):
                    e = cc.expected(c["name"], image)
                    n += int(cond(e).sum())
        return n
    assert tiles("noise", lambda e: e["residual"] == 0) > 0                               # nothing to hand out one by one
    assert tiles("noise", lambda e: (e["residual"] >= 1) & (e["residual"] <= 128)) > 0
    for content in ("low_contrast", "constant"):
        assert tiles(content, lambda e: e["residual"] > 128) > 0                    # step 1
        assert tiles(content, lambda e: e["batch"] > 0) > 0
    assert tiles("texture", lambda e: e["clipped"] > 0, cc.VARIATIONS[0]) == 0      # clip_limit 0 clips nothing
    for c in cc.cases():
        for image in (0, 1):
            e = cc.expected(c["name"], image)
            if c["content"] == "constant":
                continue
            # pixels whose blend is an exact .5 over an even floor: round-half-up would store another byte.  Hundreds where the
            # tile sides are powers of two or small (dyadic weights), fewer with the 9 x 7 tiles of the sizes that do not divide.
            assert e["ties"] >= (100 if (c["w"], c["h"]) in ((64, 48), (256, 128)) else 1), (c["name"], image, e["ties"])


def test_edge_cases_have_the_geometry_their_names_state():
    """On the checker's geometry alone: the tile widths around 256, the area that is no multiple of 4, one tile on an axis."""
    geo = {c["tag"]: (c, cc.expected(c["name"], 0)["geometry"]) for c in cc.edge_cases()}
    assert len(geo) == len(cc.EDGE) == 10
    for tag, tile_w in cc.EDGE_TILE_W.items():
        assert geo[tag][1]["tile_w"] == tile_w, tag
    assert geo["tile_w_300_one_tile"][1]["tile_h"] == 40 and geo["tile_w_256"][1]["ext_w"] == 512
    assert geo["tile_w_258_clip_40"][1]["clip"] == int(40.0 * 258 * 13 / 256.0) and geo["no_clip"][1]["clip"] == 0
    c = geo["area_mod4_3"][0]
    assert (c["w"] * c["h"]) % 4 == 3 and c["w"] % 4 != 0
    assert (geo["tiles_32x32"][1]["tile_w"], geo["tiles_32x32"][1]["tile_h"]) == (2, 2)
    assert (geo["width_tiles_plus_1"][1]["ext_w"], geo["width_tiles_plus_1"][1]["ext_h"]) == (16, 12)
    assert (geo["narrowest"][1]["tile_w"], geo["narrowest"][1]["tile_h"]) == (2, 2)
    assert (geo["one_tile"][1]["tile_w"], geo["one_tile"][1]["tile_h"]) == (5, 5)
    for c, g in geo.values():                       # no case is an identity or a constant: the equalised image differs from the raw one
        for image in (0, 1):
            dst = cc.expected(c["name"], image)["dst"]
            assert not np.array_equal(dst, c["right" if image else "left"]) and len(np.unique(dst)) > 4, c["name"]


@pytest.mark.parametrize("name", ["texture_70x52_c3_t8x8", "noise_256x128_c3_t4x2"])
def test_pyramids_and_derivatives_follow_the_equalised_image(name):
    c = cc.case(name)
    f, g = _pushed(c), _flow(c["w"], c["h"])
    g.push_frame(cc.expected(name, 0)["dst"], cc.expected(name, 1)["dst"])
    for image in (0, 1):
        for level in range(cc.FLOW_PARAMS["max_level"] + 1):
            a, b = f.download_level(flow.SLOT_CURRENT, image, level), g.download_level(flow.SLOT_CURRENT, image, level)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (image, level)
    f.close(); g.close()


def test_slots_rotate_as_with_push_frame():
    c, d = cc.case("texture_64x48_c3_t8x8"), cc.case("noise_64x48_c3_t8x8")
    f = _pushed(c)
    f.push_frame(d["left"], d["right"])                                             # a plain push behind an equalised one
    assert f.download_level(flow.SLOT_PREVIOUS, 0, 0)[0].tobytes() == cc.expected(c["name"], 0)["dst"].tobytes()
    assert f.download_level(flow.SLOT_CURRENT, 1, 0)[0].tobytes() == d["right"].tobytes()
    clahe.push_frame(f, clahe.default_params(), d["left"], d["right"])
    assert f.download_level(flow.SLOT_PREVIOUS, 0, 0)[0].tobytes() == d["left"].tobytes()
    assert f.download_level(flow.SLOT_CURRENT, 1, 0)[0].tobytes() == cc.expected(d["name"], 1)["dst"].tobytes()
    f.close()


def test_every_table_is_monotone_and_ends_at_255():
    for c in cc.cases() + cc.edge_cases():
        f = _pushed(c)
        for image in (0, 1):
            st = clahe.download(f, image)
            lut = st["lut"].astype(np.int32)
            assert (np.diff(lut, axis=2) >= 0).all() and (lut[..., 255] == 255).all(), c["name"]
            g = clahe.hook_geometry(clahe.default_params(**c["params"]), c["w"], c["h"])
            assert (st["hist"].sum(axis=2) == g["tile_w"] * g["tile_h"]).all() and (st["hist"] >= 0).all()
        f.close()


def test_an_image_periodic_in_the_tile_size_maps_through_one_table():
    """Every tile holds the same pixels, so all tables agree and the blend's weights sum to one: dst == lut[src]."""
    tile = np.random.default_rng(5).integers(0, 256, size=(8, 16), dtype=np.uint8)
    img = np.tile(tile, (8, 8))                                                      # 128 x 64, 8 x 8 tiles of 16 x 8
    f = _flow(128, 64)
    clahe.push_frame(f, clahe.default_params(), img, img[:, ::-1])
    lut = clahe.download(f, 0)["lut"]
    assert (lut == lut[0, 0]).all()
    assert np.array_equal(f.download_level(flow.SLOT_CURRENT, 0, 0)[0], lut[0, 0][img])
    f.close()


def test_no_clipping_on_a_flat_histogram_is_the_identity_up_to_the_table_rounding():
    """Each tile holds every level area / 256 times: the cumulative count of level v is (v + 1) area / 256, so the table is
    rint((v + 1) * 255 / 256) up to the one float32 rounding of the product, and all tiles share it."""
    rng = np.random.default_rng(6)
    img = np.zeros((64, 128), dtype=np.uint8)
    for ty in range(2):
        for tx in range(4):
            img[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32] = rng.permutation(np.repeat(np.arange(256), 4)).reshape(32, 32)
    f = _flow(128, 64)
    clahe.push_frame(f, clahe.default_params(clip_limit=0.0, tiles_x=4, tiles_y=2), img, img)
    lut = clahe.download(f, 0)["lut"].astype(np.int64)
    exact = (np.arange(256) + 1) * 255.0 / 256.0
    assert (np.abs(lut - exact[None, None, :]) <= 0.5 + 1e-4).all()
    out = f.download_level(flow.SLOT_CURRENT, 0, 0)[0].astype(np.int64)
    assert np.abs(out - img).max() <= 1 and np.array_equal(out, lut[0, 0][img])
    f.close()


def test_stride_larger_than_width():
    c = cc.case("texture_70x52_c3_t8x8")
    wide = np.full((2, c["h"], c["w"] + 13), 255, dtype=np.uint8)
    wide[0, :, :c["w"]], wide[1, :, :c["w"]] = c["left"], c["right"]
    f = _flow(c["w"], c["h"])
    clahe.push_frame(f, clahe.default_params(), wide[0, :, :c["w"]], wide[1, :, :c["w"]])
    for image in (0, 1):
        assert f.download_level(flow.SLOT_CURRENT, image, 0)[0].tobytes() == cc.expected(c["name"], image)["dst"].tobytes()
    f.close()


def test_argument_checks():
    lib = clahe.load()
    assert lib.visfs_clahe_abi_version() == clahe.ABI_VERSION == 1
    p = clahe.default_params()
    assert (p.clip_limit, p.tiles_x, p.tiles_y) == (3.0, 8, 8)
    c = cc.case("texture_64x48_c3_t8x8")
    f = _flow(64, 48)
    with pytest.raises(backend.BackendError):
        clahe.download(f)                                                            # nothing pushed yet
    assert lib.visfs_flow_clahe_download(f.h, 0, None, None) == abi.ERR_NOT_LOADED
    push = lambda prm: clahe.push_frame_status(f, prm, c["left"], c["right"])
    assert push(None) == abi.ERR_BAD_ARGUMENT
    for bad in (dict(clip_limit=float("nan")), dict(clip_limit=float("inf")), dict(clip_limit=-1.0), dict(tiles_x=0), dict(tiles_y=-3)):
        assert push(clahe.default_params(**bad)) == abi.ERR_BAD_ARGUMENT, bad
        assert clahe.hook_geometry_status(clahe.default_params(**bad), 64, 48)[0] == abi.ERR_BAD_ARGUMENT
    for bad in (dict(tiles_x=33), dict(tiles_y=33), dict(tiles_x=32, tiles_y=48)):
        assert push(clahe.default_params(**bad)) == abi.ERR_UNSUPPORTED, bad
    assert clahe.hook_geometry_status(clahe.default_params(tiles_x=8), 8, 48)[0] == abi.ERR_UNSUPPORTED        # width <= tiles_x
    assert clahe.hook_geometry_status(clahe.default_params(tiles_y=8), 64, 8)[0] == abi.ERR_UNSUPPORTED
    assert clahe.hook_geometry_status(clahe.default_params(), 9, 9)[0] == abi.OK
    assert clahe.hook_geometry_status(None, 64, 48)[0] == abi.ERR_BAD_ARGUMENT
    assert lib.visfs_flow_push_frame_clahe(f.h, clahe.default_params(), c["left"].ctypes.data_as(clahe._pu8),
                                           c["right"].ctypes.data_as(clahe._pu8), 63) == abi.ERR_BAD_ARGUMENT
    assert lib.visfs_flow_push_frame_clahe(f.h, clahe.default_params(), None, c["right"].ctypes.data_as(clahe._pu8), 64) == abi.ERR_BAD_ARGUMENT
    with pytest.raises(backend.BackendError):
        f.download_level(flow.SLOT_CURRENT, 0, 0)                                    # no refused call pushed a frame
    assert push(clahe.default_params(tiles_x=32, tiles_y=32)) == abi.OK              # the largest table; 2 x 1 + 1 pixels a tile
    assert clahe.download(f)["lut"].shape == (32, 32, 256)
    assert clahe.hook_geometry(clahe.default_params(clip_limit=1e300), 64, 48)["clip"] == 2 ** 31 - 1
    f.close()
