"""Laser sub-maps, host side (no GPU): the library's tables, per-column ray work items and whole-insertion restatement
against the reference's own unit-test vectors (tests/golden/ref_map2d_*.json) and an independent Python restatement
(tests/submap_oracle.py)."""
import json
import math
import os
import random

import numpy as np
import pytest

import submap_oracle as so
from visfs_amd import abi
from visfs_amd import submap as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def close(a, b, pct):
    """BOOST_CHECK_CLOSE: relative difference to both values within pct percent."""
    d = abs(a - b)
    return d <= abs(a) * pct / 100.0 and d <= abs(b) * pct / 100.0


@pytest.fixture(scope="module")
def tables():
    cost, crop = sm.hook_value_tables()
    return dict(cost=cost, crop=crop, hit=sm.hook_odds_table(so.odds(0.55)), miss=sm.hook_odds_table(so.odds(0.49)))


def test_abi_version():
    assert sm.load().visfs_submap_abi_version() == sm.ABI_VERSION == 1
    p = sm.default_params()
    assert (p.num_range_data_limit, p.grid_map_type, p.map_resolution, p.insert_free_space, p.hit_probability, p.miss_probability) == \
        (50, 0, 0.05, 1, 0.55, 0.49)


# ---------------------------------------------------------------- tables
def test_tables_equal_the_python_restatement(tables):
    for p, t in ((0.55, tables["hit"]), (0.49, tables["miss"]), (0.9, sm.hook_odds_table(so.odds(0.9)))):
        assert [int(v) for v in t] == so.odds_table(so.odds(p))
    assert all(v >= so.K_UPDATE_MARKER for v in tables["hit"])
    assert [float(v) for v in tables["cost"]] == [so.value_to_cost(v) for v in range(32768)]
    assert tables["cost"][0] == so.K_MAX_CC
    assert [int(v) for v in tables["crop"]] == [0] + [so.crop_value(v) for v in range(1, 32768)]


def test_reference_value_checks(tables):
    fx = json.load(open(os.path.join(GOLDEN, "ref_map2d_probability.json")))
    c = fx["odds_conversions"]
    for p in c["probabilities"]:
        assert close(so.prob_from_odds(so.odds(p)), p, c["tol_percent"])
    c = fx["odds_conversions_cost"]
    for cc in c["costs"]:
        assert close(1.0 - so.prob_from_odds(so.odds(1.0 - cc)), cc, c["tol_percent"])
    c = fx["conversion_lookup_table"]
    assert close(so.value_to_probability(0), 1.0 - tables["cost"][0], c["tol_percent"])
    for i in range(1, 32768):
        assert close(so.value_to_probability(i), tables["cost"][i], c["tol_percent"])
    # CellUpdate / MultipleCellUpdate: the library's correspondence-cost tables against the probability-form table
    def ptab(o, v):                                         # computeLookupTableToApplyOdds(o)[v]
        q = so.prob_from_odds(o) if v == 0 else so.prob_from_odds(o * so.odds(so.value_to_probability(v)))
        return so.probability_to_value(q) + so.K_UPDATE_MARKER
    c = fx["cell_update"]
    o = so.odds(c["odds_probability"])
    ct = sm.hook_odds_table(o)
    assert close(so.value_to_probability(ptab(o, 0)), 1.0 - tables["cost"][ct[0] & 0x7FFF], c["tol_percent_first"])
    for i in range(c["evaluations"]):
        p = (i / c["evaluations"]) * (so.K_MAX_PROBABILITY - so.K_MIN_PROBABILITY) + so.K_MIN_PROBABILITY
        pv, cv = so.probability_to_value(p), so.cost_to_value(1.0 - p)
        assert abs(pv - (32768 - cv)) <= 1            # (off by one where 1 - p rounds: the reference check logs those)
        assert close(so.value_to_probability(ptab(o, pv)), 1.0 - tables["cost"][ct[cv] & 0x7FFF], c["tol_percent"]), i
    c = fx["multiple_cell_update"]
    o = so.odds(c["odds_probability"])
    ct = sm.hook_odds_table(o)
    for i in range(c["evaluations"]):
        p = (i / c["evaluations"]) * (so.K_MAX_PROBABILITY - so.K_MIN_PROBABILITY) + so.K_MIN_PROBABILITY
        pv = so.probability_to_value(p) + so.K_UPDATE_MARKER
        cv = so.cost_to_value(1.0 - p) + so.K_UPDATE_MARKER
        for _ in range(c["updates"]):
            pv = ptab(o, pv - so.K_UPDATE_MARKER)
            cv = int(ct[cv - so.K_UPDATE_MARKER])
        assert close(so.value_to_probability(pv), 1.0 - tables["cost"][cv & 0x7FFF], c["tol_percent"]), i


def test_apply_odds_and_get_probability(tables):
    fx = json.load(open(os.path.join(GOLDEN, "ref_map2d_probability.json")))
    a = fx["apply_odds"]
    g = so.Grid(a["resolution"], *a["max"], a["num_x_cells"], a["num_y_cells"])
    for st in a["steps"]:
        x, y = st["cell"]
        if st["op"] == "set":
            g.set_probability(x, y, st["p"])
        else:
            g.apply(x, y, [int(v) for v in sm.hook_odds_table(so.odds(st["odds_p"]))])
            if st.get("finish"):
                g.finish_update()
        p = 1.0 - tables["cost"][g.cells[g.nx * y + x] & 0x7FFF]          # getProbability through the library's table
        if "expect_eq" in st:
            assert p == st["expect_eq"]
        if "expect_gt" in st:
            assert p > st["expect_gt"]
        if "expect_lt" in st:
            assert p < st["expect_lt"]
        if "expect_close" in st:
            assert close(p, st["expect_close"], st["tol_percent"] * 100)   # (BOOST_CHECK_CLOSE 1e-2 %: the table's step is 2.4e-5)
    gp = fx["get_probability"]
    g = so.Grid(gp["resolution"], *gp["max"], gp["num_x_cells"], gp["num_y_cells"])
    c = so.cell_index(g.res, g.max_x, g.max_y, *gp["set_point"])
    g.set_probability(*c, gp["set_p"])
    assert close(1.0 - tables["cost"][g.cells[g.nx * c[1] + c[0]]], gp["set_p"], gp["tol_percent"])
    for pt in gp["unknown_points"]:
        x, y = so.cell_index(g.res, g.max_x, g.max_y, *pt)
        assert g.contains(x, y) and g.cells[g.nx * y + x] == 0


def test_correct_cropping():
    c = json.load(open(os.path.join(GOLDEN, "ref_map2d_probability.json")))["correct_cropping"]
    rng = random.Random(5)
    g = so.Grid(c["resolution"], *c["max"], c["num_x_cells"], c["num_y_cells"])
    (x0, y0), (x1, y1) = c["known_min"], c["known_max"]
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            g.set_probability(x, y, rng.uniform(*c["p_range"]))
    cells = np.array(g.cells, dtype=np.uint16).reshape(g.ny, g.nx)
    off, out, box = sm.hook_crop(cells, g.box)
    assert list(off) == c["expected_offset"] and [out.shape[1], out.shape[0]] == c["expected_cells"]
    gc, off2 = g.cropped()
    assert off2 == off and np.array_equal(out, np.array(gc.cells, dtype=np.uint16).reshape(gc.ny, gc.nx))
    assert box == gc.box == (0, 0, c["expected_cells"][0] - 1, c["expected_cells"][1] - 1)
    # an empty grid crops to one unknown cell
    off, out, box = sm.hook_crop(np.zeros((4, 4), np.uint16), (1, 1, 0, 0))
    assert off == (0, 0) and out.shape == (1, 1) and out[0, 0] == 0 and box[0] > box[2]


# ---------------------------------------------------------------- rays
def test_ray_mask_reference_vectors():
    fx = json.load(open(os.path.join(GOLDEN, "ref_map2d_ray_mask.json")))
    for c in fx["cases"]:
        exp = [tuple(v) for v in c["expected"]]
        assert sm.hook_ray(c["begin"], c["end"], c["scale"]) == exp, c["source"]
        assert so.ray_to_pixel_mask(tuple(c["begin"]), tuple(c["end"]), c["scale"]) == exp, c["source"]
        if c.get("both_orders"):
            assert sm.hook_ray(c["end"], c["begin"], c["scale"]) == exp, c["source"]
    for c in fx["multiscale"]:
        exp = [tuple(v) for v in c["expected"]]
        for s in c["scales"]:
            res = c["resolution"] / s
            b = so.cell_index(res, *c["max"], *c["begin_point"])
            e = so.cell_index(res, *c["max"], *c["end_point"])
            assert sm.hook_ray(b, e, s) == exp, (c["source"], s)


def _segments(n, seed):
    rng = random.Random(seed)
    S = so.K_SUBPIXEL_SCALE
    out = []
    for i in range(n):
        kind = i % 8
        bx, by = rng.randrange(0, 40 * S), rng.randrange(0, 40 * S)
        if kind == 0:                                        # vertical: same column
            ex, ey = (bx // S) * S + rng.randrange(S), rng.randrange(0, 40 * S)
        elif kind == 1:                                      # horizontal: same row
            ex, ey = rng.randrange(0, 40 * S), (by // S) * S + rng.randrange(S)
        elif kind == 2:                                      # single cell
            ex, ey = (bx // S) * S + rng.randrange(S), (by // S) * S + rng.randrange(S)
        elif kind == 3:                                      # endpoints on cell borders
            bx, by = (bx // S) * S, (by // S) * S
            ex, ey = rng.randrange(0, 40) * S + rng.choice([0, S - 1]), rng.randrange(0, 40) * S + rng.choice([0, S - 1])
        elif kind == 4:                                      # exact diagonals
            d = rng.randrange(-10, 11) * S
            ex, ey = bx + abs(d), by + d
            if ey < 0:
                ey = by - d
        else:                                                # all octants, long and short
            L = rng.choice([2, 30, 600]) * S
            ang = rng.uniform(0, 2 * math.pi)
            ex, ey = int(bx + L * math.cos(ang)), int(by + L * math.sin(ang))
            ex, ey = max(ex, 0), max(ey, 0)
        out.append(((bx, by), (ex, ey)))
    return out


def test_ray_work_items_equal_the_stepping_restatement():
    for b, e in _segments(12000, 11):
        assert sm.hook_ray(b, e) == so.ray_to_pixel_mask(b, e, so.K_SUBPIXEL_SCALE), (b, e)


# ---------------------------------------------------------------- whole insertions
def _frames(n, seed, n_ret=12, n_miss=2, reach=4.0, with_empty=False):
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n):
        yaw = 0.3 * f
        c, s = math.cos(yaw), math.sin(yaw)
        T = [c, -s, 0.0, 0.2 * f, s, c, 0.0, -0.15 * f, 0.0, 0.0, 1.0, 0.0]
        rds = []
        for k in range(2):
            ang = rng.uniform(0, 2 * math.pi, n_ret)
            rad = rng.uniform(0.05, reach * (1 + f % 3), n_ret)
            ret = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n_ret)], -1)
            if n_ret >= 2:
                ret[1] = ret[0] + [1e-4, -1e-4, 0]                 # two returns in one cell
            ma = rng.uniform(0, 2 * math.pi, n_miss)
            mis = np.stack([6.0 * np.cos(ma), 6.0 * np.sin(ma), np.zeros(n_miss)], -1)
            o = [0.1 * k, 0.0, 0.0]
            if with_empty and f % 5 == 2 and k == 1:
                ret, mis = np.zeros((0, 3)), np.zeros((0, 3))
            rds.append((o, ret, mis))
        out.append((T, rds))
    return out


def _compare(lib_maps, py_maps):
    d = lib_maps.describe()
    assert len(d) == len(py_maps.subs)
    for i, (info, (g, count, fin)) in enumerate(zip(d, py_maps.subs)):
        assert (info["num_range_data"], bool(info["finished"])) == (count, fin)
        assert (info["resolution"], info["max_x"], info["max_y"], info["num_x_cells"], info["num_y_cells"]) == (g.res, g.max_x, g.max_y, g.nx, g.ny)
        box = (info["known_min_x"], info["known_min_y"], info["known_max_x"], info["known_max_y"])
        assert (box if box[0] <= box[2] else None) == g.box
        cells, cost = lib_maps.download(i)
        assert np.array_equal(cells.reshape(-1), np.array(g.cells, dtype=np.uint16))
        assert np.array_equal(cost.reshape(-1), np.array([so.value_to_cost(v) for v in g.cells], dtype=np.float32))


def test_host_insertion_equals_the_python_restatement():
    """Growth (returns up to 12 m from a 5 m grid), miss rays, returns in cells other rays cross, two returns in one cell,
    the add / finish / drop cycle (limit 3), empty range data."""
    lib_maps = sm.Submaps(sm.default_params(num_range_data_limit=3))
    py_maps = so.Submaps(limit=3)
    for T, rds in _frames(9, 3, with_empty=True):
        assert lib_maps.insert(T, rds) == abi.OK
        for o, ret, mis in rds:
            py_maps.insert_range_data(T, o, ret.tolist(), mis.tolist())
        _compare(lib_maps, py_maps)
    lib_maps.close()


def test_submap_range_data_count():
    c = json.load(open(os.path.join(GOLDEN, "ref_map2d_probability.json")))["submap_range_data_count"]
    m = sm.Submaps(sm.default_params(num_range_data_limit=c["limit"]))
    seen = []
    eye = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    for i in range(c["insertions"]):
        assert m.insert(eye, [([0, 0, 0], np.zeros((0, 3)), np.zeros((0, 3)))]) == abi.OK
        d = m.describe()
        if len(d) > 1:
            assert d[0]["num_range_data"] >= c["limit"]
        # a sub-map is identified by the insertion it was added at; its last state is what it ends with
        first = i + 1 - d[-1]["num_range_data"]
        seen = [s for s in seen if s[0] != first] + [(first, d[-1]["num_range_data"], d[-1]["finished"])]
        if len(d) == 2:
            first0 = i + 1 - d[0]["num_range_data"]
            seen = [s for s in seen if s[0] != first0] + [(first0, d[0]["num_range_data"], d[0]["finished"])]
    assert len(m.describe()) == c["expected_active"]
    fin = [s for s in seen if s[1] == c["expected_finished_count"]]
    unf = [s for s in seen if s[1] != c["expected_finished_count"]]
    assert len(fin) == len(seen) - 1 and all(s[2] for s in fin)
    assert len(unf) == c["expected_unfinished"] and unf[0][1] == c["expected_unfinished_count"]


def test_parameters_refused():
    with pytest.raises(Exception):
        sm.Submaps(sm.default_params(grid_map_type=1))
    p = sm.default_params(grid_map_type=1)
    import ctypes as C
    h = C.c_void_p()
    assert sm.load().visfs_submaps_create_host(C.byref(p), C.byref(h)) == abi.ERR_UNSUPPORTED
    p = sm.default_params(num_range_data_limit=0)
    assert sm.load().visfs_submaps_create_host(C.byref(p), C.byref(h)) == abi.ERR_BAD_ARGUMENT


def test_insert_free_space_has_no_effect():
    a = sm.Submaps(sm.default_params(insert_free_space=1, num_range_data_limit=4))
    b = sm.Submaps(sm.default_params(insert_free_space=0, num_range_data_limit=4))
    for T, rds in _frames(4, 8):
        assert a.insert(T, rds) == b.insert(T, rds) == abi.OK
    assert a.describe() == b.describe()
    for i in range(len(a.describe())):
        assert np.array_equal(a.download(i)[0], b.download(i)[0])
