"""Sub-map insertion at its batch, chunk and growth edges, host side (no GPU): the twin (visfs_submaps_create_host) against
the checker (tests/submap_oracle.py) on every case of tests/submap_cases.py after every call, the answers known without code,
the refusals that leave state behind, and the mark kernel's work items enumerated on the CPU."""
import numpy as np
import pytest

import submap_cases as sc
import submap_oracle as so
from test_submap_host import _compare, _segments
from visfs_amd import abi
from visfs_amd import submap as sm

CASES = sc.cases()
S = so.K_SUBPIXEL_SCALE


def checker_for(params):
    return so.Submaps(limit=params.get("num_range_data_limit", 50), res=params.get("map_resolution", 0.05),
                      p_hit=params.get("hit_probability", 0.55), p_miss=params.get("miss_probability", 0.49))


def checker_insert(py_maps, T, rds):
    for o, ret, mis in rds:
        py_maps.insert_range_data(list(T), o, ret.tolist(), mis.tolist())


_tables = {}


def tables(params):
    """(H, M): the hit and miss tables of the case without the update marker."""
    key = (params.get("hit_probability", 0.55), params.get("miss_probability", 0.49))
    if key not in _tables:
        _tables[key] = tuple(sm.hook_odds_table(so.odds(p)).astype(np.int64) - so.K_UPDATE_MARKER for p in key)
    return _tables[key]


def cell_of(info, point):
    """The cell an inserter working on limits `info` puts `point` (map frame) into: its superscaled index / 1000."""
    ix, iy = so.cell_index(info["resolution"] / S, info["max_x"], info["max_y"], *point)
    return so.cdiv(ix, S), so.cdiv(iy, S)


def check_known(case, maps):
    """The case's `known`, `fixed` and (last) `sizes` on a library object (twin or device) after the last call.  The poses of
    the cases that carry them are the identity, so a point of the robot frame is a point of the map."""
    H, M = tables(case["params"])
    d = maps.describe()
    if case["sizes"] is not None:
        assert [x["num_x_cells"] for x in d] == [x["num_y_cells"] for x in d] == case["sizes"][-1]
    if not (case["known"] or case["fixed"]):
        return
    cells, _ = maps.download(0)
    for point, seq in case["known"]:
        v = 0
        for ch in seq:
            v = int((H if ch == "H" else M)[v])
        x, y = cell_of(d[0], point)
        assert int(cells[y, x]) == v, (point, seq)
    for point, which in case["fixed"]:
        x, y = cell_of(d[0], point)
        v = int(cells[y, x])
        assert v != 0 and int((H if which == "H" else M)[v]) == v, (point, which, v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_equals_the_checker_after_every_call(case):
    lib_maps = sm.Submaps(sm.default_params(**case["params"]))
    py_maps = checker_for(case["params"])
    for k, (T, rds) in enumerate(case["calls"]):
        assert lib_maps.insert(T, rds) == abi.OK, lib_maps.last_error()
        checker_insert(py_maps, T, rds)
        _compare(lib_maps, py_maps)
        if case["sizes"] is not None:
            assert [g.nx for g, _, _ in py_maps.subs] == case["sizes"][k]
    check_known(case, lib_maps)
    lib_maps.close()


def test_the_cases_reach_the_edges_they_are_built_for():
    """Conditions on the cases, read from the checker alone."""
    by = {c["name"]: c for c in CASES}
    assert len(by) == len(CASES)
    # growth inside a batch: 100 -> 200 after rd1, 200 -> 400 after rd3; the far returns fix the known box along y
    T, rds = by["growth_in_batch"]["calls"][0]
    py = so.Submaps()
    sizes = []
    for o, ret, mis in rds:
        py.insert_range_data(list(T), o, ret.tolist(), mis.tolist())
        sizes.append(py.subs[0][0].nx)
    assert sizes == [100, 200, 200, 400, 400, 400]
    box = py.subs[0][0].box
    assert (box[1], box[3]) == (120, 380) and 150 <= box[0] < box[2] <= 249
    # limit 2: the first range data of the second call adds a sub-map and grows it and the old one
    c = by["growth_new_and_old_limit2"]
    py = checker_for(c["params"])
    checker_insert(py, *c["calls"][0])
    assert [(g.nx, n) for g, n, _ in py.subs] == [(100, 2)]
    T, rds = c["calls"][1]
    checker_insert(py, T, rds[:1])
    assert [(g.nx, n) for g, n, _ in py.subs] == [(200, 3), (200, 1)]
    checker_insert(py, T, rds[1:2])                                                             # both grown again; the front finished
    assert py.subs[0][1:] == [4, True] and [(g.nx, n, f) for g, n, f in py.subs[1:]] == [(400, 2, False)]
    checker_insert(py, T, rds[2:3])                                                             # a sub-map added, the front dropped
    assert [(g.nx, n, f) for g, n, f in py.subs] == [(400, 3, False), (100, 1, False)]
    checker_insert(py, T, rds[3:4])                                                             # the new one grown alone
    assert py.subs[0][1:] == [4, True] and [(g.nx, n, f) for g, n, f in py.subs[1:]] == [(400, 2, False)]
    # limit 1, five range data: a sub-map added at every insertion, the front finished at 2 and dropped at the next add
    c = by["life_limit1_five"]
    py = checker_for(c["params"])
    T, rds = c["calls"][0]
    for k, (o, ret, mis) in enumerate(rds):
        py.insert_range_data(list(T), o, ret.tolist(), mis.tolist())
        assert [(n, f) for _, n, f in py.subs] == ([(1, False)] if k == 0 else [(2, True), (1, False)])
    # limit 1, two empty range data: the front finishes with an empty known box and crops to one unknown cell
    c = by["life_limit1_two_empty"]
    py = checker_for(c["params"])
    checker_insert(py, *c["calls"][0])
    g = py.subs[0][0]
    assert py.subs[0][2] and (g.nx, g.ny, g.cells, g.box) == (1, 1, [0], None)
    # saturation: 33 insertions do not reach the miss clamp, 65 do
    H, M = tables({})
    v33 = v65 = 0
    for k in range(65):
        v65 = int(M[v65])
        v33 = v65 if k == 32 else v33
    assert int(M[v33]) != v33 and int(M[v65]) == v65


# ---------------------------------------------------------------- refusals that leave state behind
def check_too_far(maps, compare_to, reference):
    """The call refused at its second range data: the first is inserted and the third is not; the object takes a later call.
    `reference` is fed the first range data alone, then the later call."""
    (T0, first), (T1, later) = sc.refusal_too_far()
    assert maps.insert(T0, first) == abi.ERR_UNSUPPORTED
    assert "2^28" in maps.last_error()
    reference(T0, first[:1])
    compare_to()
    assert maps.describe()[0]["num_range_data"] == 1
    assert maps.insert(T1, later) == abi.OK
    reference(T1, later)
    compare_to()
    assert maps.describe()[0]["num_range_data"] == 3 and maps.describe()[0]["num_x_cells"] == 200


def check_not_finite(maps, snapshot):
    (T0, good), (T1, bad) = sc.refusal_not_finite()
    assert maps.insert(T0, good) == abi.OK
    before = snapshot()
    assert maps.insert(T1, bad) == abi.ERR_BAD_ARGUMENT
    assert "finite" in maps.last_error()
    after = snapshot()
    assert before[0] == after[0] and len(before[0]) == 1 and before[0][0]["num_range_data"] == 2
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1]))


def snapshot_of(maps):
    d = maps.describe()
    return d, [a for i in range(len(d)) for a in maps.download(i)]


def test_growth_beyond_the_cell_limit_is_refused_after_the_first_range_data():
    lib_maps = sm.Submaps(sm.default_params())
    py_maps = so.Submaps()
    check_too_far(lib_maps, lambda: _compare(lib_maps, py_maps), lambda T, rds: checker_insert(py_maps, T, rds))
    lib_maps.close()


def test_a_return_that_is_not_finite_changes_nothing():
    lib_maps = sm.Submaps(sm.default_params())
    check_not_finite(lib_maps, lambda: snapshot_of(lib_maps))
    lib_maps.close()


# ---------------------------------------------------------------- the mark kernel's work items
def item_segments():
    return _segments(12000, 11) + sc.chunk_segments() + sc.STEEP_SEGMENTS


def test_mark_items_enumerate_every_cell_once_in_order():
    """The (column, chunk) items of a ray's record, sized as a batch sizes them, hold rayToPixelMask's cells as a list: every
    cell once, none dropped past the last chunk, columns in order."""
    for b, e in item_segments():
        cells, _ = sm.hook_mark_items(b, e)
        assert cells == so.ray_to_pixel_mask(b, e, S), (b, e)


def test_mark_items_are_bounded_by_the_rays_y_extent():
    """A column's cells lie in the ray's own y range, so no ray needs more than columns x ceil((|ey/S - by/S| + 1) / 8) items.
    The slope bound alone (|dy| / dx + 2 cells a column) sized the first steep ray of submap_cases at 2 x 8 251 items for
    two columns of 34 cells, and 57 of the 12 021 rays here broke this bound; with the y extent that ray takes 2 x 9."""
    for b, e in item_segments():
        _, items = sm.hook_mark_items(b, e)
        columns = abs(so.cdiv(e[0], S) - so.cdiv(b[0], S)) + 1
        extent = abs(so.cdiv(e[1], S) - so.cdiv(b[1], S)) + 1
        assert items <= columns * ((extent + 7) // 8), (b, e, items, columns, extent)
    b, e = sc.STEEP_SEGMENTS[0]
    assert sc.column_spans(b, e) == [34, 34]
    assert sm.hook_mark_items(b, e)[1] == 2 * 9
