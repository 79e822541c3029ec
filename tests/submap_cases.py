"""The insertions the sub-map tests share (CPU: twin against checker, tests/test_submap_cases.py; GPU: device against twin,
tests/test_gpu_submap.py), all tiny and generated from fixed seeds.

A case is a dict: `name`, `params` (keywords over sm.default_params) and `calls`, a list of (Twr[12], [range data]) with one
entry per `insert` call; a range data is (origin[3], returns[n][3], misses[m][3]) in the robot frame.  Optional keys state what is
known about the case without running any code:
  `known`  [(world point (x, y), "HMH..")]: the cell of that point in sub-map 0 after the last call holds the tables applied to 0
           in that order (H: hit table, M: miss table, both without the update marker);
  `fixed`  [(world point, "H" | "M")]: that cell ends on a fixed point of the table;
  `sizes`  [[num_x_cells per sub-map] per call]: the grids' sizes after every call.

At resolution 0.05 the first grid is 100 x 100 cells, +-2.5 m about the pose; "near" points stay within 2 m of it, so they never
grow a grid.  The x index of a cell comes from world y and the y index from world x (MapLimits::getCellIndex), so a column of a ray
is a band of world y and rays along world x lie in one column."""
import math
from collections import Counter

import numpy as np

import submap_oracle as so

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
Y = 0.013                                   # a world y off every cell border
O = (0.012, Y)                              # the origin the crafted rays start from: cell (49, 49) of the first grid
EMPTY = ([0.0, 0.0, 0.0], np.zeros((0, 3)), np.zeros((0, 3)))


def pose(x, y, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return (c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, 0.0)


def xyz(points):
    p = np.zeros((len(points), 3))
    if len(points):
        p[:, :2] = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return p


def rd(origin, returns=(), misses=()):
    return ([float(origin[0]), float(origin[1]), 0.0], xyz(returns), xyz(misses))


def near(rng, n_ret=8, n_miss=1):
    """Returns between 0.2 m and 1.9 m of the pose and misses at 1.95 m, as [(x, y)] lists."""
    a = rng.uniform(0, 2 * math.pi, n_ret)
    r = rng.uniform(0.2, 1.9, n_ret)
    m = rng.uniform(0, 2 * math.pi, n_miss)
    return [(float(r[i] * math.cos(a[i])), float(r[i] * math.sin(a[i]))) for i in range(n_ret)], \
           [(1.95 * math.cos(float(v)), 1.95 * math.sin(float(v))) for v in m]


def near_rd(rng, origin=O, extra=(), n_ret=8, n_miss=1):
    ret, mis = near(rng, n_ret, n_miss)
    return rd(origin, ret + list(extra), mis)


# ---------------------------------------------------------------- rays in superscaled cells (the chunk case and the item test)

def segment(origin, point, res=0.05, max_xy=(2.5, 2.5)):
    """(begin, end) of the ray origin -> point in superscaled cells of the first grid about the identity pose."""
    sres = res / so.K_SUBPIXEL_SCALE
    return so.cell_index(sres, max_xy[0], max_xy[1], *origin), so.cell_index(sres, max_xy[0], max_xy[1], *point)


def column_spans(b, e):
    """Cells per column of rayToPixelMask(b, e), in column order."""
    c = Counter(x for x, _ in so.ray_to_pixel_mask(b, e, so.K_SUBPIXEL_SCALE))
    return [c[x] for x in sorted(c)]


CHUNK_SPANS = (8, 9, 16, 17, 25, 32)        # cells of the single column of the rays along world x
# near-vertical rays, both signs of dy in either order of the endpoints: two to four columns of tens of cells each
CHUNK_STEEP = [(1.9, Y + 0.06), (-1.9, Y + 0.06), (1.9, Y - 0.07), (-1.9, Y - 0.07), (1.7, Y - 0.0131), (-1.7, Y + 0.1)]


def chunk_returns():
    """Rays from O along world x (+x) of exactly CHUNK_SPANS cells in one column, and the steep ones."""
    return [(0.0125 + 0.05 * (n - 1), Y) for n in CHUNK_SPANS] + CHUNK_STEEP


def chunk_misses():
    """Miss points along -x: columns of exactly CHUNK_SPANS cells that end (in the column's order) on the ray's own end cell."""
    return [(0.0125 - 0.05 * (n - 1), Y) for n in CHUNK_SPANS]


def chunk_range_data():
    """The range data of the chunk case.  The first holds every crafted ray.  Within one insertion a cell is marked once however
    many rays cross it, and the rays along x are nested, so a cell lost from one ray's last chunk would be marked by a longer ray
    all the same: the others hold one ray each, every ray an insertion (a mark bit) of its own."""
    out = [rd(O, chunk_returns(), [(-1.9, Y), (-1.2, Y + 0.03)])]
    out += [rd(O, [p]) for p in chunk_returns()]
    out += [rd(O, [], [p]) for p in chunk_misses()]
    return out


def chunk_segments():
    """The rays of the chunk case as (begin, end) in superscaled cells; the spans the case is built for are asserted here."""
    segs = [segment(O, p) for p in chunk_returns()]
    back = [segment(O, p) for p in chunk_misses()]
    for n, (b, e), (b2, e2) in zip(CHUNK_SPANS, segs, back):
        assert column_spans(b, e) == column_spans(b2, e2) == [n], (n, column_spans(b, e), column_spans(b2, e2))
    steep = [column_spans(b, e) for b, e in segs[len(CHUNK_SPANS):]]
    assert all(2 <= len(s) <= 4 and max(s) >= 10 for s in steep), steep
    assert max(max(s) for s in steep) > 24, steep
    dys = [(e[1] - b[1]) * (1 if e[0] >= b[0] else -1) for b, e in segs[len(CHUNK_SPANS):]]
    assert min(dys) < 0 < max(dys)
    return segs + back


# Steep rays in superscaled cells that the slope bound of a column's span (|dy| / dx + 2) overestimates most: one column border
# crossed with dx of 1 to 3 sub-cells.  The first: dy = 66 001, its longer column holds 34 cells, the slope bound says 66 003.
STEEP_SEGMENTS = [
    ((20999, 500), (21000, 66501)),
    ((21000, 66501), (20999, 500)),
    ((20999, 66501), (21000, 500)),
    ((20998, 70000), (21001, 1)),
    ((5999, 999), (6000, 24000)),
    ((5999, 24000), (6001, 0)),
    ((999, 0), (1000, 8999)),
    ((999, 0), (1000, 9000)),
    ((1999, 8000), (2000, 0)),
]


# ---------------------------------------------------------------- the cases

def cases():
    out = []

    def add(name, calls, known=(), fixed=(), sizes=None, **params):
        out.append(dict(name=name, params=params, calls=calls, known=list(known), fixed=list(fixed), sizes=sizes))

    # batch sizes: n range data in one call from one pose, origins 0.01 k apart on the line y = Y.  Every range data holds a return
    # at (-1, Y), whose ray runs back along that line through the cell of O: that cell is crossed, never hit, by every insertion,
    # so bit 31 of one batch and bit 0 of the next meet in it.  65 range data are three batches (32 + 32 + 1): the limit of 100
    # keeps the life cycle (an added sub-map flushes the batch) out of these cases.
    for n in (1, 2, 31, 32, 33, 65):
        rng = np.random.default_rng(100 + n)
        rds = [near_rd(rng, origin=(O[0] + 0.01 * k, Y), extra=[(-1.0, Y)]) for k in range(n)]
        add(f"batch_{n}", [(IDENTITY, rds)], known=[(O, "M" * n)], sizes=[[100]], num_range_data_limit=100)

    # order inside a batch: the cell of (1, Y) is hit, crossed, hit and crossed in one insertion (the hit wins), crossed by a miss ray
    order = [rd(O, [(1.0, Y)]), rd(O, [(2.0, Y)]), rd(O, [(1.0, Y), (2.0, Y)]), rd(O, [], [(2.0, Y)])]
    add("order_one_call", [(IDENTITY, order)], known=[((1.0, Y), "HMHM"), ((2.0, Y), "HHM"), (O, "MMMM")])
    add("order_four_calls", [(IDENTITY, [r]) for r in order], known=[((1.0, Y), "HMHM"), ((2.0, Y), "HHM"), (O, "MMMM")])

    # saturation: 65 identical range data; the hit cell and a crossed cell end on the clamps of their tables
    same = rd(O, [(1.0, Y), (0.3, 1.2)], [(-1.5, -0.4)])
    add("saturation_65", [(IDENTITY, [same] * 65)], known=[((1.0, Y), "H" * 65), ((0.5, Y), "M" * 65)],
        fixed=[((1.0, Y), "H"), ((0.5, Y), "M")], num_range_data_limit=100)

    # growth inside a batch: 100 -> 200 after rd1, 200 -> 400 after rd3; records are staged before, between and after the two steps
    # (the far returns lie on cell borders, so which cell they fall in depends on the limits in force: not among the known cells)
    rng = np.random.default_rng(7)
    g = [near_rd(rng), near_rd(rng, extra=[(4.0, 0.3)]), near_rd(rng), near_rd(rng, extra=[(-9.0, -1.0)]), near_rd(rng), near_rd(rng)]
    add("growth_in_batch", [(IDENTITY, g)], sizes=[[400]], known=[(O, "M" * 6)])
    # ... and with a batch flushed at kMaxBatch between the two steps, from a turned pose
    rng = np.random.default_rng(8)
    g40 = [near_rd(rng, extra=[(4.0, 0.3)] if k == 20 else [(-9.0, -1.0)] if k == 35 else []) for k in range(40)]
    add("growth_across_batches_40", [(pose(0.3, -0.2, 0.7), g40)], sizes=[[400]])
    # limit 2 (a batch is at most two insertions): the first range data of call 2 adds a sub-map and grows it and the old one,
    # the second grows both again with the first one's records staged; the third adds and drops; the fourth grows the new
    # sub-map alone, 100 -> 400, with the third one's records staged
    rng = np.random.default_rng(9)
    add("growth_new_and_old_limit2",
        [(IDENTITY, [near_rd(rng), near_rd(rng)]),
         (pose(0.1, 0.05, 0.2), [near_rd(rng, extra=[(4.0, 0.3)]), near_rd(rng, extra=[(-9.0, -1.0)]), near_rd(rng),
                                 near_rd(rng, extra=[(0.3, 6.0)])])],
        num_range_data_limit=2)

    # chunks of a column: single columns of exactly 8, 9, 16, 17, 25 and 32 cells, and near-vertical rays
    chunk_segments()
    add("chunks", [(IDENTITY, chunk_range_data())], sizes=[[100]], num_range_data_limit=100,
        known=[(O, "M" * len(chunk_range_data())), (chunk_misses()[-1], "MM")])      # (the first one's miss ray crosses it too)

    # life cycle inside one call
    rng = np.random.default_rng(10)
    add("life_limit1_five", [(IDENTITY, [near_rd(rng) for _ in range(5)])], num_range_data_limit=1)
    add("life_limit2_seven", [(pose(-0.2, 0.1, -0.4), [near_rd(rng) for _ in range(7)])], num_range_data_limit=2)
    add("life_limit1_two_empty", [(IDENTITY, [EMPTY, EMPTY])], num_range_data_limit=1)
    add("life_limit1_empty_then_real", [(IDENTITY, [EMPTY, EMPTY, near_rd(rng), EMPTY, near_rd(rng)])], num_range_data_limit=1)
    add("zero_range_data", [(IDENTITY, []), (IDENTITY, [near_rd(rng)]), (pose(0.1, 0.0, 0.1), []), (pose(0.1, 0.0, 0.1), [near_rd(rng)])])
    add("empty_calls_between", [(IDENTITY, [near_rd(rng)]), (pose(0.2, 0.0, 0.1), [EMPTY]), (pose(0.3, 0.0, 0.2), [EMPTY, EMPTY]),
                                (pose(0.4, 0.1, 0.3), [near_rd(rng), near_rd(rng)]), (pose(0.5, 0.1, 0.3), [EMPTY]),
                                (pose(0.6, 0.1, 0.4), [near_rd(rng)])], num_range_data_limit=3)
    add("turned_poses_limit3", [(pose(0.3 * f, -0.2 * f, 0.9 * f), [near_rd(rng, extra=[(3.0, 0.5)] if f == 2 else []) for _ in range(3)])
                                for f in range(4)], num_range_data_limit=3)

    # degenerate rays
    add("return_is_origin", [(IDENTITY, [rd(O, [O, (1.0, 0.4)])])], known=[(O, "H")], sizes=[[100]])
    add("origin_and_return_in_one_cell", [(IDENTITY, [rd(O, [(O[0] + 0.02, Y + 0.02)])])], known=[(O, "H")], sizes=[[100]])
    add("two_returns_in_one_cell", [(IDENTITY, [rd(O, [(1.012, 0.512), (1.02, 0.52), (-0.7, 0.3)])])],
        known=[((1.012, 0.512), "H"), (O, "M")], sizes=[[100]])
    add("misses_only", [(IDENTITY, [rd(O, [], [(1.5, 0.7), (-1.2, -1.4), (0.4, -1.9)])])],
        known=[(O, "M"), ((1.5, 0.7), "M")], sizes=[[100]])
    edge = [(2.49, Y), (-2.49, Y), (Y, 2.49), (Y, -2.49), (2.49, 2.49), (-2.49, -2.49), (2.49, -2.49), (-2.49, 2.49)]
    add("last_cell_before_growth", [(IDENTITY, [rd(O, edge)])], known=[(p, "H") for p in edge], sizes=[[100]])
    add("first_cell_past_the_edge", [(IDENTITY, [rd(O, [(2.5, Y)])])], known=[((2.5, Y), "H")], sizes=[[200]])

    # other tables: resolution 0.1 (the first grid +-5 m), hit 0.7, miss 0.4, with growth and the life cycle
    rng = np.random.default_rng(11)
    add("other_tables", [(pose(0.2 * f, 0.1 * f, 0.5 * f), [near_rd(rng, extra=[(7.0, -1.0)] if f == 1 else []), near_rd(rng)])
                         for f in range(3)], num_range_data_limit=2, map_resolution=0.1, hit_probability=0.7, miss_probability=0.4)
    return out


# ---------------------------------------------------------------- refusals (tests of their own)

def refusal_too_far():
    """(first call: its second range data holds a return 1 000 m away, more than 2^28 cells at 0.05 m; a normal later call)."""
    rng = np.random.default_rng(12)
    first = [near_rd(rng), near_rd(rng, extra=[(1000.0, 0.0)]), near_rd(rng)]
    return (IDENTITY, first), (pose(0.1, 0.1, 0.3), [near_rd(rng), near_rd(rng, extra=[(3.5, 0.2)])])


def refusal_not_finite():
    """(a normal call; a call whose second range data holds a non-finite return)."""
    rng = np.random.default_rng(13)
    bad = near_rd(rng)
    bad[1][3, 1] = float("nan")
    return (IDENTITY, [near_rd(rng), near_rd(rng)]), (IDENTITY, [near_rd(rng), bad])
