"""An independent pure-Python restatement of the reference's 2-D laser sub-maps (corelib Map/2d), for the parity tests.

It follows the reference's own control flow (RayToPixelMask.cpp's stepping loop, ProbabilityGrid::applyLookUpTable with
update markers, Grid2D::growLimits, ActiveSubmaps2D::insertRangeData), not the per-column closed form the library runs.
Python floats are IEEE doubles and every expression below is formed in the reference's order, so the values are the
reference's bit for bit.
"""
import math

K_SUBPIXEL_SCALE = 1000
K_UPDATE_MARKER = 1 << 15
K_MIN_PROBABILITY = 0.1
K_MAX_PROBABILITY = 1.0 - K_MIN_PROBABILITY
K_MIN_CC = 1.0 - K_MAX_PROBABILITY
K_MAX_CC = 1.0 - K_MIN_PROBABILITY


def lround(v):
    """std::lround: nearest integer, halves away from zero."""
    f = math.floor(v)
    d = v - f
    if d > 0.5 or (d == 0.5 and v > 0):
        return int(f) + 1
    return int(f)


def cdiv(a, b):
    """C++ integer division (truncation toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def cmod(a, b):
    return a - b * cdiv(a, b)


# ---------------------------------------------------------------- values (ProbabilityValues.h/.cpp)
def clamp(v, lo, hi):
    if v > hi:
        return hi
    if v < lo:
        return lo
    return v


def bounded_to_value(v, lo, hi):
    return lround((clamp(v, lo, hi) - lo) * (32766.0 / (hi - lo))) + 1


def value_to_bounded(value, unknown, lo, hi):
    if value == 0:
        return unknown
    k = (hi - lo) / 32766.0
    return value * k + (lo - k)


def odds(p):
    return p / (1.0 - p)


def prob_from_odds(o):
    return o / (o + 1.0)


def value_to_cost(v):
    return value_to_bounded(v & (K_UPDATE_MARKER - 1), K_MAX_CC, K_MIN_CC, K_MAX_CC)


def value_to_probability(v):
    return value_to_bounded(v & (K_UPDATE_MARKER - 1), K_MIN_PROBABILITY, K_MIN_PROBABILITY, K_MAX_PROBABILITY)


def cost_to_value(c):
    return bounded_to_value(c, K_MIN_CC, K_MAX_CC)


def probability_to_value(p):
    return bounded_to_value(p, K_MIN_PROBABILITY, K_MAX_PROBABILITY)


def odds_table(o):
    """computeLookupTableToApplyCorrespondenceCostOdds."""
    t = [cost_to_value(1.0 - prob_from_odds(o)) + K_UPDATE_MARKER]
    for v in range(1, 32768):
        t.append(cost_to_value(1.0 - prob_from_odds(o * odds(1.0 - value_to_cost(v)))) + K_UPDATE_MARKER)
    return t


def crop_value(v):
    """setProbability(getProbability(cell)) of a known cell."""
    return cost_to_value(1.0 - (1.0 - value_to_cost(v)))


# ---------------------------------------------------------------- rayToPixelMask, stepped as the reference steps
def ray_to_pixel_mask(b, e, s):
    bx, by = b
    ex, ey = e
    if bx > ex:
        return ray_to_pixel_mask(e, b, s)
    out = []

    def push(c):
        if not out or out[-1] != c:
            out.append(c)
    if cdiv(bx, s) == cdiv(ex, s):
        x = cdiv(bx, s)
        y = cdiv(min(by, ey), s)
        out.append((x, y))
        end_y = cdiv(max(by, ey), s)
        while y <= end_y:
            push((x, y))
            y += 1
        return out
    dx = ex - bx
    dy = ey - by
    den = 2 * s * dx
    cx, cy = cdiv(bx, s), cdiv(by, s)
    out.append((cx, cy))
    sub_y = (2 * cmod(by, s) + 1) * dx
    first = 2 * s - 2 * cmod(bx, s) - 1
    last = 2 * cmod(ex, s) + 1
    end_x = cdiv(max(bx, ex), s)
    sub_y += dy * first
    if dy > 0:
        while True:
            push((cx, cy))
            while sub_y > den:
                sub_y -= den
                cy += 1
                push((cx, cy))
            cx += 1
            if sub_y == den:
                sub_y -= den
                cy += 1
            if cx == end_x:
                break
            sub_y += dy * 2 * s
        sub_y += dy * last
        push((cx, cy))
        while sub_y > den:
            sub_y -= den
            cy += 1
            push((cx, cy))
        return out
    while True:
        push((cx, cy))
        while sub_y < 0:
            sub_y += den
            cy -= 1
            push((cx, cy))
        cx += 1
        if sub_y == 0:
            sub_y += den
            cy -= 1
        if cx == end_x:
            break
        sub_y += dy * 2 * s
    sub_y += dy * last
    push((cx, cy))
    while sub_y < 0:
        sub_y += den
        cy -= 1
        push((cx, cy))
    return out


# ---------------------------------------------------------------- grid
def cell_index(res, mx, my, px, py):
    return (lround((my - py) / res - 0.5), lround((mx - px) / res - 0.5))


class Grid:
    def __init__(self, res, mx, my, nx, ny):
        self.res, self.max_x, self.max_y, self.nx, self.ny = res, mx, my, nx, ny
        self.cells = [0] * (nx * ny)
        self.box = None          # (min_x, min_y, max_x, max_y)
        self.upd = []

    def contains(self, x, y):
        return 0 <= x < self.nx and 0 <= y < self.ny

    def extend(self, x, y):
        if self.box is None:
            self.box = (x, y, x, y)
        else:
            a, b, c, d = self.box
            self.box = (min(a, x), min(b, y), max(c, x), max(d, y))

    def grow_limits(self, px, py):
        while not self.contains(*cell_index(self.res, self.max_x, self.max_y, px, py)):
            xo, yo = self.nx // 2, self.ny // 2
            nmx, nmy = self.max_x + self.res * yo, self.max_y + self.res * xo
            nnx, nny = 2 * self.nx, 2 * self.ny
            new = [0] * (nnx * nny)
            for i in range(self.ny):
                new[xo + (i + yo) * nnx: xo + (i + yo) * nnx + self.nx] = self.cells[i * self.nx:(i + 1) * self.nx]
            self.cells, self.max_x, self.max_y, self.nx, self.ny = new, nmx, nmy, nnx, nny
            if self.box is not None:
                a, b, c, d = self.box
                self.box = (a + xo, b + yo, c + xo, d + yo)

    def apply(self, x, y, table):
        i = self.nx * y + x
        if self.cells[i] >= K_UPDATE_MARKER:
            return False
        self.upd.append(i)
        self.cells[i] = table[self.cells[i]]
        self.extend(x, y)
        return True

    def finish_update(self):
        for i in self.upd:
            self.cells[i] -= K_UPDATE_MARKER
        self.upd = []

    def set_probability(self, x, y, p):
        i = self.nx * y + x
        assert self.cells[i] == 0
        self.cells[i] = cost_to_value(1.0 - p)
        self.extend(x, y)

    def get_probability(self, x, y):
        if not self.contains(x, y):
            return K_MIN_PROBABILITY
        return 1.0 - value_to_cost(self.cells[self.nx * y + x])

    def cropped(self):
        if self.box is None:
            off, cx, cy = (0, 0), 1, 1
        else:
            off = (self.box[0], self.box[1])
            cx, cy = self.box[2] - self.box[0] + 1, self.box[3] - self.box[1] + 1
        g = Grid(self.res, self.max_x - self.res * off[1], self.max_y - self.res * off[0], cx, cy)
        for y in range(cy):
            for x in range(cx):
                sx, sy = x + off[0], y + off[1]
                if self.contains(sx, sy) and self.cells[self.nx * sy + sx] != 0:
                    g.set_probability(x, y, self.get_probability(sx, sy))
        return g, off


def transform_xy(T, p):
    return (((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3], ((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7])


def insert(grid, origin, returns, misses, hit, miss):
    """ProbabilityGridRangeDataInserter2D::insert of one range data already in the map frame (xy pairs)."""
    xs = [origin[0]] + [p[0] for p in returns] + [p[0] for p in misses]
    ys = [origin[1]] + [p[1] for p in returns] + [p[1] for p in misses]
    grid.grow_limits(min(xs) - 1e-6, min(ys) - 1e-6)
    grid.grow_limits(max(xs) + 1e-6, max(ys) + 1e-6)
    sres = grid.res / K_SUBPIXEL_SCALE
    begin = cell_index(sres, grid.max_x, grid.max_y, *origin)
    ends = []
    for p in returns:
        ends.append(cell_index(sres, grid.max_x, grid.max_y, *p))
        grid.apply(cdiv(ends[-1][0], K_SUBPIXEL_SCALE), cdiv(ends[-1][1], K_SUBPIXEL_SCALE), hit)
    for e in ends:
        for c in ray_to_pixel_mask(begin, e, K_SUBPIXEL_SCALE):
            grid.apply(c[0], c[1], miss)
    for p in misses:
        e = cell_index(sres, grid.max_x, grid.max_y, *p)
        for c in ray_to_pixel_mask(begin, e, K_SUBPIXEL_SCALE):
            grid.apply(c[0], c[1], miss)
    grid.finish_update()


class Submaps:
    """ActiveSubmaps2D (probability grids)."""

    def __init__(self, limit=50, res=0.05, p_hit=0.55, p_miss=0.49):
        self.limit, self.res = limit, res
        self.hit, self.miss = odds_table(odds(p_hit)), odds_table(odds(p_miss))
        self.subs = []           # [grid, count, finished]

    def insert_range_data(self, T, origin, returns, misses):
        if not self.subs or self.subs[-1][1] == self.limit:
            if len(self.subs) >= 2:
                assert self.subs[0][2]
                self.subs.pop(0)
            h = 0.5 * 100 * self.res
            self.subs.append([Grid(self.res, T[3] + h, T[7] + h, 100, 100), 0, False])
        o = transform_xy(T, origin)
        r = [transform_xy(T, p) for p in returns]
        m = [transform_xy(T, p) for p in misses]
        for s in self.subs:
            insert(s[0], o, r, m, self.hit, self.miss)
            s[1] += 1
        if self.subs[0][1] == 2 * self.limit:
            self.subs[0][0] = self.subs[0][0].cropped()[0]
            self.subs[0][2] = True
