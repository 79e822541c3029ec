"""What the scan refinement's tests share (CPU: host twin against the NumPy checker; GPU: device against twin), so both see the
same inputs: the smooth field of the accuracy test, and refinement cases on the scenes of tests/scan_match_cases.py.

A refinement case is a dict: `name`, `scene` (a scan_match_cases case: the insertions and the sub-map index), `on` ("stack": the
sub-map frozen; "live": the sub-map itself; "grid": a stack made from `grid` = (limits, cells), no scene), `initial` (x, y, yaw),
`target` (x, y), `points` [n][3] and `prm` (keywords of visfs_scan_refine_params).
"""
import math

import numpy as np

import scan_fast_cases as sfc
import scan_match_cases as smc

LANES = 256                                              # VISFS_SCAN_REFINE_LANES
RES = 0.05

# ---------------------------------------------------------------- the smooth field
HALF = (2.63, 1.87)                                      # half-sides of the rectangle, not cell-aligned
SIGMA = 1.5 * RES
FIELD_LIMITS = dict(resolution=RES, max_x=3.05, max_y=2.3, num_x_cells=92, num_y_cells=122)
FIELD_TRUTH = (0.31, -0.17, 0.4)


def cost_to_value(cost):
    """Grid2D's correspondenceCostToValue."""
    lo, hi = 1.0 - (1.0 - 0.1), 1.0 - 0.1
    return (np.rint((np.clip(cost, lo, hi) - lo) * (32766.0 / (hi - lo))) + 1).astype(np.uint16)


def smooth_field():
    """(limits, cells): probability 0.1 + 0.8 exp(-d^2 / (2 sigma^2)) of the distance d of a cell's centre to the rectangle's
    walls, as cell values.  The x index runs along -y and the y index along -x (MapLimits)."""
    L = FIELD_LIMITS
    X = L["max_x"] - (np.arange(L["num_y_cells"]) + 0.5) * RES
    Y = L["max_y"] - (np.arange(L["num_x_cells"]) + 0.5) * RES
    ax, ay = np.abs(X)[:, None], np.abs(Y)[None, :]
    dx, dy = ax - HALF[0], ay - HALF[1]
    inside = (dx <= 0) & (dy <= 0)
    d_in = np.minimum(-dx, -dy)
    d_out = np.hypot(np.maximum(dx, 0), np.maximum(dy, 0))
    d = np.where(inside, d_in, d_out)
    p = 0.1 + 0.8 * np.exp(-d * d / (2 * SIGMA * SIGMA))
    return dict(L), cost_to_value(1.0 - p)


def wall_scan(pose, n):
    """The exact hits on the rectangle's walls of n rays from `pose` (inside), in the robot frame [n][3]."""
    x, y, yaw = pose
    ang = (np.arange(n) + 0.5) / n * 2 * math.pi - math.pi
    cx, cy = np.cos(ang + yaw), np.sin(ang + yaw)
    with np.errstate(divide="ignore"):
        tx = np.where(cx > 0, (HALF[0] - x) / cx, (-HALF[0] - x) / cx)
        ty = np.where(cy > 0, (HALF[1] - y) / cy, (-HALF[1] - y) / cy)
    t = np.minimum(np.where(cx == 0, np.inf, tx), np.where(cy == 0, np.inf, ty))
    return np.stack([t * np.cos(ang), t * np.sin(ang), np.zeros(n)], -1)


FIELD_COUNTS = (7, 64, 360)
FIELD_STARTS = 20
FIELD_PRM = dict(occupied_space_weight=1.0, translation_weight=0.0, rotation_weight=0.0, function_tolerance=0.0)


def field_starts():
    """20 seeded starts within one cell and 0.01 rad of the truth."""
    rng = np.random.default_rng(90)
    off = rng.uniform(-1.0, 1.0, size=(FIELD_STARTS, 3)) * np.array([RES, RES, 0.01])
    return [tuple(np.array(FIELD_TRUTH) + o) for o in off]


# ---------------------------------------------------------------- refinement cases on the matchers' scenes
def _near(pose, dx=0.021, dy=-0.017, dyaw=0.004):
    return (pose[0] + dx, pose[1] + dy, pose[2] + dyaw)


def cases():
    base = smc.base_cases()
    edge = {c["name"]: c for c in smc.edge_cases()}
    rng = np.random.default_rng(91)
    out = []

    def add(name, scene, on="stack", **kw):
        c = dict(name=name, scene=scene, on=on, initial=_near(scene["truth"]), target=scene["truth"][:2], points=scene["points"], prm={})
        c.update(kw)
        out.append(c)

    # the pipeline's use: the start is a lattice pose near the truth, the target the guess
    for i, b in enumerate(base):
        lattice = (round(b["truth"][0] / RES) * RES, round(b["truth"][1] / RES + 0.5) * RES - RES / 2, b["truth"][2] + 0.003 * (i - 2))
        add(f"base{i}", b, initial=lattice, target=b["guess"][:2])
    add("n1_priors", base[0], points=smc.cast(smc.TRUTH, 1, rng))                          # the occupied-space system alone is singular
    for n in (LANES - 1, LANES, LANES + 1, 1025):
        add(f"n{n}", base[0], points=smc.cast(smc.TRUTH, n, rng))
    add("outside", edge["outside"], initial=edge["outside"]["guess"], target=edge["outside"]["guess"][:2])   # constant cost, zero gradient
    add("outside_free", edge["outside"], initial=edge["outside"]["guess"], target=edge["outside"]["guess"][:2],
        prm=dict(translation_weight=0.0, rotation_weight=0.0))                              # ... and a singular system: ten rejected trials
    add("grid_edge", edge["grid_edge"], initial=edge["grid_edge"]["guess"], target=edge["grid_edge"]["guess"][:2])   # 4 x 4 patches across the border
    add("after_growth_live", edge["after_growth"], on="live")                              # the allocation trails the limits on the device
    add("cropped_front_live", edge["cropped_front"], on="live")
    add("second_submap_live", edge["second_submap"], on="live")
    # (function_tolerance = 0 with 50 iterations on base1 runs into the noise floor, where the twin and a checker that sums in another
    # order accept different trials: replaced by twelve iterations on base4, which stop above it; DESIGN.md section 9o names it)
    add("no_tolerance", base[4], prm=dict(function_tolerance=0.0, max_iterations=12))
    add("occupied_only", base[3], prm=dict(translation_weight=0.0, rotation_weight=0.0, max_iterations=8))
    add("one_iteration", base[2], prm=dict(max_iterations=1))
    limits, cells = sfc.corner_grid()                                                      # random values, an update marker, known cells on the border
    pts = np.stack([rng.uniform(-0.6, 0.6, 40), rng.uniform(-0.5, 0.5, 40), np.zeros(40)], -1)
    out.append(dict(name="corner_grid", scene=None, on="grid", grid=(limits, cells), initial=(0.1, 0.05, 0.2), target=(0.12, 0.03), points=pts, prm={}))
    # returns on both sides of the grid's far and near borders, within two cells of them: their 4 x 4 patches straddle the border
    off = np.array([-0.12, -0.07, -0.02, 0.03, 0.07])
    xs = np.concatenate([limits["max_x"] + off, limits["max_x"] - 29 * RES - off, np.linspace(-0.3, 0.8, 5)])
    ys = np.concatenate([np.linspace(-0.9, 0.7, 5), np.linspace(-0.9, 0.7, 5), limits["max_y"] + off])
    out.append(dict(name="border", scene=None, on="grid", grid=(limits, cells), initial=(0.004, -0.003, 0.002), target=(0.0, 0.0),
                    points=np.stack([xs, ys, np.zeros(15)], -1), prm={}))
    return out


def same_refinement(a, b, ta=None, tb=None):
    """Two refinement records equal byte for byte (and their traces)."""
    assert a["bytes"] == b["bytes"], ({k: v for k, v in a.items() if k != "bytes"}, {k: v for k, v in b.items() if k != "bytes"})
    if ta is not None:
        assert ta.shape == tb.shape and ta.tobytes() == tb.tobytes()


class Opened:
    """A case's object of one flavour (solver: a backend.Solver for the device, None for the host twin): `refine(**kw)` runs the
    case (keywords override initial, target, points) and returns (status, record), `trace()` the hook's trials, `grid()` the
    (limits, cells) of what is refined against, as values."""

    def __init__(self, case, solver=None, subs=None):
        from visfs_amd import scan_fast as sf
        from visfs_amd import scan_refine as sr
        from visfs_amd import submap as sm
        self.case, self.sr, self.own = case, sr, []
        self.sub = self.stack = None
        if case["on"] == "grid":
            limits, cells = case["grid"]
            self.stack = sf.ScanStack.from_grid(cells, limits, 3, solver=solver)
            assert self.stack.status == 0
            self.own.append(self.stack)
            return
        scene = case["scene"]
        self.sub = subs
        if self.sub is None:
            self.sub = sm.Submaps(sm.default_params(num_range_data_limit=scene["limit"]), solver=solver)
            smc.fill(self.sub, scene)
            self.own.append(self.sub)
        if case["on"] == "stack":
            self.stack = self.sub.freeze(scene["index"], 3)
            assert self.stack.status == 0, self.sub.last_error()
            self.own.insert(0, self.stack)

    def refine(self, **kw):
        c = self.case
        a, t, p = kw.pop("initial", c["initial"]), kw.pop("target", c["target"]), kw.pop("points", c["points"])
        prm = dict(c["prm"]); prm.update(kw)
        if self.stack is not None:
            return self.stack.refine(a, t, p, **prm)
        return self.sub.refine(a, t, p, index=c["scene"]["index"], **prm)

    def trace(self):
        return self.sr.stack_trace(self.stack) if self.stack is not None else self.sr.submaps_trace(self.sub)

    def last_error(self):
        return (self.stack if self.stack is not None else self.sub).last_error()

    def grid(self):
        if self.case["on"] == "grid":
            limits, cells = self.case["grid"]
            return limits, np.asarray(cells) & 0x7FFF
        i = self.case["scene"]["index"]
        return self.sub.describe()[i], self.sub.download(i)[0]

    def close(self):
        for o in self.own:
            o.close()


def group_setting():
    """The group of the mixed test: members (the base stack, the base stack again, the cropped front), the scan of
    scan_fast_cases.overflow_case with its windows (nl = 1, S = 27, H = 2), and per member a guess: base guess 2 matches (score 0.589),
    the overflow case's own guess keeps every node and overflows at frontier_capacity 32, base guess 4 stays below min_score 0.5
    (score 0.381).  Returns (guesses, points, keywords of visfs_scan_stack_params)."""
    base = smc.base_cases()
    over = sfc.overflow_case()
    guesses = [base[2]["guess"], over["guess"], base[4]["guess"]]
    return guesses, over["points"], dict(linear_search_window=over["prm"][0], angular_search_window=over["prm"][1], frontier_capacity=32, min_score=0.5)
