"""What the scan stack group's tests share (CPU: host group against single calls and the checker; GPU: device group against the
host group and device single calls): the member sub-maps, the overflow settings and the comparisons."""
import scan_fast_cases as cases
from visfs_amd import abi
from visfs_amd import scan_fast as sf

BASE = cases.base_cases()
EDGE = {c["name"]: c for c in cases.edge_cases()}
MEMBERS = [BASE[0], EDGE["cropped_front"], EDGE["after_growth"]]          # 200 x 200, a cropped front, a grid frozen after growth


def on(member, search):
    """The search (guess, points, windows) of one case on the sub-map of another."""
    return dict(member, guess=search["guess"], points=search["points"], prm=search["prm"])


def single_call(st, guess, points, **kw):
    rc, r = st.match(guess, points, sf.default_params(**kw))
    return rc, r, (st.match_download() if rc == abi.OK else None)


def windows(case, **kw):
    return dict(linear_search_window=case["prm"][0], angular_search_window=case["prm"][1], **kw)


def argmax_lowest(results, status):
    best, top = -1, -1
    for i, (r, s) in enumerate(zip(results, status)):
        if s == abi.OK and r["matched"] == 1 and r["sum"] > top:
            best, top = i, r["sum"]
    return best


# The overflowing member is scan_fast_cases.overflow_case: nl = 1, L = 3, H = 2, S = 27, every read outside the grid, so all 27 top
# nodes, 108 nodes of level 1 and 243 leaves tie at 0 and are kept.  At capacity 8 the base members overflow as well (with these
# windows the base stack keeps [1, 5, 13] nodes at levels 0, 1, 2 from base guess 2 and [1, 12, 19] from base guess 0), so the
# capacity is the smallest power of two at which the single base call succeeds: 16 for guess 2 (the `outside` member then overflows
# at the top level, in the keep step) and 32 for guess 0 (it overflows at level 1, inside the level sweep).
OVERFLOWS = [(2, 16, 2), (0, 32, 1)]                     # (base guess, frontier_capacity, the level at which `outside` overflows)
