"""Scenarios of the pose guess inside the resident tracker (include/visfs_tracker_pnp.h), shared by the host
and the device tests.  All are 320 x 240 (but the full-size one) with min_distance 12.  Everything is generated.  A scenario is one
of tracker_cases.py (or of tracker_cull_cases.py, with its `cull` entry) with a `pnp` entry: the keywords of pnp.default_params.

The counts asserted in assert_conditions are what the staged chain (the checker) gives on these scenes; they are conditions on
the scenario, looked at on the reference's own run, not targets for the code under test."""
import functools

import numpy as np

import group_cases as gc
import tracker_cases as tc
import tracker_cull_cases as cc
import tracker_oracle as to
import tracker_pnp_oracle as tpo
from visfs_amd import flow, pnp, tracker, tracker_pnp


def with_pnp(scn, **kw):
    scn = dict(scn)
    scn.setdefault("cull", None)
    scn["pnp"] = kw
    return scn


def pnp_params(scn):
    return pnp.default_params(**scn["pnp"])


def steady():
    return with_pnp(tc.scenario(tc.sequence(6), 60, 12))


def foreign(cull=0, **kw):
    kw.setdefault("iterations", 64)
    return with_pnp(cc.scenario(cc.foreign_sequence(), 60, 10, 64, cull=cull), **kw)


def tight():
    return with_pnp(tc.scenario(tc.sequence(5), 60, 12), reproj_error=0.15, iterations=64)


def too_few():
    return with_pnp(tc.scenario(tc.sequence(4), 60, 12), min_inliers=58)


def no_refine():
    return with_pnp(tc.scenario(tc.sequence(4), 60, 12), refine_iterations=0)


def nan_rows():
    return with_pnp(tc.bootstrap_nan())


def lost():
    return with_pnp(tc.lost_case())


def small(max_features):
    return with_pnp(tc.scenario(tc.sequence(4), max_features, 12, min_inliers=2), min_inliers=0, iterations=5)


def no_words():
    return with_pnp(tc.scenario(tc.sequence(5), 60, 12, max_depth=3.0), min_inliers=0)


def edge(max_features, iterations):
    return with_pnp(tc.scenario(tc.sequence(4), max_features, 12), iterations=iterations)


BIG_FEATURES, BIG_MIN_DISTANCE = 300, 20       # the most rows 752 x 480 gives with these is above one 256-row chunk of the refine stage


def big():
    return with_pnp(tc.scenario(tc.sequence(3, 752, 480), BIG_FEATURES, BIG_MIN_DISTANCE), iterations=256)


EDGE_FEATURES, EDGE_ITERATIONS = (63, 64, 65, 66, 67, 129), (5, 65)
CASES = {"steady": steady, "foreign": foreign, "foreign_cull": functools.partial(foreign, cull=1),
         "winner_below_min": functools.partial(foreign, min_inliers=50), "tight": tight, "too_few": too_few, "no_refine": no_refine,
         "nan_rows": nan_rows, "lost": lost, "m4": functools.partial(small, 4), "m3": functools.partial(small, 3), "no_words": no_words,
         "big": big}
for _mf in EDGE_FEATURES:
    for _it in EDGE_ITERATIONS:
        CASES[f"edge_mf{_mf}_it{_it}"] = functools.partial(edge, _mf, _it)


def tracker_params(scn):
    return cc.params(scn) if scn["cull"] is not None else tracker.default_params(clahe=1 if scn["clahe"] else 0, **scn["trk"])


class Subject:
    """A tracker.Tracker with the pose guess enabled (enable=False: never enabled) behind the checker's process() signature:
    result["pose"] is tracker_pnp.last, intermediates["pnp"] is tracker_pnp.download."""

    def __init__(self, scn, solver=None, enable=True):
        self.scn = scn
        self.flow = flow.Flow(flow.default_params(**scn["flow"]), scn["width"], scn["height"], solver=solver)
        self.trk = tracker.Tracker(self.flow, flow.camera(), tracker_params(scn))
        if enable:
            tracker_pnp.enable(self.trk, pnp_params(scn))

    def process(self, left, right, delta_guess=None, outliers=()):
        out = self.trk.process(left, right, delta_guess, outliers)
        out["pose"] = tracker_pnp.last(self.trk)
        if out["flags"] & tracker.NO_PREVIOUS:
            return out, None
        inter = self.trk.download()
        if self.scn["cull"] is not None:
            inter["cull"] = self.trk.download_cull()
        inter["pnp"] = tracker_pnp.download(self.trk)
        return out, inter

    def close(self):
        self.trk.close()
        self.flow.close()


def checker(scn, solver=None):
    return tpo.PnpChecker(tpo.base_checker(scn, flow.camera(), solver=solver), flow.camera(), pnp_params(scn), solver=solver)


def same(got, want, what):
    """Byte equality of (result, intermediates): the tracker's, the cull's where the reference has them, the pose guess's."""
    gc.same(got, want, what)
    tpo.assert_same_pose(got[0]["pose"], want[0]["pose"], what + " pose")
    if want[1] is not None:
        if "cull" in want[1]:
            cc.tco.assert_same_cull(got[1]["cull"], want[1]["cull"], what + " cull")
        tpo.assert_same_hook(got[1]["pnp"], want[1]["pnp"], what + " pnp hook")


def outliers_of(scn, k, prev):
    rule = scn["outliers"][k]
    return rule(prev) if (rule is not None and prev is not None) else []


def lockstep(scn, reference, subjects, what=""):
    log, prev = [], None
    for k, (left, right) in enumerate(scn["frames"]):
        outl = outliers_of(scn, k, prev)
        want = reference.process(left, right, scn["guesses"][k], outl)
        for s in subjects:
            same(s.process(left, right, scn["guesses"][k], outl), want, f"{what} frame {k}")
        log.append(want)
        prev = want[0]
    return log


def against_log(scn, log, subject, what=""):
    prev = None
    for k, (left, right) in enumerate(scn["frames"]):
        same(subject.process(left, right, scn["guesses"][k], outliers_of(scn, k, prev)), log[k], f"{what} frame {k}")
        prev = log[k][0]


def summary(log):
    """Per frame: None, or (matches, inliers, winner count, pass counts, sentinel)."""
    out = []
    for r, i in log:
        if i is None:
            out.append(None)
            continue
        h = i["pnp"]
        wc = int(h["counts"][h["winner"]]) if h["winner"] >= 0 else -1
        out.append((len(r["pose"]["matches"]), len(r["pose"]["inliers"]), wc, [int(c) for c in h["pass_count"]], not r["pose"]["T"].any()))
    return out


def is_sentinel(pose):
    return not pose["T"].any() and pose["cov"].tobytes() == np.eye(6).tobytes() and len(pose["inliers"]) == 0


def assert_conditions(name, scn, log):
    """The scenario does what it is for, on the reference's own run (a broken scenario is a broken test, not a pass)."""
    s = summary(log)
    tracked = [(k, r, i) for k, (r, i) in enumerate(log) if i is not None]
    assert tracked and log[0][1] is None and log[0][0]["pose"]["ran"] == 0, name
    assert all(r["pose"]["ran"] == 1 for _, r, _ in tracked), name
    if name == "steady":
        assert [(x[0], x[1]) for x in s[1:]] == [(59, 59), (57, 57), (57, 57), (55, 55), (56, 56)], s
    if name in ("foreign", "foreign_cull"):
        assert all(i["pnp"]["valid"].sum() > 0 and len(i["pnp"]["counts"]) == 64 for _, _, i in tracked), s
        assert all(0 < x[1] < x[0] for x in s[3:8]), s                 # inliers are a proper subset: the search and the selection work
    if name == "foreign":
        assert [(x[1], x[0]) for x in s[3:8]] == [(44, 58), (41, 52), (43, 57), (29, 55), (45, 57)], s
        assert s[6][3] == [41, 40, 36, 29, 22], s
    if name == "winner_below_min":
        assert all(x[4] and x[0] >= 50 for x in s[3:8]) and [x[2] for x in s[3:8]] == [44, 41, 43, 42, 45], s
        assert all(is_sentinel(log[k][0]["pose"]) for k in range(3, 8))
    if name == "tight":
        assert s[2][3] == [53, 49, 41, 32, 27] and s[4][3] == [55, 51, 45, 39, 32], s
    if name == "too_few":
        assert s[1][0] == 59 and not s[1][4] and s[1][1] >= 58, s
        assert all(x[0] == 57 and x[4] and x[2] == -1 for x in s[2:4]), s
        assert all(len(log[k][1]["pnp"]["counts"]) == 0 for k in (2, 3))
    if name == "no_refine":
        assert all(x[4] and x[1] == 0 and x[0] >= 12 and x[2] >= 12 and x[3] == [] for x in s[1:]), s
    if name == "nan_rows":
        assert len(log[1][0]["covisible_id"]) == 59 and s[1][0] == 21 and log[1][1]["pnp"]["rows_without_word"] == 39, \
            (len(log[1][0]["covisible_id"]), s[1], log[1][1]["pnp"]["rows_without_word"])
    if name == "lost":
        assert log[3][0]["flags"] & to.LOST and s[3][0] == 0 and is_sentinel(log[3][0]["pose"]), s
        assert log[4][0]["flags"] & to.BOOTSTRAPPED and not s[4][4], s
    if name == "m4":
        assert any(x[0] == 4 and not x[4] for x in s[1:]), s
        assert all(len(i["pnp"]["counts"]) == (5 if x[0] >= 4 else 0) for x, (_, _, i) in zip(s[1:], tracked)), s
    if name == "m3":
        assert all(x[0] <= 3 and x[4] and x[2] == -1 for x in s[1:]) and any(x[0] == 3 for x in s[1:]), s
        assert all(len(i["pnp"]["counts"]) == 0 for _, _, i in tracked)
    if name == "no_words":
        assert all(len(r["word_id"]) == 0 and i["pnp"]["to_xyz_is_null"] for _, r, i in tracked), [len(r["word_id"]) for _, r, _ in tracked]
        assert s[4][0] == 4, s
    if name == "big":
        assert max(x[0] for x in s[1:]) > 256, s
    if name.startswith("edge"):
        assert all(len(i["pnp"]["counts"]) == scn["pnp"]["iterations"] for _, _, i in tracked), s


@functools.lru_cache(maxsize=None)
def host_log(name):
    """The case on the host-twin tracker; computed once, shared and left unchanged."""
    scn = CASES[name]()
    sub = Subject(scn)
    try:
        log, prev = [], None
        for k, (left, right) in enumerate(scn["frames"]):
            log.append(sub.process(left, right, scn["guesses"][k], outliers_of(scn, k, prev)))
            prev = log[-1][0]
    finally:
        sub.close()
    for _, i in log:                                   # (what only the checker can tell)
        if i is not None:
            i["pnp"].setdefault("rows_without_word", None)
    return scn, log


# ---- the rig of four for the group: the members of tracker_cull_cases.py (the cull on, which makes member 1 lose tracking and
# bootstrap inside the run), the pose guess behind it
RIG_PNP = dict(iterations=64)


class Rig(cc.Rig):
    """tracker_cull_cases.Rig whose trackers have the pose guess enabled before the group exists (enable=False: never)."""

    def __init__(self, members, solver=None, cull=1, flow_back=0, enable=True):
        super().__init__(members, solver=solver, cull=cull, flow_back=flow_back)
        if enable:
            for t in self.trks:
                tracker_pnp.enable(t, pnp.default_params(**RIG_PNP))

    def single(self, i, left, right, guess=None, outliers=()):
        out, inter = super().single(i, left, right, guess, outliers)
        return self._with_pose(i, out, inter)

    def _with_pose(self, i, out, inter):
        out["pose"] = tracker_pnp.last(self.trks[i])
        if inter is not None:
            inter["pnp"] = tracker_pnp.download(self.trks[i])
        return out, inter

    def grouped(self, args):
        return [self._with_pose(i, out, inter) for i, (out, inter) in enumerate(super().grouped(args))]


def rig_against(members, log, sub, what, grouped=True, between=None):
    prev = [None] * len(members)
    for i, m in enumerate(members):
        for pair in m["pre"]:
            prev[i] = sub.single(i, *pair)[0]
    for k, want in enumerate(log):
        if between is not None:
            between(k)
        args = gc.call_args(members, k, prev)
        got = sub.grouped(args) if grouped else [sub.single(i, *a) for i, a in enumerate(args)]
        for i in range(len(members)):
            same(got[i], want[i], f"{what}: call {k}, member {i}")
        prev = [w[0] for w in want]


@functools.lru_cache(maxsize=None)
def rig_reference():
    """The rig on host twins called singly: (members, per call per member (result, intermediates), per call per member whether it
    bootstraps).  Computed once and left unchanged."""
    members = cc.rig_members()
    ref = Rig(members)
    try:
        prev = [None] * len(members)
        for i, m in enumerate(members):
            for pair in m["pre"]:
                prev[i] = ref.single(i, *pair)[0]
        before_first, log = list(prev), []
        for k in range(len(members[0]["frames"])):
            log.append([ref.single(i, *a) for i, a in enumerate(gc.call_args(members, k, prev))])
            prev = [w[0] for w in log[-1]]
    finally:
        ref.close()
    flags = [[r["flags"] for r, _ in call] for call in log]
    assert any(f[1] & to.LOST for f in flags) and any(f[1] & to.BOOTSTRAPPED for f in flags[2:]), flags      # lost, and back inside the run
    assert len(log[2][3][1]["lk_status"]) < len(log[2][0][1]["lk_status"]), "the outlier list of member 3 took no row away"
    poses = [[r["pose"] for r, _ in call] for call in log]
    assert all(any(p["ran"] and p["T"].any() for p in col) for col in zip(*poses)), "a member never got a pose"
    assert any(p["ran"] and is_sentinel(p) for call in poses for p in call), "no call of the rig gave the sentinel"
    return members, log, cc.boots(log, before_first)
