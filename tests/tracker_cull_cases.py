"""Scenarios of the fundamental-matrix cull inside the resident tracker, shared by the host and the device
tests.  All are 320 x 240 (but the full-size one), min_distance 12, flow_back 0, cull on, pixel_error 1.0, seed 0.  Everything is
generated.  A scenario is one of tracker_cases.py with a `cull` entry: dict(cull, pixel_error, iterations, seed)."""
import functools

import flow_cases as fc
import group_cases as gc
import tracker_cases as tc
import tracker_cull_oracle as tco
import tracker_oracle as to
from visfs_amd import flow, fund, tracker


def scenario(frames, max_features, min_inliers, iterations, min_distance=12, cull=1, flow_back=0, pixel_error=1.0, **kw):
    scn = tc.scenario(frames, max_features, min_distance, min_inliers=min_inliers, flow_back=flow_back, **kw)
    scn["cull"] = dict(cull=cull, pixel_error=pixel_error, iterations=iterations, seed=0)
    return scn


@functools.lru_cache(maxsize=None)
def foreign_sequence():
    """The drifting sequence; in the odd frames from 3 on a rectangle of the left image shows another texture: the words on it are
    tracked somewhere with status 1 and do not move with the rest."""
    base, other = tc.sequence(8), fc.sequence(8, seed=105)
    out = []
    for k, (left, right) in enumerate(base):
        if k >= 3 and k % 2 == 1:
            left = left.copy()
            left[60:160, 100:220] = other[(3 * k) % 8][0][60:160, 100:220]
        out.append((left, right))
    return out


def foreign():
    return scenario(foreign_sequence(), 60, 10, 64)


def lost_by_cull():
    return scenario(foreign_sequence(), 60, 50, 64)


def small(max_features):
    return scenario(tc.sequence(4), max_features, 3, 16)


def nan_rows():
    return scenario(tc.sequence(4), 60, 10, 64, max_depth=4.2, guesses=[tc.translation(ty=0.023)] * 4)


def edge(max_features, iterations):
    return scenario(tc.sequence(4), max_features, 10, iterations)


def full_size():
    scn = tc.full_size()
    scn["flow"]["flow_back"] = 0
    scn["cull"] = dict(cull=1, pixel_error=1.0, iterations=256, seed=0)
    return scn


def ignored():
    """cull = 1 with the reverse pass on: the field is ignored, as Tracker.cpp:275 ignores it."""
    return scenario(tc.sequence(6), 60, 10, 64, flow_back=1)


CASES = {"ignored": ignored, "foreign": foreign, "lost_by_cull": lost_by_cull, "m6": functools.partial(small, 6), "m7": functools.partial(small, 7),
         "m8": functools.partial(small, 8), "nan_rows": nan_rows, "full_size": full_size}
for _mf in (63, 64, 65, 129):
    for _it in (5, 65):
        CASES[f"edge_mf{_mf}_it{_it}"] = functools.partial(edge, _mf, _it)


def params(scn):
    c = scn["cull"]
    return tracker.default_params(clahe=1 if scn["clahe"] else 0, cull=c["cull"],
                                  cull_params=fund.default_params(pixel_error=c["pixel_error"], iterations=c["iterations"], seed=c["seed"]),
                                  **scn["trk"])


class Subject(tc.Subject):
    """tracker_cases.Subject with the cull fields set and download_cull among the intermediates."""

    def __init__(self, scn, solver=None):
        self.own_flow = True
        self.flow = flow.Flow(flow.default_params(**scn["flow"]), scn["width"], scn["height"], solver=solver)
        self.trk = tracker.Tracker(self.flow, flow.camera(), params(scn))

    def process(self, left, right, delta_guess=None, outliers=()):
        out, inter = super().process(left, right, delta_guess, outliers)
        if inter is not None:
            inter["cull"] = self.trk.download_cull()
        return out, inter


def checker(scn, solver=None):
    return tco.CullChecker(scn["width"], scn["height"], flow.camera(), scn["cull"], solver=solver, **scn["trk"], **scn["flow"])


def same(got, want, what):
    gc.same(got, want, what)
    if want[1] is not None:
        tco.assert_same_cull(got[1]["cull"], want[1]["cull"], what + " cull")


def lockstep(scn, reference, subjects, what=""):
    """tracker_cases.lockstep with the cull intermediates compared too.  Returns the reference's per-frame (result, intermediates)."""
    log, prev = [], None
    for k, (left, right) in enumerate(scn["frames"]):
        rule = scn["outliers"][k]
        outl = rule(prev) if (rule is not None and prev is not None) else []
        want = reference.process(left, right, scn["guesses"][k], outl)
        for s in subjects:
            same(s.process(left, right, scn["guesses"][k], outl), want, f"{what} frame {k}")
        log.append(want)
        prev = want[0]
    return log


def against_log(scn, log, subject, what=""):
    """Drives a subject over a scenario whose reference log exists already."""
    prev = None
    for k, (left, right) in enumerate(scn["frames"]):
        rule = scn["outliers"][k]
        outl = rule(prev) if (rule is not None and prev is not None) else []
        same(subject.process(left, right, scn["guesses"][k], outl), log[k], f"{what} frame {k}")
        prev = log[k][0]


def before_and_after(inter):
    """(rows with LK status 1 and in bounds, rows of them the cull left)."""
    ok = (inter["lk_status"] == 1) & (inter["in_bounds"] == 1)
    return int(ok.sum()), int((ok & (inter["cull"]["status"] == 1)).sum()) if inter["cull"]["applied"] or len(inter["cull"]["status"]) else int(ok.sum())


def assert_conditions(name, scn, log):
    """The scenario does what it is for, on the reference's own run (a broken scenario is a broken test, not a pass)."""
    tracked = [(r, i) for r, i in log if i is not None]
    assert tracked, name
    if name == "ignored":
        assert len(tracked) == 5 and all(i["cull"]["applied"] == 0 and i["cull"]["m"] == 0 and len(i["cull"]["status"]) == 0 for _, i in tracked)
    if name == "foreign":
        assert not any(r["flags"] & to.LOST for r, _ in log), [r["flags"] for r, _ in log]
        for k in range(3, 8):
            before, after = before_and_after(log[k][1])
            assert before - after >= 5, (name, k, before, after)
    if name == "lost_by_cull":
        assert any((r["flags"] & to.LOST) and before_and_after(i)[0] >= scn["trk"]["min_inliers"] for r, i in tracked), \
            [(r["flags"], before_and_after(i)) for r, i in tracked]
    if name == "m6":
        assert all(i["cull"]["applied"] == 0 and i["cull"]["n_hypotheses"] == 0 and i["cull"]["m"] < 7 for _, i in tracked)
    if name == "m7":
        assert all(i["cull"]["applied"] == 1 and i["cull"]["n_hypotheses"] == 1 and i["cull"]["m"] == 7 for _, i in tracked)
    if name == "m8":
        assert all(i["cull"]["applied"] == 1 and i["cull"]["n_hypotheses"] == 16 and i["cull"]["m"] == 8 for _, i in tracked)
    if name == "nan_rows":
        assert any(7 <= i["cull"]["m"] < len(i["lk_status"]) for _, i in tracked), [(i["cull"]["m"], len(i["lk_status"])) for _, i in tracked]
    if name.startswith("edge") or name == "full_size":
        assert all(i["cull"]["applied"] == 1 and i["cull"]["n_hypotheses"] == scn["cull"]["iterations"] for _, i in tracked)
        assert max(len(i["lk_status"]) for _, i in tracked) >= scn["trk"]["max_features"] - 8      # the rows do reach the boundary


@functools.lru_cache(maxsize=None)
def host_log(name):
    """The case on the host-twin tracker; computed once, shared and left unchanged."""
    scn = CASES[name]()
    sub = Subject(scn)
    try:
        log, prev = [], None
        for k, (left, right) in enumerate(scn["frames"]):
            rule = scn["outliers"][k]
            outl = rule(prev) if (rule is not None and prev is not None) else []
            log.append(sub.process(left, right, scn["guesses"][k], outl))
            prev = log[-1][0]
    finally:
        sub.close()
    assert_conditions(name, scn, log)
    return scn, log


# ---- the rig of four for the group
RIG_FEATURES, RIG_MIN_INLIERS, RIG_ITERATIONS = 60, 50, 64


def rig_members():
    """Member 1 loses tracking to the cull and bootstraps inside the run, member 2 runs the same frames two single calls ahead,
    member 3 has outlier lists and a guess."""
    plain, foreign_frames = tc.sequence(8), foreign_sequence()
    return [gc.member(plain[:6]),
            gc.member(foreign_frames[:6]),
            gc.member(foreign_frames[2:], pre=foreign_frames[:2]),
            gc.member(plain[:6], outliers=[None, None, tc.every_third, None, tc.every_third, tc.every_third],
                      guesses=[None, None, None, tc.translation(ty=0.023), None, tc.translation(ty=0.023)])]


class Rig(gc.Rig):
    """group_cases.Rig whose trackers have the cull on (cull=0: off, for the launch counts of the sequence without it)."""

    def __init__(self, members, solver=None, cull=1, flow_back=0):
        self.flows, self.trks, self.group, self.counts = [], [], None, []
        scn = scenario([members[0]["frames"][0]], RIG_FEATURES, RIG_MIN_INLIERS, RIG_ITERATIONS, cull=cull, flow_back=flow_back)
        for m in members:
            f = flow.Flow(flow.default_params(**scn["flow"]), gc.W, gc.H, solver=solver)
            self.flows.append(f)
            self.trks.append(tracker.Tracker(f, m["cam"] if m["cam"] is not None else flow.camera(), params(scn)))

    def _inter(self, i, out):
        inter = super()._inter(i, out)
        if inter is not None:
            inter["cull"] = self.trks[i].download_cull()
        return inter


def rig_against(members, log, sub, what, grouped=True, between=None):
    """group_cases.against with the cull intermediates compared too."""
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


def boots(log, before_first):
    """Per call, per member: does the member bootstrap in this call?  It does when the result of its call before holds no words.
    before_first: per member the result of its last single call in front of the group calls, or None."""
    out, before = [], list(before_first)
    for call in log:
        out.append([inter is not None and (b is None or len(b["word_id"]) == 0) for (_, inter), b in zip(call, before)])
        before = [r for r, _ in call]
    return out


@functools.lru_cache(maxsize=None)
def rig_reference():
    """The rig on host twins called singly: (members, per call per member (result, intermediates), per call per member whether it
    bootstraps).  Computed once and left unchanged."""
    members = rig_members()
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
    assert any(f[2] & to.LOST for f in flags), flags
    assert all(f[0] in (0, to.NO_PREVIOUS, to.BOOTSTRAPPED) for f in flags), flags
    assert len(log[2][3][1]["lk_status"]) < len(log[2][0][1]["lk_status"]), "the outlier list of member 3 took no row away"
    assert any(i is not None and i["cull"]["applied"] == 1 for call in log for _, i in call)
    return members, log, boots(log, before_first)
