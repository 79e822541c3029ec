"""What the tracker-group tests share (include/visfs_tracker_group.h): the mixed-state rig of four members, the staggered rig of three,
a Rig of trackers that can be driven singly or through a group, and the lockstep comparison.  Everything is generated.

A member is a dict: frames [(left, right)] per group call, outliers [None | f(previous result) -> ids] and guesses [None | 3x4] per
call, cam (None: the bench camera), pre [(left, right)]: frames the member gets in single calls before the first group call."""
import functools

import flow_cases as fc
import tracker_cases as tc
import tracker_oracle as to
from visfs_amd import flow, tracker

W, H, MIN_DISTANCE, MIN_INLIERS = 320, 240, 12, 30


def member(frames, outliers=None, guesses=None, cam=None, pre=()):
    n = len(frames)
    return dict(frames=list(frames), outliers=outliers or [None] * n, guesses=guesses or [None] * n, cam=cam, pre=list(pre))


@functools.lru_cache(maxsize=None)
def seeded(n, seed):
    return fc.sequence(n, W, H, seed=seed)


def mixed_four():
    """Six calls: member 1 loses track in call 3 and bootstraps in call 4, member 2 has outliers and a guess and bootstraps in call 5
    behind blocked words, member 3 runs two frames ahead of member 0 on the same texture."""
    return [member(tc.sequence(8)[:6]),
            member(tc.lost_sequence()),
            member(seeded(8, 11)[:6], outliers=[None, None, tc.every_third, None, tc.first_middle_last, tc.every_id],
                   guesses=[None, None, None, tc.translation(ty=0.023), None, None]),
            member(tc.sequence(8)[2:])]


def staggered_three(n_calls=3):
    """Members 0 and 1 have had two single calls when the group starts, member 2 none."""
    a, b, c = tc.sequence(8), seeded(8, 11), seeded(8, 105)
    return [member(a[2:2 + n_calls], pre=a[:2]), member(b[2:2 + n_calls], pre=b[:2]), member(c[:n_calls])]


def nine(n_calls=3):
    cams = [flow.camera(), flow.camera(fx=400.0, fy=400.0)]
    return [member(seeded(8, (5, 11, 105)[i % 3])[i // 3:i // 3 + n_calls], cam=cams[i % 2]) for i in range(9)]


class Rig:
    """One tracker per member, each on a flow object of its own (solver given: device; None: host twins)."""

    def __init__(self, members, max_features, clahe_on=False, solver=None, **flow_kw):
        self.flows, self.trks, self.group, self.counts = [], [], None, []
        for m in members:
            f = flow.Flow(flow.default_params(**flow_kw), W, H, solver=solver)
            p = tracker.default_params(clahe=1 if clahe_on else 0, max_features=max_features, quality_level=0.01,
                                       min_distance=MIN_DISTANCE, min_inliers=MIN_INLIERS)
            self.flows.append(f)
            self.trks.append(tracker.Tracker(f, m["cam"] if m["cam"] is not None else flow.camera(), p))

    def _inter(self, i, out):
        return None if out["flags"] & tracker.NO_PREVIOUS else self.trks[i].download()

    def single(self, i, left, right, guess=None, outliers=()):
        out = self.trks[i].process(left, right, guess, outliers)
        return out, self._inter(i, out)

    def grouped(self, args):
        """One group call; the counts of the call are appended to self.counts before any download."""
        if self.group is None:
            self.group = tracker.TrackerGroup(self.trks)
        outs = self.group.process(args)
        self.counts.append(self.group.last_counts())
        return [(out, self._inter(i, out)) for i, out in enumerate(outs)]

    def close(self):
        if self.group is not None:
            self.group.close()
        for t in self.trks:
            t.close()
        for f in self.flows:
            f.close()


def same(got, want, what):
    to.assert_same(got[0], want[0], what)
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        to.assert_same(got[1], want[1], what + " intermediates")


def call_args(members, k, prev):
    args = []
    for m, p in zip(members, prev):
        rule = m["outliers"][k]
        outl = rule(p) if (rule is not None and p is not None) else []
        args.append((m["frames"][k][0], m["frames"][k][1], m["guesses"][k], outl))
    return args


def reference_log(members, ref):
    """The members run singly on `ref`, `pre` frames first: per call, per member (result, intermediates)."""
    prev = [None] * len(members)
    for i, m in enumerate(members):
        for pair in m["pre"]:
            prev[i] = ref.single(i, *pair)[0]
    log = []
    for k in range(len(members[0]["frames"])):
        log.append([ref.single(i, *a) for i, a in enumerate(call_args(members, k, prev))])
        prev = [w[0] for w in log[-1]]
    return log


def against(members, log, sub, what, grouped=True, between=None):
    """Drives `sub` (through its group, or singly) over the calls of a reference log and asserts byte equality of every output,
    flag and intermediate list after every call.  between(k): called in front of call k."""
    prev = [None] * len(members)
    for i, m in enumerate(members):
        for pair in m["pre"]:
            prev[i] = sub.single(i, *pair)[0]
    for k, want in enumerate(log):
        if between is not None:
            between(k)
        args = call_args(members, k, prev)
        got = sub.grouped(args) if grouped else [sub.single(i, *a) for i, a in enumerate(args)]
        for i in range(len(members)):
            same(got[i], want[i], f"{what}: call {k}, member {i}")
        prev = [w[0] for w in want]


def flags(log, k):
    return [r["flags"] for r, _ in log[k]]


def from_rows(log, k):
    return [len(i["lk_status"]) for _, i in log[k]]


def assert_mixed_conditions(log, with_loss=True):
    """The scenario does what it is for (a broken scenario is a broken test, not a pass)."""
    rows = from_rows(log, 2)
    assert len(set(rows)) > 1, rows
    assert flags(log, 5)[2] == to.BOOTSTRAPPED, flags(log, 5)
    if with_loss:
        assert max(rows) - min(rows) >= 15, rows
        assert flags(log, 5) == [0, 0, to.BOOTSTRAPPED, 0], flags(log, 5)
        assert flags(log, 3) == [0, to.LOST, 0, 0], flags(log, 3)
        assert flags(log, 4) == [0, to.BOOTSTRAPPED, 0, 0], flags(log, 4)


@functools.lru_cache(maxsize=None)
def mixed_reference(max_features, clahe_on=False, flow_back=1):
    """The mixed-state rig on host twins called singly; computed once per setting and left unchanged."""
    members = mixed_four()
    ref = Rig(members, max_features, clahe_on=clahe_on, flow_back=flow_back)
    try:
        log = reference_log(members, ref)
    finally:
        ref.close()
    assert_mixed_conditions(log, with_loss=not clahe_on)
    return members, log
