"""Scenarios the resident-tracker tests share (host twin against the checker of tracker_oracle.py, device against host twin), built
from the synthetic scenes of flow_cases.py / flow_oracle.py.  Everything is generated; nothing is read from disk.

A scenario is a dict: width, height, frames [(left, right)], tracker keywords (max_features, quality_level, min_distance,
min_inliers), flow keywords, clahe (bool), guesses [None | 3x4] per frame, outliers [None | f(previous result) -> ids] per frame."""
import functools

import numpy as np

import flow_cases as fc
import tracker_oracle as to
from visfs_amd import clahe, flow, tracker


def scenario(frames, max_features, min_distance, min_inliers=10, clahe_on=False, guesses=None, outliers=None, quality_level=0.01, **flow_kw):
    h, w = frames[0][0].shape
    n = len(frames)
    return dict(width=w, height=h, frames=frames, clahe=clahe_on, flow=flow_kw,
                trk=dict(max_features=max_features, quality_level=quality_level, min_distance=min_distance, min_inliers=min_inliers),
                guesses=guesses or [None] * n, outliers=outliers or [None] * n)


@functools.lru_cache(maxsize=None)
def sequence(n, width=320, height=240):
    return fc.sequence(n, width, height)


@functools.lru_cache(maxsize=None)
def still_sequence(n, width=320, height=240):
    """The same stereo pair n times: every word is tracked onto itself."""
    left, right, _ = fc.still_pair(width, height, "slant", seed=5)
    return [(left, right)] * n


@functools.lru_cache(maxsize=None)
def patch_sequence(n, width=320, height=240):
    """A flat image with one textured patch: the discs of the words on the patch cover it, and a top-up behind them finds nothing."""
    left, right, d = fc.still_pair(width, height, "plane", seed=5)
    shift = int(round(d.d0))                     # the patch is a rectangle at the plane's depth: the right image shows it shifted
    out = []
    for img, x0 in ((left, 140), (right, 140 - shift)):
        flat = np.full_like(img, 128)
        flat[100:140, x0:x0 + 40] = img[100:140, x0:x0 + 40]
        out.append(flat)
    return [(out[0], out[1])] * n


@functools.lru_cache(maxsize=None)
def lost_sequence(width=320, height=240):
    """Frames 0-2 of the drifting sequence, then frames 3-5 of the same drift over a differently seeded texture (the idea of
    flow_cases.replaced_region_pair over the whole frame): frame 3 finds nothing of frame 2, frame 4 starts afresh on frame 3."""
    return list(sequence(3, width, height)) + list(fc.sequence(6, width, height, seed=105))[3:]


def translation(tx=0.0, ty=0.0, tz=0.0):
    return np.array([[1, 0, 0, tx], [0, 1, 0, ty], [0, 0, 1, tz]], dtype=np.float64)


def yaw(angle, tx=0.0):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0, tx], [s, c, 0, 0], [0, 0, 1, 0]], dtype=np.float64)


# ---- outlier rules: f(previous result) -> ids
def first_middle_last(prev):
    ids = prev["word_id"]
    return [int(ids[0]), int(ids[len(ids) // 2]), int(ids[-1]), 10 ** 9, int(ids[-1]) + 12345] if len(ids) else [7]


def every_id(prev):
    return [int(i) for i in prev["word_id"]]


def every_third(prev):
    return [int(i) for i in prev["word_id"][::3]]


def full_outlier_list(prev):
    """The 4096 ids a call may carry at the most: every third id of the previous result, then ids no tracker has handed out."""
    ids = every_third(prev)
    return ids + [int(prev["next_id"]) + 1000 + k for k in range(tracker.MAX_OUTLIERS - len(ids))]


class Subject:
    """A tracker.Tracker on a flow.Flow (solver given: device; None: host twin) behind the checker's process() signature."""

    def __init__(self, scn, solver=None, flow_obj=None):
        self.own_flow = flow_obj is None
        self.flow = flow_obj if flow_obj is not None else flow.Flow(flow.default_params(**scn["flow"]), scn["width"], scn["height"], solver=solver)
        self.trk = tracker.Tracker(self.flow, flow.camera(), tracker.default_params(clahe=1 if scn["clahe"] else 0, **scn["trk"]))

    def process(self, left, right, delta_guess=None, outliers=()):
        out = self.trk.process(left, right, delta_guess, outliers)
        return out, (None if out["flags"] & tracker.NO_PREVIOUS else self.trk.download())

    def close(self):
        self.trk.close()
        if self.own_flow:
            self.flow.close()


def checker(scn, solver=None):
    return to.Checker(scn["width"], scn["height"], flow.camera(), clahe_params=clahe.default_params() if scn["clahe"] else None,
                      solver=solver, **scn["trk"], **scn["flow"])


def lockstep(scn, reference, subjects, what=""):
    """Runs the scenario on `reference` and on every subject, frame by frame, asserting byte equality of every output array, flag
    and intermediate list.  The outlier lists come from the reference's previous result.  Returns the reference's per-frame
    (result, intermediates)."""
    log, prev = [], None
    for k, (left, right) in enumerate(scn["frames"]):
        rule = scn["outliers"][k]
        outl = rule(prev) if (rule is not None and prev is not None) else []
        want, want_inter = reference.process(left, right, scn["guesses"][k], outl)
        for s in subjects:
            got, got_inter = s.process(left, right, scn["guesses"][k], outl)
            to.assert_same(got, want, f"{what} frame {k}")
            assert (got_inter is None) == (want_inter is None), (what, k)
            if want_inter is not None:
                to.assert_same(got_inter, want_inter, f"{what} frame {k} intermediates")
        log.append((want, want_inter))
        prev = want
    return log


# ---- the cases of the issue, shared by the host and the device tests: name -> () -> scenario
def base_cases():
    out = {}
    for mf, md in ((60, 12), (300, 20)):
        for cl in (False, True):
            for fb in (1, 0):
                out[f"mf{mf}_md{md}_clahe{int(cl)}_back{fb}"] = functools.partial(scenario, sequence(20), mf, md, clahe_on=cl, flow_back=fb)
    return out


BASE = base_cases()
WAVE = {f"mf{mf}": functools.partial(scenario, sequence(6), mf, 12) for mf in (63, 64, 65, 129)}
# k_trk_track_g and k_trk_stereo_g carry their own copy of the wavefront's window cells (7 slots of 64): window sizes that end one
# row of cells past a slot boundary (9), exactly on one (8: 64 cells, 16: 256 cells) and inside slot 0 (3), at other pyramid depths
WINDOW = {
    "win_9_levels_3": functools.partial(scenario, sequence(5), 65, 12, win_size=9, max_level=2),
    "win_8_levels_2": functools.partial(scenario, sequence(5), 65, 12, win_size=8, max_level=1),
    "win_16_levels_3_back0": functools.partial(scenario, sequence(5), 65, 12, win_size=16, max_level=2, flow_back=0),
    "win_3_levels_5": functools.partial(scenario, sequence(5), 65, 12, win_size=3, max_level=4),
}


def full_size():
    return scenario(sequence(3, 752, 480), 300, 40)


def bootstrap_nan():
    """max_depth inside the slant's depth range (3.5 .. 5 m): the ungated bootstrap stereo leaves NaN triples in the table."""
    return scenario(sequence(4), 60, 12, max_depth=4.2)


def blocked_bootstrap():
    """Every word of frame 1 is an outlier in frame 2: it bootstraps behind blocked discs alone (radius 13 / 2)."""
    return scenario(sequence(4), 60, 13, outliers=[None, None, every_id, None])


def lost_case():
    """min_inliers above the handful of chance matches a foreign texture gives."""
    return scenario(lost_sequence(), 60, 12, min_inliers=30)


def no_top_up():
    return scenario(still_sequence(4), 8, 12, min_inliers=4)


def empty_top_up():
    """min_distance 80 over a 40 x 40 patch: the disc of any counted word covers every corner the patch has."""
    return scenario(patch_sequence(4), 60, 80, min_inliers=1)


def full_outliers():
    """Frame 2, a steady frame, gets an outlier list of full length."""
    return scenario(sequence(4), 60, 12, outliers=[None, None, full_outlier_list, None])


def guess_cases():
    n = 5
    seq = sequence(n)
    return {
        # the sequence drifts 2.5 px right per frame; at ~4 m that is the image of a sideways step of about -2.5 * 4 / 435 m
        "translation": scenario(seq, 60, 12, guesses=[translation(ty=0.023)] * n),
        "identity": scenario(seq, 60, 12, guesses=[translation()] * n),
        "thrown_out": scenario(seq, 60, 12, guesses=[None, None, yaw(0.25), yaw(-0.3, 0.2), translation(ty=0.023)]),
    }


def pretreatment_cases():
    n = 6
    seq = sequence(n)
    return {
        "first_middle_last": scenario(seq, 60, 13, outliers=[None, None, first_middle_last, first_middle_last, None, first_middle_last]),
        "every_id": scenario(seq, 60, 13, outliers=[None, None, None, every_id, None, every_third]),
        "empty": scenario(seq, 60, 13, outliers=[None] * n),
    }
