"""An independent checker of the resident front end (include/visfs_tracker.h): Tracker::pretreatment and Tracker::imageProcess
(corelib/src/Tracker.cpp:98-419) restated in plain Python, with dicts standing in for the reference's std::maps.

It drives the *staged* calls of a host-twin flow.Flow (track, corners.corners, stereo, hook_triangulate) and does all the bookkeeping
itself: pretreatment, the guess projection in float64, the reduce, track counts, the disc order, ids, erasures.  It shares no code
with ba_tracker.*; what it shares with the library is the pixel work of the staged calls, which have their own checkers."""
import numpy as np

from visfs_amd import clahe, corners, flow

NO_PREVIOUS, BOOTSTRAPPED, LOST = 1, 2, 4


def _f32(rows, width):
    return np.asarray(rows, dtype=np.float32).reshape(-1, width)


def _u64(ids):
    return np.asarray(list(ids), dtype=np.uint64)


def guess_camera_ref(delta, tir):
    """(delta * Tir)^-1 of two 3x4 row-major isometries, every product and sum a rounded float64 operation, sums left to right."""
    D = [float(v) for v in np.asarray(delta, dtype=np.float64).reshape(-1)[:12]]
    T = [float(v) for v in tir]
    R = [[(D[4 * i] * T[j] + D[4 * i + 1] * T[4 + j]) + D[4 * i + 2] * T[8 + j] for j in range(3)] for i in range(3)]
    t = [((D[4 * i] * T[3] + D[4 * i + 1] * T[7]) + D[4 * i + 2] * T[11]) + D[4 * i + 3] for i in range(3)]
    Ri = [[R[j][i] for j in range(3)] for i in range(3)]
    ti = [-((R[0][i] * t[0] + R[1][i] * t[1]) + R[2][i] * t[2]) for i in range(3)]
    return Ri, ti


def project(Ri, ti, cam, xyz):
    """cv::projectPoints without distortion, float64, cast to float32 (Tracker.cpp:251)."""
    P = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        X = [((Ri[r][0] * P[:, 0] + Ri[r][1] * P[:, 1]) + Ri[r][2] * P[:, 2]) + ti[r] for r in range(3)]
        u = (float(cam.fx) * X[0]) / X[2] + float(cam.cx)
        v = (float(cam.fy) * X[1]) / X[2] + float(cam.cy)
        return np.stack([u, v], -1).astype(np.float32)


def in_bounds(v, size):
    """uIsInBounds(v, 0, size) of utilite/include/Math.h:47 on float32 values."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.isfinite(v) & (v >= np.float32(0)) & (v < np.float32(size))


class Checker:
    """State of the reference's Tracker between frames, and one frame of it per process() call."""

    def __init__(self, width, height, cam, max_features=300, quality_level=0.01, min_distance=40, min_inliers=10, clahe_params=None,
                 solver=None, **flow_params):
        self.prm = flow.default_params(**flow_params)
        # staged calls only; on the host twin, or (solver given) on the device, which pins the resident call to today's staged path
        self.flow = flow.Flow(self.prm, width, height, solver=solver)
        self.w, self.h, self.cam = width, height, cam
        self.max_features, self.quality_level = int(max_features), float(quality_level)
        self.min_distance, self.min_inliers = int(min_distance), int(min_inliers)
        self.clahe_params = clahe_params
        self.words, self.words3d, self.track_cnt = {}, {}, {}    # lastSignature_'s words, words3d; trackCnt_
        self.next_id = 0                                         # globalFeatureId_
        self.frames = 0
        self.stats = dict(left_border=0, topups_after_first=0, undrawn=0, unequal_counts=0, nan_covisible=0, duplicate_pixels=0)

    def close(self):
        self.flow.close()

    def reset(self):
        self.words, self.words3d = {}, {}

    def _push(self, left, right):
        if self.clahe_params is not None:
            clahe.push_frame(self.flow, self.clahe_params, left, right)
        else:
            self.flow.push_frame(left, right)
        self.frames += 1

    def _corners(self, n, discs=None):
        return corners.corners(self.flow, discs=discs if discs else None, max_corners=n, quality_level=self.quality_level,
                               min_distance=float(self.min_distance))

    @staticmethod
    def _empty(flags, next_id):
        z2, z3 = _f32([], 2), _f32([], 3)
        return dict(flags=flags, next_id=next_id, covisible_id=_u64([]), covisible_from_xy=z2, covisible_from_xyz=z3, covisible_to_xy=z2,
                    new_id=_u64([]), new_xy=z2, word_id=_u64([]), word_left_xy=z2, word_right_xy=z2, word_xyz=z3,
                    word_count=np.zeros(0, dtype=np.int32), blocked_id=_u64([]))

    def process(self, left, right, delta_guess=None, outliers=()):
        """-> (result dict as tracker.Tracker.process gives it, intermediates dict as tracker.Tracker.download gives it or None)."""
        # ---- pretreatment (:143-165): outliers leave words, words3d and trackCnt_; they are this frame's blocked words
        blocked = {}
        if self.words and len(outliers):
            for o in sorted(set(int(v) for v in outliers)):
                if o in self.words:
                    blocked[o] = self.words.pop(o)
                    self.words3d.pop(o)
                self.track_cnt.pop(o, None)
        # ---- nothing to track against (:168)
        if self.frames == 0:
            self._push(left, right)
            return self._empty(NO_PREVIOUS, 0), None
        # ---- an empty from-signature gets its words from its own images (:179-230); they are still the newest pair here
        boot = not self.words
        if boot:
            xy = self._corners(self.max_features)
            right_xy, _, _ = self.flow.stereo(xy, self.cam)      # the forward pass's points, whatever the gate says (:207)
            xyz = flow.hook_triangulate(self.prm, self.cam, xy, right_xy)
            for k in range(len(xy)):
                self.words[self.next_id] = xy[k].copy()
                self.words3d[self.next_id] = xyz[k].copy()
                self.next_id += 1
        self._push(left, right)
        ids = sorted(self.words)                                 # uKeys / uValues: ascending id
        from_xy = _f32([self.words[i] for i in ids], 2)
        from_xyz = _f32([self.words3d[i] for i in ids], 3)
        # ---- guess (:237-252)
        guess = None
        if delta_guess is not None and len(ids):
            Ri, ti = guess_camera_ref(delta_guess, list(self.cam.Tir))
            guess = project(Ri, ti, self.cam, from_xyz)
        # ---- track (:257-274) and reduce (:280-301)
        to, status, _ = self.flow.track(from_xy, guess)
        inb = in_bounds(to[:, 0], self.w) & in_bounds(to[:, 1], self.h) if len(ids) else np.zeros(0, dtype=bool)
        keep = (status == 1) & inb
        self.stats["left_border"] += int(((status == 1) & ~inb).sum())
        inter = dict(guess_xy=guess if guess is not None else from_xy.copy(), to_xy=to, lk_status=status, in_bounds=inb.astype(np.uint8),
                     discs=np.zeros(0, dtype=corners.DISC_DTYPE), disc_drawn=np.zeros(0, dtype=np.uint8),
                     stereo_status=np.zeros(0, dtype=np.uint8))
        kept_ids = [i for i, k in zip(ids, keep) if k]
        if len(kept_ids) < self.min_inliers:                     # :303: the new signature has no words; the next frame starts afresh
            self.words, self.words3d = {}, {}
            return self._empty(LOST, self.next_id), inter
        out = self._empty(BOOTSTRAPPED if boot else 0, 0)
        out["covisible_id"] = _u64(kept_ids)
        out["covisible_from_xy"], out["covisible_from_xyz"], out["covisible_to_xy"] = from_xy[keep], from_xyz[keep], to[keep]
        self.stats["nan_covisible"] += int(np.isnan(from_xyz[keep]).any(axis=1).sum())
        words_to = {i: p.copy() for i, p in zip(kept_ids, to[keep])}
        # ---- top-up behind getMask (:116-141, :322-341)
        backup = self.max_features - len(kept_ids)
        new_ids, new_xy = [], _f32([], 2)
        if backup > 0:
            current = [(self.track_cnt[i], i) for i in kept_ids if i in self.track_cnt]
            current.sort(key=lambda c: -c[0])                    # stable: equal counts stay in id order
            if len(set(c for c, _ in current)) > 1:
                self.stats["unequal_counts"] += 1
            discs = [(float(words_to[i][0]), float(words_to[i][1]), self.min_distance) for _, i in current]
            discs += [(float(blocked[i][0]), float(blocked[i][1]), self.min_distance // 2) for i in sorted(blocked)]
            new_xy = self._corners(backup, discs)
            if discs:
                inter["discs"] = corners.make_discs(discs)
                inter["disc_drawn"] = corners.download(self.flow, len(discs))["disc_drawn"]
                self.stats["undrawn"] += int((inter["disc_drawn"] == 0).sum())
            if len(new_xy) and self.frames > 2:
                self.stats["topups_after_first"] += 1
            if len(new_xy) and len(kept_ids):                    # new words on top of kept ones: only the uncounted rows allow it
                d = np.linalg.norm(new_xy[:, None, :].astype(np.float64) - to[keep][None].astype(np.float64), axis=2)
                self.stats["duplicate_pixels"] += int((d.min(axis=1) < 2.0).sum())
            for p in new_xy:
                new_ids.append(self.next_id)
                words_to[self.next_id] = p.copy()
                self.next_id += 1
        out["new_id"], out["new_xy"] = _u64(new_ids), new_xy
        # ---- stereo (:343-397)
        all_ids = sorted(words_to)
        left_xy = _f32([words_to[i] for i in all_ids], 2)
        right_xy, st, _ = self.flow.stereo(left_xy, self.cam)
        inter["stereo_status"] = st
        words_right = {}
        for k, i in enumerate(all_ids):
            if st[k] and in_bounds(right_xy[k, 0], self.w) and in_bounds(right_xy[k, 1], self.h):
                words_right[i] = right_xy[k].copy()
            else:
                del words_to[i]
        ids_left = sorted(words_to)
        xyz = flow.hook_triangulate(self.prm, self.cam, _f32([words_to[i] for i in ids_left], 2), _f32([words_right[i] for i in ids_left], 2))
        words3d = {}
        for k, i in enumerate(ids_left):
            if np.isfinite(xyz[k]).all():
                words3d[i] = xyz[k].copy()
            else:
                del words_to[i], words_right[i]
        # ---- updateTrackCounter (:98-114)
        arrived = set(words_to)
        for i in list(self.track_cnt):
            if i in arrived:
                self.track_cnt[i] += 1
                arrived.discard(i)
            else:
                del self.track_cnt[i]
        for i in arrived:
            self.track_cnt[i] = 1
        self.words, self.words3d = words_to, words3d
        final = sorted(words_to)
        out["word_id"] = _u64(final)
        out["word_left_xy"] = _f32([words_to[i] for i in final], 2)
        out["word_right_xy"] = _f32([words_right[i] for i in final], 2)
        out["word_xyz"] = _f32([words3d[i] for i in final], 3)
        out["word_count"] = np.asarray([self.track_cnt[i] for i in final], dtype=np.int32)
        out["blocked_id"] = _u64(sorted(blocked))
        out["next_id"] = self.next_id
        return out, inter


RESULT_KEYS = ("covisible_id", "covisible_from_xy", "covisible_from_xyz", "covisible_to_xy", "new_id", "new_xy", "word_id",
               "word_left_xy", "word_right_xy", "word_xyz", "word_count", "blocked_id")
INTER_KEYS = ("guess_xy", "to_xy", "lk_status", "in_bounds", "discs", "disc_drawn", "stereo_status")


def assert_same(got, want, what=""):
    """Byte equality of two result (or intermediates) dicts."""
    for key in ("flags", "next_id"):
        if key in want:
            assert got[key] == want[key], (what, key, got[key], want[key])
    for key in RESULT_KEYS + INTER_KEYS:
        if key not in want:
            continue
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        assert a.dtype == b.dtype, (what, key, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, key)
