"""One frame of the image front end at 752 x 480 with 300 features, three ways over the same frames:

  resident   visfs_tracker_process of this tree's library (one upload, one launch sequence, one download, one synchronise)
  staged     the chain callers had before it: push_frame -> track -> host reduce -> corners behind the host-made discs -> stereo ->
             host erase and track counts, on the library VISFS_BA_STAGED_LIB names (the parent commit's build; default: this tree's)
  host twin  visfs_tracker_process on a visfs_flow_create_host object (one core)

Each GPU way runs in a child process of its own (a process loads one library), --repeats children per way, interleaved
(resident, staged, resident, ...).  A child runs the whole sequence once; the first --warmup frames (no previous pair, the bootstrap,
first steady frames) are not counted.  Reported: the median over a child's frames, then median and min .. max of that over the
repeats; the spread of the staged chain's own repeats is the yardstick for the difference.  Both ways go through the ctypes
bindings, so both carry their Python overhead (the staged chain's reduce and disc list are vectorised NumPy).

    python tools/tracker_timing.py [--frames-file F.npz] [--repeats 4] [--warmup 4] [--out profiles/tracker_timing.log]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, FEATURES, MIN_DISTANCE, N_FRAMES = 752, 480, 300, 20, 16


def load_frames(path):
    z = np.load(path)
    return [(z["left"][k], z["right"][k]) for k in range(len(z["left"]))]


def make_frames(path):
    import flow_cases as fc
    frames = fc.sequence(N_FRAMES, W, H)
    np.savez(path, left=np.stack([f[0] for f in frames]), right=np.stack([f[1] for f in frames]))


def run_resident(frames, device):
    from visfs_amd import abi, backend, flow, tracker
    s = backend.Solver(abi.default_params()) if device else None
    f = flow.Flow(flow.default_params(), W, H, solver=s)
    t = tracker.Tracker(f, flow.camera(), max_features=FEATURES, min_distance=MIN_DISTANCE)
    ms, words = [], []
    for left, right in frames:
        t0 = time.perf_counter()
        out = t.process(left, right)
        ms.append((time.perf_counter() - t0) * 1e3)
        words.append((int(out["flags"]), len(out["covisible_id"]), len(out["new_id"]), len(out["word_id"])))
    t.close(); f.close()
    if s is not None:
        s.close()
    return ms, words


def run_staged(frames):
    """The staged chain with the bookkeeping of Tracker.cpp on the host, as tests/test_gpu_corners.py::_step and
    examples/tracker_step.cpp do it (bootstrap included, so the words are those of the resident call)."""
    from visfs_amd import abi, backend, corners, flow
    s = backend.Solver(abi.default_params())
    f = flow.Flow(flow.default_params(), W, H, solver=s)
    cam = flow.camera()
    ids = np.zeros(0, dtype=np.uint64); xy = np.zeros((0, 2), dtype=np.float32); cnt = np.zeros(0, dtype=np.int32)
    next_id, ms, words = 0, [], []
    for k, (left, right) in enumerate(frames):
        t0 = time.perf_counter()
        flags, n_kept, n_new = 0, 0, 0
        if k == 0:
            f.push_frame(left, right)
            flags = 1
        else:
            if len(ids) == 0:                                    # bootstrap on the pair pushed last (3-D not needed for the pixels)
                xy = corners.corners(f, max_corners=FEATURES, min_distance=float(MIN_DISTANCE))
                f.stereo(xy, cam)
                ids = np.arange(next_id, next_id + len(xy), dtype=np.uint64); cnt = np.zeros(len(xy), dtype=np.int32)
                next_id += len(xy)
                flags = 2
            f.push_frame(left, right)
            to, st, _ = f.track(xy)
            keep = (st == 1) & np.isfinite(to).all(axis=1) & (to[:, 0] >= 0) & (to[:, 0] < W) & (to[:, 1] >= 0) & (to[:, 1] < H)
            ids, xy, cnt = ids[keep], to[keep], cnt[keep]
            n_kept = len(ids)
            if n_kept < FEATURES:
                counted = np.flatnonzero(cnt > 0)
                order = counted[np.argsort(-cnt[counted], kind="stable")]
                discs = np.zeros(len(order), dtype=corners.DISC_DTYPE)
                discs["x"], discs["y"], discs["radius"] = xy[order, 0], xy[order, 1], MIN_DISTANCE
                new = corners.corners(f, discs=discs, max_corners=FEATURES - n_kept, min_distance=float(MIN_DISTANCE))
                n_new = len(new)
                ids = np.concatenate([ids, np.arange(next_id, next_id + n_new, dtype=np.uint64)])
                xy = np.concatenate([xy, new]); cnt = np.concatenate([cnt, np.zeros(n_new, dtype=np.int32)])
                next_id += n_new
            rt, st, xyz = f.stereo(xy, cam)
            ok = (st == 1) & (rt[:, 0] >= 0) & (rt[:, 0] < W) & (rt[:, 1] >= 0) & (rt[:, 1] < H) & np.isfinite(xyz).all(axis=1)
            ids, xy, cnt = ids[ok], xy[ok], cnt[ok] + 1
        ms.append((time.perf_counter() - t0) * 1e3)
        words.append((flags, n_kept, n_new, len(ids) if k else 0))
    f.close(); s.close()
    return ms, words


def child(role, frames_file):
    frames = load_frames(frames_file)
    if role == "resident":
        ms, words = run_resident(frames, True)
    elif role == "host":
        ms, words = run_resident(frames, False)
    else:
        ms, words = run_staged(frames)
    print("TRACKER_TIMING " + json.dumps(dict(role=role, ms=ms, words=words)))


def spawn(role, frames_file, lib):
    env = dict(os.environ)
    if lib:
        env["VISFS_BA_LIB"] = lib
    else:
        env.pop("VISFS_BA_LIB", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", role, "--frames-file", frames_file], env=env,
                         capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise RuntimeError(f"{role} child failed ({res.returncode}):\n{res.stderr[-2000:]}")
    line = [l for l in res.stdout.splitlines() if l.startswith("TRACKER_TIMING ")][-1]
    return json.loads(line[len("TRACKER_TIMING "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--frames-file", default=None)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.frames_file)
        return
    frames_file = a.frames_file
    if not frames_file:
        frames_file = os.path.join(tempfile.mkdtemp(), "tracker_frames.npz")
        make_frames(frames_file)
    staged_lib = os.environ.get("VISFS_BA_STAGED_LIB")
    runs = dict(resident=[], staged=[])
    for _ in range(a.repeats):
        runs["resident"].append(spawn("resident", frames_file, None))
        runs["staged"].append(spawn("staged", frames_file, staged_lib))
    host = spawn("host", frames_file, None)
    same_words = all(r["words"] == runs["resident"][0]["words"] for rs in runs.values() for r in rs) and host["words"] == runs["resident"][0]["words"]
    med = {k: [float(np.median(r["ms"][a.warmup:])) for r in rs] for k, rs in runs.items()}
    host_med = float(np.median(host["ms"][a.warmup:]))
    n_counted = len(host["ms"]) - a.warmup
    lines = [f"tracker_timing: {W} x {H}, {FEATURES} features, min distance {MIN_DISTANCE}, {len(host['ms'])} frames of a drifting texture, "
             f"the first {a.warmup} not counted; per child the median over {n_counted} frames, ms; {a.repeats} children per way, interleaved",
             f"staged chain on: {os.path.relpath(staged_lib, ROOT) if staged_lib else 'the library of this tree'}"]
    for k in ("resident", "staged"):
        m = med[k]
        lines.append(f"{k:<10} medians {[round(v, 3) for v in m]}  median {np.median(m):.3f}  min {min(m):.3f}  max {max(m):.3f}")
    lines.append(f"host twin  median {host_med:.3f} (one core, one run)")
    sp = (max(med["staged"]) - min(med["staged"])) / np.median(med["staged"]) * 100.0
    gain = (np.median(med["staged"]) - np.median(med["resident"])) / np.median(med["staged"]) * 100.0
    lines.append(f"spread of the staged chain's own repeats: {sp:.1f} % of its median; the resident call's median is {gain:.1f} % below the staged chain's")
    lines.append(f"word counts per frame (flags, kept, new, words) identical in every run: {same_words}; last frame {host['words'][-1]}")
    lines.append(json.dumps(dict(tool="tracker_timing", width=W, height=H, features=FEATURES, repeats=a.repeats, warmup=a.warmup,
                                 resident_ms=med["resident"], staged_ms=med["staged"], host_twin_ms=host_med, staged_spread_pct=sp,
                                 resident_below_staged_pct=gain, same_words=bool(same_words))))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
