"""One frame of the image front end with Tracker/FlowBack off at 752 x 480 with 300 features, three ways over the same frames:

  A  resident + cull   visfs_tracker_process with cull = 1 at --iterations hypotheses, this tree's library
  B  resident          the same call with cull = 0, this tree's library: A - B is what the cull adds inside the call
  C  staged + cull     what a caller had before: push_frame -> track -> visfs_fund_cull -> host reduce -> corners behind the host-made
                       discs -> stereo -> host erase and track counts, on the library VISFS_BA_STAGED_LIB names (the parent commit's
                       build, tools/build_variant.sh parent; default: this tree's)

Each way runs in a child process of its own (a process loads one library), --repeats children per way, interleaved (A, B, C, A, ...).
A child runs the whole sequence once; the first --warmup frames (no previous pair, the bootstrap, first steady frames) are not
counted.  Before a time is reported the words of A and C (ids, left pixels, track counts of every frame) are compared through a
digest.  Reported: the median over a child's frames, then median and min .. max of that over the repeats; the spread of C's own
repeats is the yardstick for A against C.

    python tools/tracker_cull_timing.py [--repeats 4] [--warmup 4] [--iterations 1000] [--out profiles/tracker_cull_timing.log]
"""
import argparse
import hashlib
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


def digest(ids, xy, cnt):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(ids, dtype=np.uint64).tobytes())
    h.update(np.ascontiguousarray(xy, dtype=np.float32).tobytes())
    h.update(np.ascontiguousarray(cnt, dtype=np.int32).tobytes())
    return h.hexdigest()[:16]


def run_resident(frames, cull, iterations):
    from visfs_amd import abi, backend, flow, fund, tracker
    s = backend.Solver(abi.default_params())
    f = flow.Flow(flow.default_params(flow_back=0), W, H, solver=s)
    t = tracker.Tracker(f, flow.camera(), tracker.default_params(max_features=FEATURES, min_distance=MIN_DISTANCE, cull=1 if cull else 0,
                                                                 cull_params=fund.default_params(iterations=iterations)))
    ms, words = [], []
    for left, right in frames:
        t0 = time.perf_counter()
        out = t.process(left, right)
        ms.append((time.perf_counter() - t0) * 1e3)
        words.append((int(out["flags"]), len(out["covisible_id"]), len(out["new_id"]), len(out["word_id"]),
                      digest(out["word_id"], out["word_left_xy"], out["word_count"])))
    t.close(); f.close(); s.close()
    return ms, words


def run_staged(frames, iterations):
    """The staged chain with the bookkeeping of Tracker.cpp on the host, as tools/tracker_timing.py has it, with the staged cull
    between the track and the reduce (Tracker.cpp:275-277)."""
    from visfs_amd import abi, backend, corners, flow, fund
    s = backend.Solver(abi.default_params())
    f = flow.Flow(flow.default_params(flow_back=0), W, H, solver=s)
    fd = fund.Fund(FEATURES, solver=s)
    fp = fund.default_params(iterations=iterations)
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
            st = fd.cull(fp, xy, to, st)["status"]
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
        words.append((flags, n_kept, n_new, len(ids) if k else 0, digest(ids if k else [], xy if k else np.zeros((0, 2)), cnt if k else [])))
    fd.close(); f.close(); s.close()
    return ms, words


def child(role, frames_file, iterations):
    frames = load_frames(frames_file)
    if role == "A":
        ms, words = run_resident(frames, True, iterations)
    elif role == "B":
        ms, words = run_resident(frames, False, iterations)
    else:
        ms, words = run_staged(frames, iterations)
    print("TRACKER_CULL_TIMING " + json.dumps(dict(role=role, ms=ms, words=words)))


def spawn(role, frames_file, lib, iterations):
    env = dict(os.environ)
    if lib:
        env["VISFS_BA_LIB"] = lib
    else:
        env.pop("VISFS_BA_LIB", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", role, "--frames-file", frames_file, "--iterations",
                          str(iterations)], env=env, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise RuntimeError(f"{role} child failed ({res.returncode}):\n{res.stderr[-2000:]}")
    line = [l for l in res.stdout.splitlines() if l.startswith("TRACKER_CULL_TIMING ")][-1]
    return json.loads(line[len("TRACKER_CULL_TIMING "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--frames-file", default=None)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.frames_file, a.iterations)
        return
    frames_file = a.frames_file
    if not frames_file:
        frames_file = os.path.join(tempfile.mkdtemp(), "tracker_cull_frames.npz")
        make_frames(frames_file)
    staged_lib = os.environ.get("VISFS_BA_STAGED_LIB")
    runs = dict(A=[], B=[], C=[])
    for _ in range(a.repeats):
        runs["A"].append(spawn("A", frames_file, None, a.iterations))
        runs["B"].append(spawn("B", frames_file, None, a.iterations))
        runs["C"].append(spawn("C", frames_file, staged_lib, a.iterations))
    same_ac = all(r["words"] == runs["A"][0]["words"] for k in ("A", "C") for r in runs[k])
    same_b = all(r["words"] == runs["B"][0]["words"] for r in runs["B"])
    if not same_ac:
        bad = next((k, x, y) for k, (x, y) in enumerate(zip(runs["A"][0]["words"], runs["C"][0]["words"])) if x != y) \
            if runs["A"][0]["words"] != runs["C"][0]["words"] else "between repeats"
        raise SystemExit(f"the words of A and C differ ({bad}): no time is reported")
    med = {k: [float(np.median(r["ms"][a.warmup:])) for r in rs] for k, rs in runs.items()}
    mm = {k: float(np.median(v)) for k, v in med.items()}
    n_counted = len(runs["A"][0]["ms"]) - a.warmup
    names = dict(A=f"A resident + cull ({a.iterations})", B="B resident, cull off", C="C staged + cull")
    lines = [f"tracker_cull_timing: {W} x {H}, {FEATURES} features, min distance {MIN_DISTANCE}, flow_back 0, {len(runs['A'][0]['ms'])} frames of "
             f"a drifting texture, the first {a.warmup} not counted; per child the median over {n_counted} frames, ms; {a.repeats} children "
             f"per way, interleaved",
             f"staged chain on: {os.path.relpath(staged_lib, ROOT) if staged_lib else 'the library of this tree'}"]
    for k in ("A", "B", "C"):
        m = med[k]
        lines.append(f"{names[k]:<28} medians {[round(v, 3) for v in m]}  median {mm[k]:.3f}  min {min(m):.3f}  max {max(m):.3f}")
    sp = (max(med["C"]) - min(med["C"])) / mm["C"] * 100.0
    gain = (mm["C"] - mm["A"]) / mm["C"] * 100.0
    lines.append(f"A - B (the rows kernel, the search and the mask inside the call): {mm['A'] - mm['B']:.3f} ms")
    lines.append(f"spread of C's own repeats: {sp:.1f} % of its median; A's median is {gain:.1f} % below C's")
    lines.append(f"words of every frame (flags, kept, new, words, digest of ids / left pixels / counts) identical in A and C and in every "
                 f"repeat: {same_ac}; B identical in its repeats: {same_b}; last frame of A {runs['A'][0]['words'][-1]}, of B {runs['B'][0]['words'][-1]}")
    lines.append(json.dumps(dict(tool="tracker_cull_timing", width=W, height=H, features=FEATURES, iterations=a.iterations, repeats=a.repeats,
                                 warmup=a.warmup, a_ms=med["A"], b_ms=med["B"], c_ms=med["C"], a_minus_b_ms=mm["A"] - mm["B"],
                                 c_spread_pct=sp, a_below_c_pct=gain, same_words_a_c=bool(same_ac))))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
