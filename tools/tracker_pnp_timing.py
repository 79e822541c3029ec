"""One frame of the image front end with the pose guess at 752 x 480 with 300 features, three ways over the same frames, for one
tracker and for groups of --members trackers:

  A  resident + pnp    visfs_tracker_process / visfs_tracker_group_process with the pose guess enabled at
                       --iterations hypotheses and --refine passes, then visfs_tracker_pnp_last per member; this tree's library
  B  resident          the same call without it, this tree's library: A - B is what the pose guess adds inside the call
  C  resident + staged the same call without it, followed by one staged visfs_pnp_solve per member on the covisible rows it handed
                       out (one solver object, the members in sequence), on the library VISFS_BA_STAGED_LIB names (the parent
                       commit's build, tools/build_variant.sh parent; default: this tree's)

C passes to_xyz = NULL, as examples/frame_step.cpp does, so it does not pay for the id matching in Python; the transform and the
inliers do not depend on to_xyz.  Each way runs in a child process of its own (a process loads one library), --repeats children per
way, interleaved (A, B, C, A, ...).  A child runs the whole sequence once; the first --warmup frames (no previous pair, the
bootstrap, first steady frames) are not counted.  Before a time is reported A and C are compared through a digest of T, the inlier
ids and the word ids of every member and frame.  Reported: the median over a child's frames, then median and min .. max of that
over the repeats; the spread of C's own repeats is the yardstick for A against C.

    python tools/tracker_pnp_timing.py [--members 1,4,16] [--repeats 4] [--warmup 4] [--out profiles/tracker_pnp_timing.log]

--host runs every way on the one-core host twins (no device): its times say nothing about the device, it is there to check the tool
and the agreement of A and C.
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
TAG = "TRACKER_PNP_TIMING "


def load_frames(path):
    z = np.load(path)
    return [(z["left"][k], z["right"][k]) for k in range(len(z["left"]))]


def make_frames(path):
    import flow_cases as fc
    frames = fc.sequence(N_FRAMES, W, H)
    np.savez(path, left=np.stack([f[0] for f in frames]), right=np.stack([f[1] for f in frames]))


def digest(T, inlier_ids, word_ids):
    h = hashlib.sha1()
    h.update(np.ascontiguousarray(T, dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(inlier_ids, dtype=np.uint64).tobytes())
    h.update(np.ascontiguousarray(word_ids, dtype=np.uint64).tobytes())
    return h.hexdigest()[:16]


def run(role, frames, n, iterations, refine, host=False):
    from visfs_amd import abi, backend, flow, pnp, tracker
    tracker.load(require_group=True)
    s = None if host else backend.Solver(abi.default_params())
    flows = [flow.Flow(flow.default_params(), W, H, solver=s) for _ in range(n)]
    trks = [tracker.Tracker(f, flow.camera(), tracker.default_params(max_features=FEATURES, min_distance=MIN_DISTANCE)) for f in flows]
    prm = pnp.default_params(iterations=iterations, refine_iterations=refine)
    staged, cam = None, None
    if role == "A":
        from visfs_amd import tracker_pnp
        for t in trks:
            tracker_pnp.enable(t, prm)
    elif role == "C":
        staged = pnp.Pnp(FEATURES, solver=s)
        c = flow.camera()
        cam = pnp.camera(fx=float(c.fx), fy=float(c.fy), cx=float(c.cx), cy=float(c.cy), Tir=list(c.Tir))
    group = tracker.TrackerGroup(trks) if n > 1 else None
    ms, marks = [], []
    for left, right in frames:
        t0 = time.perf_counter()
        outs = group.process([(left, right)] * n) if group is not None else [trks[0].process(left, right)]
        poses = []
        if role == "A":
            poses = [tracker_pnp.last(t) for t in trks]
        elif role == "C":
            poses = [staged.solve(prm, cam, o["covisible_from_xyz"], o["covisible_to_xy"]) if not (o["flags"] & tracker.NO_PREVIOUS) else None
                     for o in outs]
        ms.append((time.perf_counter() - t0) * 1e3)
        mark = []
        for i, o in enumerate(outs):
            p = poses[i] if poses else None
            if p is None or (role == "A" and not p["ran"]):
                mark.append((int(o["flags"]), len(o["word_id"]), 0, digest(np.zeros((4, 4)), [], o["word_id"])))
            else:
                mark.append((int(o["flags"]), len(o["word_id"]), len(p["inliers"]), digest(p["T"], o["covisible_id"][p["inliers"]], o["word_id"])))
        marks.append(mark)
    if group is not None:
        group.close()
    if staged is not None:
        staged.close()
    for t in trks:
        t.close()
    for f in flows:
        f.close()
    if s is not None:
        s.close()
    return ms, marks


def child(a):
    ms, marks = run(a.child, load_frames(a.frames_file), a.n, a.iterations, a.refine, a.host)
    print(TAG + json.dumps(dict(role=a.child, ms=ms, marks=marks)))


def spawn(role, frames_file, lib, n, a):
    env = dict(os.environ)
    if lib:
        env["VISFS_BA_LIB"] = lib
    else:
        env.pop("VISFS_BA_LIB", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", role, "--frames-file", frames_file, "--n", str(n), "--iterations",
                          str(a.iterations), "--refine", str(a.refine)] + (["--host"] if a.host else []), env=env, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise RuntimeError(f"{role} child failed ({res.returncode}):\n{res.stderr[-2000:]}")
    line = [l for l in res.stdout.splitlines() if l.startswith(TAG)][-1]
    return json.loads(line[len(TAG):])


def measure(n, frames_file, staged_lib, a):
    runs = dict(A=[], B=[], C=[])
    for _ in range(a.repeats):
        runs["A"].append(spawn("A", frames_file, None, n, a))
        runs["B"].append(spawn("B", frames_file, None, n, a))
        runs["C"].append(spawn("C", frames_file, staged_lib, n, a))
    same_ac = all(r["marks"] == runs["A"][0]["marks"] for k in ("A", "C") for r in runs[k])
    if not same_ac:
        raise SystemExit(f"members {n}: T, inliers or words of A and C differ: no time is reported")
    med = {k: [float(np.median(r["ms"][a.warmup:])) for r in rs] for k, rs in runs.items()}
    mm = {k: float(np.median(v)) for k, v in med.items()}
    names = dict(A=f"A resident + pnp ({a.iterations}, {a.refine})", B="B resident, pnp off", C=f"C resident + {n} staged solve(s)")
    lines = [f"members {n}:"]
    for k in ("A", "B", "C"):
        m = med[k]
        lines.append(f"  {names[k]:<34} medians {[round(v, 3) for v in m]}  median {mm[k]:.3f}  min {min(m):.3f}  max {max(m):.3f}")
    sp_ms = max(med["C"]) - min(med["C"])
    gap = mm["C"] - mm["A"]
    verdict = "A below C by more than C's spread" if gap > sp_ms else ("level (the difference is inside C's spread)" if abs(gap) <= sp_ms else "A ABOVE C")
    lines.append(f"  A - B (rows kernel, search, refinement, larger download, host finalize): {mm['A'] - mm['B']:.3f} ms")
    lines.append(f"  C - A: {gap:.3f} ms; spread of C's own repeats (max - min): {sp_ms:.3f} ms: {verdict}")
    lines.append(f"  last frame of A, member 0: {runs['A'][0]['marks'][-1][0]}")
    return lines, dict(members=n, a_ms=med["A"], b_ms=med["B"], c_ms=med["C"], a_minus_b_ms=mm["A"] - mm["B"], c_minus_a_ms=gap,
                       c_spread_ms=sp_ms, same_a_c=bool(same_ac))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--frames-file", default=None)
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--members", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--refine", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    frames_file = a.frames_file
    if not frames_file:
        frames_file = os.path.join(tempfile.mkdtemp(), "tracker_pnp_frames.npz")
        make_frames(frames_file)
    staged_lib = os.environ.get("VISFS_BA_STAGED_LIB")
    lines = [f"tracker_pnp_timing{' ON THE HOST TWINS (not a device measurement)' if a.host else ''}: {W} x {H}, {FEATURES} features, min distance {MIN_DISTANCE}, {N_FRAMES} frames of a drifting texture, the "
             f"first {a.warmup} not counted; per child the median over {N_FRAMES - a.warmup} frames, ms; {a.repeats} children per way, interleaved",
             f"staged solves on: {os.path.relpath(staged_lib, ROOT) if staged_lib else 'the library of this tree'}"]
    records = []
    for n in [int(v) for v in a.members.split(",")]:
        more, rec = measure(n, frames_file, staged_lib, a)
        lines += more
        records.append(rec)
        print("\n".join(more), flush=True)
    lines.append(json.dumps(dict(tool="tracker_pnp_timing", width=W, height=H, features=FEATURES, iterations=a.iterations, refine=a.refine,
                                 repeats=a.repeats, warmup=a.warmup, runs=records)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
