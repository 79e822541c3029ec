"""Lucas-Kanade front end: push_frame, track and stereo of one 752 x 480 frame with 300 points on the GPU and on the host twin (one
core) of the same machine.  Median of --calls calls after --warmup warm-ups; every GPU time is a host clock around a call that ends
in a device synchronise.  Prints a table and one JSON line (and --out FILE).

    python tools/flow_timing.py [--calls 20] [--warmup 3] [--out profiles/flow_timing.log]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend  # noqa: E402
from visfs_amd import flow  # noqa: E402
import flow_cases as fc  # noqa: E402

_hip = None


def sync():
    """hipDeviceSynchronize of the HIP runtime the library already loaded (push_frame only enqueues)."""
    global _hip
    if _hip is None:
        import ctypes
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
            try:
                _hip = ctypes.CDLL(name)
                break
            except OSError:
                continue
    assert _hip.hipDeviceSynchronize() == 0


def measure(f, frames, pts, cam, calls, warmup, device):
    t = dict(push_frame=[], track=[], stereo=[])
    f.push_frame(*frames[0])
    for i in range(calls + warmup):
        pair = frames[(i + 1) % 2]
        if device:
            sync()
        t0 = time.perf_counter(); f.push_frame(*pair)
        if device:
            sync()
        t1 = time.perf_counter(); tr = f.track(pts); t2 = time.perf_counter(); st = f.stereo(pts, cam); t3 = time.perf_counter()
        if i >= warmup:
            t["push_frame"].append(t1 - t0); t["track"].append(t2 - t1); t["stereo"].append(t3 - t2)
    return {k: (float(np.median(v)) * 1e3, float(np.min(v)) * 1e3, float(np.max(v)) * 1e3) for k, v in t.items()}, tr, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = 752, 480
    first = fc.base_image(w, h)
    left, right, _, _ = fc.moved_pair(w, h)
    frames = [(first, first), (left, right)]
    pts = fc.truth_points(w, h)
    cam = flow.camera()
    s = backend.Solver(abi.default_params())                  # raises without a GPU: there is no number to report then
    dev = flow.Flow(flow.default_params(), w, h, solver=s)
    host = flow.Flow(flow.default_params(), w, h)
    gpu, tr_d, st_d = measure(dev, frames, pts, cam, a.calls, a.warmup, True)
    cpu, tr_h, st_h = measure(host, frames, pts, cam, a.calls, a.warmup, False)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(tr_d + st_d, tr_h + st_h))
    lines = [f"flow_timing: {w} x {h}, {len(pts)} points, 21 x 21 window, 4 levels, <= 30 iterations, flow_back 1; median (min .. max) of {a.calls} "
             f"calls after {a.warmup} warm-ups, ms; host twin: one core of the same machine",
             f"{'call':<12}{'GPU':>28}{'host twin':>32}"]
    for k in ("push_frame", "track", "stereo"):
        lines.append(f"{k:<12}{gpu[k][0]:>10.3f} ({gpu[k][1]:.3f} .. {gpu[k][2]:.3f}){cpu[k][0]:>14.3f} ({cpu[k][1]:.3f} .. {cpu[k][2]:.3f})")
    lines.append(f"kept: track {int(tr_d[1].sum())}, stereo {int(st_d[1].sum())} of {len(pts)}; device and host twin identical: {same}")
    lines.append(json.dumps(dict(tool="flow_timing", width=w, height=h, points=len(pts), calls=a.calls, warmup=a.warmup,
                                 gpu_ms_median={k: gpu[k][0] for k in gpu}, host_1core_ms_median={k: cpu[k][0] for k in cpu},
                                 identical=bool(same))))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dev.close(); host.close(); s.close()


if __name__ == "__main__":
    main()
