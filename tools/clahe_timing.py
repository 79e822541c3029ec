"""The equalised frame push: push_frame_clahe next to plain push_frame of one 752 x 480 stereo pair on the GPU (the same object) and
on the host twin (one core) of the same machine, default parameters (clip limit 3, 8 x 8 tiles).  Median of --calls calls after
--warmup warm-ups; every GPU time is a host clock around a call that ends in a device synchronise.  Prints a table and one JSON
line (and --out FILE).

    python tools/clahe_timing.py [--calls 20] [--warmup 3] [--out profiles/clahe_timing.log]
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
from visfs_amd import clahe, flow  # noqa: E402
import flow_cases as fc  # noqa: E402

_hip = None


def sync():
    """hipDeviceSynchronize of the HIP runtime the library already loaded (the pushes only enqueue)."""
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


def measure(f, frames, prm, calls, warmup, device):
    t = dict(push_frame=[], push_frame_clahe=[])
    for i in range(calls + warmup):
        pair = frames[i % 2]
        for key in ("push_frame", "push_frame_clahe"):
            if device:
                sync()
            t0 = time.perf_counter()
            if key == "push_frame":
                f.push_frame(*pair)
            else:
                clahe.push_frame(f, prm, *pair)
            if device:
                sync()
            if i >= warmup:
                t[key].append(time.perf_counter() - t0)
    return {k: (float(np.median(v)) * 1e3, float(np.min(v)) * 1e3, float(np.max(v)) * 1e3) for k, v in t.items()}


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
    prm = clahe.default_params()
    s = backend.Solver(abi.default_params())                  # raises without a GPU: there is no number to report then
    dev = flow.Flow(flow.default_params(), w, h, solver=s)
    host = flow.Flow(flow.default_params(), w, h)
    gpu = measure(dev, frames, prm, a.calls, a.warmup, True)
    cpu = measure(host, frames, prm, a.calls, a.warmup, False)
    same = all(dev.download_level(flow.SLOT_CURRENT, i, l)[k].tobytes() == host.download_level(flow.SLOT_CURRENT, i, l)[k].tobytes()
               for i in (0, 1) for l in range(4) for k in (0, 1))
    same = same and all(clahe.download(dev, i)[k].tobytes() == clahe.download(host, i)[k].tobytes() for i in (0, 1) for k in ("lut", "hist"))
    lines = [f"clahe_timing: {w} x {h} stereo pair, clip limit {prm.clip_limit:g}, {prm.tiles_x} x {prm.tiles_y} tiles, 4 pyramid levels; median "
             f"(min .. max) of {a.calls} calls after {a.warmup} warm-ups, ms; host twin: one core of the same machine",
             f"{'call':<18}{'GPU':>28}{'host twin':>32}"]
    for k in ("push_frame", "push_frame_clahe"):
        lines.append(f"{k:<18}{gpu[k][0]:>10.3f} ({gpu[k][1]:.3f} .. {gpu[k][2]:.3f}){cpu[k][0]:>14.3f} ({cpu[k][1]:.3f} .. {cpu[k][2]:.3f})")
    lines.append(f"device and host twin identical (tables, histograms, every level and derivative): {same}")
    lines.append(json.dumps(dict(tool="clahe_timing", width=w, height=h, calls=a.calls, warmup=a.warmup,
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
