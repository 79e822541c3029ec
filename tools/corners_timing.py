"""Corner extraction: visfs_flow_corners on one resident 752 x 480 image, without discs (max_corners 300) and behind the mask of the
mid-run scenario of tests/corners_cases.py, on the GPU and on the host twin (one core) of the same machine.  Median of --calls calls
after --warmup warm-ups of the same shapes; every GPU time is a host clock around a call that ends in a device synchronise, and the
default call count keeps the timed window at a good fraction of a second.  Prints a table and one JSON line (and --out FILE).

    python tools/corners_timing.py [--calls 2000] [--host-calls 20] [--warmup 20] [--out profiles/corners_timing.log]
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
from visfs_amd import corners, flow  # noqa: E402
import corners_cases as cc  # noqa: E402
import flow_cases as fc  # noqa: E402


def measure(f, discs, params, calls, warmup):
    """(median, min, max in ms, seconds timed, corners) of the C call alone: the arguments are marshalled once."""
    import ctypes as C
    lib = corners.load()
    p = corners.default_params(**params)
    d = corners.make_discs(discs)
    xy = np.zeros((p.max_corners, 2), dtype=np.float32)
    n = C.c_int32(0)
    args = (f.h, corners.SLOT_CURRENT, corners.IMAGE_LEFT, C.byref(p), len(d), d.ctypes.data if len(d) else None, p.max_corners,
            xy.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n))
    t = []
    for i in range(calls + warmup):
        t0 = time.perf_counter()
        rc = lib.visfs_flow_corners(*args)
        t1 = time.perf_counter()
        assert rc == abi.OK, f.last_error()
        if i >= warmup:
            t.append(t1 - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3, float(np.sum(t)), xy[:n.value].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = 752, 480
    img = fc.base_image(w, h)
    cases = [("no discs, max_corners 300", None, dict(max_corners=300, min_distance=40.0)),
             ("mask scenario, max_corners 204", cc.mask_scenario(w, h), dict(max_corners=204, min_distance=40.0)),
             ("no discs, min_distance 7", None, dict(max_corners=300, min_distance=7.0))]
    s = backend.Solver(abi.default_params())                  # raises without a GPU: there is no number to report then
    dev = flow.Flow(flow.default_params(), w, h, solver=s)
    host = flow.Flow(flow.default_params(), w, h)
    dev.push_frame(img, img)
    host.push_frame(img, img)
    lines = [f"corners_timing: {w} x {h}, quality_level 0.01; median (min .. max) ms of {a.calls} GPU calls / {a.host_calls} host-twin calls after "
             f"warm-ups of the same shapes; host twin: one core of the same machine",
             f"{'case':<34}{'GPU':>30}{'host twin':>32}{'corners':>9}{'candidates':>12}  identical"]
    record = {}
    for name, discs, params in cases:
        g = measure(dev, discs, params, a.calls, a.warmup)
        nc = corners.download(dev)["n_candidates"]
        c = measure(host, discs, params, a.host_calls, 2)
        same = g[4].tobytes() == c[4].tobytes()
        lines.append(f"{name:<34}{g[0]:>10.4f} ({g[1]:.4f} .. {g[2]:.4f}){c[0]:>14.3f} ({c[1]:.3f} .. {c[2]:.3f}){len(g[4]):>9}{nc:>12}  {same}")
        lines.append(f"{'':<34}  timed window: GPU {g[3]:.3f} s, host twin {c[3]:.3f} s")
        record[name] = dict(gpu_ms_median=g[0], host_1core_ms_median=c[0], corners=len(g[4]), candidates=nc, identical=bool(same),
                            gpu_timed_s=g[3])
    lines.append(json.dumps(dict(tool="corners_timing", width=w, height=h, calls=a.calls, warmup=a.warmup, cases=record)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dev.close(); host.close(); s.close()


if __name__ == "__main__":
    main()
