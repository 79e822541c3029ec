"""PnP-RANSAC pose guess: visfs_pnp_solve on 300 correspondences (40 % outliers, the first case of tests/pnp_cases.py) at 50 and at
1024 hypotheses, on the GPU and on the host twin (one core) of the same machine.  Median of --calls calls after --warmup warm-ups of
the same shapes; every GPU time is a host clock around a call that ends in a device synchronise.  Prints a table and one JSON line
(and --out FILE).

    python tools/pnp_timing.py [--calls 2000] [--host-calls 20] [--warmup 20] [--out profiles/pnp_timing.log]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend, pnp  # noqa: E402
import pnp_cases as pc  # noqa: E402


def measure(obj, s, params, calls, warmup):
    """(median, min, max in ms, seconds timed, result bytes) of the C call alone: the arguments are marshalled once."""
    lib = pnp.load()
    p = pnp.default_params(**params)
    cam = pnp.camera(*pc.K, Tir=pc.TIR)
    a, b, c = (np.ascontiguousarray(s[k], dtype=np.float32) for k in ("from_xyz", "to_xy", "to_xyz"))
    n = len(a)
    T, cov = np.zeros(16), np.zeros(36)
    matches, inliers = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    nm, ni = C.c_int32(), C.c_int32()
    pf, pd, pi = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    args = (obj.h, C.byref(p), C.byref(cam), n, a.ctypes.data_as(pf), b.ctypes.data_as(pf), c.ctypes.data_as(pf), T.ctypes.data_as(pd),
            cov.ctypes.data_as(pd), matches.ctypes.data_as(pi), C.byref(nm), inliers.ctypes.data_as(pi), C.byref(ni))
    t = []
    for i in range(calls + warmup):
        t0 = time.perf_counter()
        rc = lib.visfs_pnp_solve(*args)
        t1 = time.perf_counter()
        assert rc == abi.OK, obj.last_error()
        if i >= warmup:
            t.append(t1 - t0)
    sig = T.tobytes() + cov.tobytes() + inliers[:ni.value].tobytes()
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3, float(np.sum(t)), sig, ni.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = pc.case("m300_out40")
    solver = backend.Solver(abi.default_params())                  # raises without a GPU: there is no number to report then
    dev, host = pnp.Pnp(pnp.MAX_POINTS, solver=solver), pnp.Pnp(pnp.MAX_POINTS)
    lines = [f"pnp_timing: 300 rows, 40 % outliers, to_xyz given; median (min .. max) ms of {a.calls} GPU calls / {a.host_calls} host-twin calls "
             f"after warm-ups of the same shapes; host twin: one core of the same machine",
             f"{'case':<22}{'GPU':>30}{'host twin':>32}{'inliers':>9}{'passes':>8}  identical"]
    record = {}
    for iterations in (50, 1024):
        params = dict(s["params"], iterations=iterations)
        g = measure(dev, s, params, a.calls, a.warmup)
        passes = len(dev.download()["pass_count"])
        c = measure(host, s, params, a.host_calls, 2)
        same = g[4] == c[4]
        name = f"{iterations} hypotheses"
        lines.append(f"{name:<22}{g[0]:>10.4f} ({g[1]:.4f} .. {g[2]:.4f}){c[0]:>14.3f} ({c[1]:.3f} .. {c[2]:.3f}){g[5]:>9}{passes:>8}  {same}")
        lines.append(f"{'':<22}  timed window: GPU {g[3]:.3f} s, host twin {c[3]:.3f} s")
        record[name] = dict(gpu_ms_median=g[0], host_1core_ms_median=c[0], inliers=g[5], passes=passes, identical=bool(same), gpu_timed_s=g[3])
    lines.append(json.dumps(dict(tool="pnp_timing", rows=300, calls=a.calls, warmup=a.warmup, cases=record)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dev.close(); host.close(); solver.close()


if __name__ == "__main__":
    main()
