"""Fundamental-matrix cull: visfs_fund_cull on 300 rows with 30 % displaced rows (the first case of tests/fund_cases.py) at 50 and at
1000 hypotheses, on the GPU and on the host twin (one core) of the same machine.  Median of --calls calls after --warmup warm-ups of
the same shapes; every GPU time is a host clock around a call that ends in a device synchronise.  Prints a table and one JSON line
(and --out FILE).

    python tools/fund_timing.py [--calls 2000] [--host-calls 20] [--warmup 20] [--out profiles/fund_timing.log]
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

from visfs_amd import abi, backend, fund  # noqa: E402
import fund_cases as fc  # noqa: E402


def measure(obj, s, params, calls, warmup):
    """(median, min, max in ms, seconds timed, result bytes, inliers) of the C call alone: the arguments are marshalled once."""
    lib = fund.load()
    p = fund.default_params(**params)
    a, b = (np.ascontiguousarray(s[k], dtype=np.float32) for k in ("from_xy", "to_xy"))
    st_in = np.ascontiguousarray(s["status"], dtype=np.uint8)
    n = len(a)
    st_out, mask, F = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(9)
    ni, ap = C.c_int32(), C.c_int32()
    pf, pd, pu = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    args = (obj.h, C.byref(p), n, a.ctypes.data_as(pf), b.ctypes.data_as(pf), st_in.ctypes.data_as(pu), st_out.ctypes.data_as(pu),
            mask.ctypes.data_as(pu), F.ctypes.data_as(pd), C.byref(ni), C.byref(ap))
    t = []
    for i in range(calls + warmup):
        t0 = time.perf_counter()
        rc = lib.visfs_fund_cull(*args)
        t1 = time.perf_counter()
        assert rc == abi.OK, obj.last_error()
        if i >= warmup:
            t.append(t1 - t0)
    sig = F.tobytes() + mask.tobytes() + st_out.tobytes()
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3, float(np.max(t)) * 1e3, float(np.sum(t)), sig, ni.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = fc.case("m300_out30")
    solver = backend.Solver(abi.default_params())                  # raises without a GPU: there is no number to report then
    dev, host = fund.Fund(fund.MAX_POINTS, solver=solver), fund.Fund(fund.MAX_POINTS)
    lines = [f"fund_timing: 300 rows, 30 % displaced, pixel_error 1.0; median (min .. max) ms of {a.calls} GPU calls / {a.host_calls} host-twin "
             f"calls after warm-ups of the same shapes; host twin: one core of the same machine",
             f"{'case':<22}{'GPU':>30}{'host twin':>32}{'inliers':>9}  identical"]
    record = {}
    for iterations in (50, 1000):
        params = dict(s["params"], iterations=iterations)
        g = measure(dev, s, params, a.calls, a.warmup)
        c = measure(host, s, params, a.host_calls, 2)
        same = g[4] == c[4]
        name = f"{iterations} hypotheses"
        lines.append(f"{name:<22}{g[0]:>10.4f} ({g[1]:.4f} .. {g[2]:.4f}){c[0]:>14.3f} ({c[1]:.3f} .. {c[2]:.3f}){g[5]:>9}  {same}")
        lines.append(f"{'':<22}  timed window: GPU {g[3]:.3f} s, host twin {c[3]:.3f} s")
        record[name] = dict(gpu_ms_median=g[0], host_1core_ms_median=c[0], inliers=g[5], identical=bool(same), gpu_timed_s=g[3])
    lines.append(json.dumps(dict(tool="fund_timing", rows=300, calls=a.calls, warmup=a.warmup, cases=record)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    dev.close(); host.close(); solver.close()


if __name__ == "__main__":
    main()
