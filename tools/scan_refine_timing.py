"""Scan refinement: the device refinement against the one-core twin, and visfs_scan_group_match_refine against
visfs_scan_group_match followed by m visfs_scan_stack_refine calls, on the same library in the same process, alternating (each side
timed up to the return of its last call, every call ending in its own stream wait).

Workloads, each measured in a child process of its own under a time limit:
  single n   the `room` of tools/scan_match_timing.py frozen as a stack; a scan of n = 360 and of n = 16384 returns refined from a
             pose a fraction of a cell off the truth: device stack against host stack;
  group m    the room of tools/scan_group_timing.py (1 000 returns, 1.6 m / 0.5 rad), m = 1, 4, 16, 64 stacks of the same sub-map.
Nothing is reported unless the records (and for the single workloads the traces) of both sides are equal byte for byte.  Writes one
JSON line per workload.

    python tools/scan_refine_timing.py [--repeats 20] [--out profiles/scan_refine_timing.log]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEPTH = 7
WORKLOADS = [("single", 360), ("single", 16384), ("group", 1), ("group", 4), ("group", 16), ("group", 64)]


def stats(ts):
    v = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), repeats=len(ts))


def plain(r):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k != "bytes"}


def child_single(n, repeats):
    import scan_fast_timing as sft
    import scan_match_cases as cases
    from visfs_amd import abi, backend
    from visfs_amd import scan_refine as sr
    s = backend.Solver(abi.default_params())
    dev, host, _, _ = sft.submaps_of("room", s)
    sd, sh = dev.freeze(0, DEPTH), host.freeze(0, DEPTH)
    assert sd.status == sh.status == abi.OK
    pts = cases.cast(cases.TRUTH, n, np.random.default_rng(3))
    start = (cases.TRUTH[0] + 0.021, cases.TRUTH[1] - 0.017, cases.TRUTH[2] + 0.004)
    target = cases.TRUTH[:2]
    t_dev, rd = sft.timed(lambda: sd.refine(start, target, pts), repeats)
    t_host, rh = sft.timed(lambda: sh.refine(start, target, pts), max(3, repeats // 4))
    out = dict(tool="scan_refine_timing", workload="single", points=n, lanes=sr.LANES)
    if rd[0] != abi.OK or rh[0] != abi.OK or rd[1]["bytes"] != rh[1]["bytes"] or sr.stack_trace(sd).tobytes() != sr.stack_trace(sh).tobytes():
        print(json.dumps(dict(out, error="the device and the twin disagree", device=plain(rd[1]), twin=plain(rh[1]))))
        return 2
    r = rd[1]
    out.update(identical=True, iterations=r["iterations"], trials=r["trials"], termination=r["termination"], initial_cost=r["initial_cost"],
               final_cost=r["final_cost"], device=stats(t_dev), twin=stats(t_host))
    print(json.dumps(out))
    sd.close(); sh.close(); dev.close(); host.close(); s.close()
    return 0


def child_group(m, repeats):
    import scan_fast_timing as sft
    from visfs_amd import abi, backend
    from visfs_amd import scan_fast as sf
    from visfs_amd import scan_group as sg
    from visfs_amd import scan_refine as sr
    s = backend.Solver(abi.default_params())
    dev, host, guess, pts = sft.submaps_of("room", s)
    host.close()
    stacks = [dev.freeze(0, DEPTH) for _ in range(m)]
    assert all(st.status == abi.OK for st in stacks), dev.last_error()
    group = sg.ScanStackGroup(stacks)
    assert group.status == abi.OK, sg.create_error()
    mp = sf.default_params(linear_search_window=1.6, angular_search_window=0.5, frontier_capacity=1 << 16)
    rp = sr.default_params()
    guesses = [(guess[0] + 0.05 * (i % 4), guess[1] - 0.05 * (i // 4 % 4), guess[2] + 0.002 * i) for i in range(m)]

    def fused():
        res, status, best, ref = group.match_refine(guesses, pts, mp, rp)
        assert group.rc == abi.OK and all(v == abi.OK for v in status), group.last_error()
        return res, ref

    def separate():
        res, status, best = group.match(guesses, pts, mp)
        assert group.rc == abi.OK and all(v == abi.OK for v in status), group.last_error()
        ref = []
        for st, g, w in zip(stacks, guesses, res):
            rc, r = st.refine((w["x"], w["y"], w["yaw"]), g[:2], pts, rp)
            assert rc == abi.OK and w["matched"] == 1, st.last_error()
            ref.append(r)
        return res, ref

    t_fused, t_sep = [], []
    for i in range(repeats + 2):
        t0 = time.perf_counter()
        rf = fused()
        t1 = time.perf_counter()
        counts = group.last_counts()
        t1b = time.perf_counter()
        rs = separate()
        t2 = time.perf_counter()
        if i >= 2:
            t_fused.append(t1 - t0); t_sep.append(t2 - t1b)
    out = dict(tool="scan_refine_timing", workload="group", members=m, depth=DEPTH, points=len(pts))
    for i in range(m):
        if rf[0][i] != rs[0][i] or rf[1][i]["bytes"] != rs[1][i]["bytes"]:
            print(json.dumps(dict(out, error=f"member {i}: the fused call and the separate calls disagree", fused=plain(rf[1][i]), separate=plain(rs[1][i]))))
            return 2
    out.update(identical=True, H=rf[0][0]["depth_used"] - 1, iterations=[r["iterations"] for r in rf[1]][:8], fused_counts=counts,
               match_refine=stats(t_fused), match_then_refines=stats(t_sep))
    print(json.dumps(out))
    group.close()
    for st in stacks:
        st.close()
    dev.close(); s.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--size", type=int, default=1)
    a = ap.parse_args()
    if a.child:
        sys.exit(child_single(a.size, a.repeats) if a.child == "single" else child_group(a.size, a.repeats))
    lines = []
    for name, size in WORKLOADS:
        res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--size", str(size),
                              "--repeats", str(a.repeats)], capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit(f"workload {name} {size} ended with status {res.returncode}: nothing reported")      # and nothing more is started
        lines.append(res.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
