#!/usr/bin/env python3
"""Times the 2-D pose graph (include/visfs_pose_graph.h): one call on the device against the same call on the one-core host twin,
at N = 512, 2048 and 4096 vertices with k = 8 and k = 40 closures, the two alternating in one process.  A row is reported only if
the device and the twin returned the same bytes (record, poses, chi2, trace); otherwise the tool stops.  Writes
profiles/pose_graph_timing.log.

usage: tools/pose_graph_timing.py [--repeats R]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pose_graph_cases as pc                      # noqa: E402
from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import pose_graph as pg             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    solver = backend.Solver(abi.default_params())
    dev, host = pg.PoseGraph(solver), pg.PoseGraph()
    lines = ["# tools/pose_graph_timing.py: median wall time of one visfs_pose_graph_optimize (default parameters), device and twin alternating",
             "# N k edges iterations trials pcg_iterations termination device_ms twin_ms device_us_per_pcg_iteration"]
    for N in (512, 2048, 4096):
        for k in (8, 40):
            c = pc.make("timing", N, k=k, seed=100 + k)
            edges = pg.make_edges(c["edges"])
            times = {"device": [], "twin": []}
            last = {}
            for rep in range(args.repeats + 1):                             # the first round warms both up
                for name, g in (("device", dev), ("twin", host)):
                    t0 = time.perf_counter()
                    rc, r = g.optimize(c["poses"], c["fixed"], edges)
                    dt = time.perf_counter() - t0
                    if rc != abi.OK:
                        sys.exit(f"{name}: status {rc}: {g.last_error()}")
                    if rep:
                        times[name].append(dt)
                    last[name] = (r["bytes"], r["poses"].tobytes(), r["chi2"].tobytes(), g.trace().tobytes(), r)
                if last["device"][:4] != last["twin"][:4]:
                    sys.exit(f"N = {N}, k = {k}: the device and the twin differ; nothing is reported")
            r = last["device"][4]
            d, t = statistics.median(times["device"]) * 1e3, statistics.median(times["twin"]) * 1e3
            lines.append(f"{N} {k} {len(c['edges'])} {r['iterations']} {r['trials']} {r['pcg_iterations']} {r['termination']} {d:.3f} {t:.3f} "
                         f"{1e3 * d / max(r['pcg_iterations'], 1):.1f}")
            print(lines[-1], flush=True)
    dev.close(); host.close(); solver.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_graph_timing.log"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
