#!/usr/bin/env python3
"""Times the pose graph's covariances (include/visfs_pose_graph_cov.h): one visfs_pose_graph_covariance call on the device against
the same call on the one-core host twin, at N = 512, 2048 and 4096 vertices with k = 8 closures and 1, 8 and 64 sources, default
parameters, the two alternating in one process.  A row is reported only if the device and the twin returned the same bytes (record,
joint, relative); otherwise the tool stops.  Medians of 5.  Writes profiles/pose_graph_cov_timing.log.

usage: tools/pose_graph_cov_timing.py [--repeats R]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                 # noqa: E402

import pose_graph_cases as pc                      # noqa: E402
from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import pose_graph as pg             # noqa: E402
from visfs_amd import pose_graph_cov as pgc        # noqa: E402


def queries(N, sources):
    """pairs over `sources` free vertices spread evenly over the trajectory (vertex 0 is held)"""
    v = [int(a) for a in np.linspace(1, N - 1, sources).round()] if sources > 1 else [N - 1]
    return [(v[k], v[k + 1]) for k in range(len(v) - 1)] or [(v[0], v[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    solver = backend.Solver(abi.default_params())
    dev, host = pg.PoseGraph(solver), pg.PoseGraph()
    lines = ["# tools/pose_graph_cov_timing.py: median wall time of one visfs_pose_graph_covariance (default parameters), device and twin alternating",
             "# N k sources columns pcg_iterations_max pcg_iterations_total unconverged device_ms twin_ms twin_over_device device_us_per_iteration_of_the_slowest_column"]
    for N in (512, 2048, 4096):
        c = pc.make("timing", N, k=8, seed=108)
        edges = pg.make_edges(c["edges"])
        for sources in (1, 8, 64):
            q = queries(N, sources)
            times = {"device": [], "twin": []}
            last = {}
            for rep in range(args.repeats + 1):                             # the first round warms both up (and makes the arena)
                for name, g in (("device", dev), ("twin", host)):
                    t0 = time.perf_counter()
                    rc, r = pgc.covariance(g, c["poses"], c["fixed"], edges, q)
                    dt = time.perf_counter() - t0
                    if rc != abi.OK:
                        sys.exit(f"{name}: status {rc}: {g.last_error()}")
                    if rep:
                        times[name].append(dt)
                    last[name] = (r["bytes"], r["joint"].tobytes(), r["relative"].tobytes(), r)
                if last["device"][:3] != last["twin"][:3]:
                    sys.exit(f"N = {N}, sources = {sources}: the device and the twin differ; nothing is reported")
            r = last["device"][3]
            assert r["sources"] == sources
            d, t = statistics.median(times["device"]) * 1e3, statistics.median(times["twin"]) * 1e3
            lines.append(f"{N} 8 {sources} {r['columns']} {r['pcg_iterations_max']} {r['pcg_iterations_total']} {r['unconverged_columns']} {d:.3f} {t:.3f} "
                         f"{t / d:.2f} {1e3 * d / max(r['pcg_iterations_max'], 1):.1f}")
            print(lines[-1], flush=True)
    dev.close(); host.close(); solver.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_graph_cov_timing.log"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
