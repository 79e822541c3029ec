"""Correlative scan matching: one call on the GPU (call + its one stream wait) against the one-core host twin on the same machine.

Two workloads, each measured in a child process of its own under a time limit:
  hall   the scene of tools/submap_timing.py: ~1 000 returns over 360 degrees in a 70 m x 50 m hall (ranges capped at 30 m), sub-maps
         grown past 1600 x 1600 cells, Cartographer's default windows (0.1 m, 20 degrees): S ~ 420 rotations, L^2 = 25 offsets;
  room   the 5 m room of tests/scan_match_cases.py, 1 000 returns, windows 0.3 m / 0.54 rad: S ~ 70, L^2 = 169.
Nothing is reported unless both paths agree on the winner, every Q and every score bit.  Writes one JSON line per workload.

    python tools/scan_match_timing.py [--repeats 50] [--out profiles/scan_match_timing.log]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(name):
    """(frames [(Twr, [range data])], guess, points, params) of a workload."""
    from visfs_amd import scan_match as scm
    if name == "hall":
        from test_gpu_submap import pose, room_scan
        room = (-35.0, 35.0, -25.0, 25.0)
        rng = np.random.default_rng(1)
        frames = []
        for x, y in ((-30, -20), (30, 20), (-30, 20), (30, -20), (0, 0), (10, 0), (9, 2)):
            T = pose(x, y, 0.0)
            frames.append((T, [room_scan(T, room, 1000, rng, n_miss=5)]))
        truth = (10 * math.cos(0.3), 8 * math.sin(0.3), 0.3)
        pts = room_scan(pose(*truth), room, 1000, rng, n_miss=0)[1]
        return frames, (truth[0] + 0.06, truth[1] - 0.05, truth[2] + 0.1), pts, scm.default_params()
    import scan_match_cases as cases
    rng = np.random.default_rng(2)
    frames = cases.arc_frames(6, 1000, rng)
    pts = cases.cast(cases.TRUTH, 1000, rng)
    g = (cases.TRUTH[0] + 0.12, cases.TRUTH[1] - 0.09, cases.TRUTH[2] + 0.2)
    return frames, g, pts, scm.default_params(linear_search_window=0.3, angular_search_window=0.54)


def child(name, repeats, host_repeats):
    from visfs_amd import abi, backend
    from visfs_amd import submap as sm
    frames, guess, pts, prm = scene(name)
    s = backend.Solver(abi.default_params())
    dev = sm.Submaps(sm.default_params(num_range_data_limit=10 ** 6), solver=s)
    host = sm.Submaps(sm.default_params(num_range_data_limit=10 ** 6))
    for T, rd in frames:
        assert dev.insert(T, rd) == abi.OK and host.insert(T, rd) == abi.OK
    d = dev.describe()[0]

    def timed(sub, reps):
        ts, r = [], None
        for i in range(reps + 2):
            t0 = time.perf_counter()
            rc, r = sub.match(guess, pts, prm)
            t1 = time.perf_counter()
            assert rc == abi.OK, sub.last_error()
            if i >= 2:
                ts.append(t1 - t0)
        return ts, r

    t_dev, r_dev = timed(dev, repeats)
    t_host, r_host = timed(host, host_repeats)
    a_dev, a_host = dev.match_download(), host.match_download()
    agree = r_dev == r_host and all(x.tobytes() == y.tobytes() for x, y in zip(a_dev, a_host))
    if not agree:
        print(json.dumps(dict(tool="scan_match_timing", workload=name, error="device and host twin disagree", device=r_dev, host=r_host)))
        return 2
    S, nl = r_dev["num_scans"], r_dev["num_linear"]
    med = lambda v: float(np.median(v)) * 1e3      # noqa: E731
    print(json.dumps(dict(tool="scan_match_timing", workload=name, grid_cells=[d["num_x_cells"], d["num_y_cells"]], points=len(pts),
                          num_scans=S, offsets=(2 * nl + 1) ** 2, lookups=S * (2 * nl + 1) ** 2 * len(pts),
                          winner=[r_dev["scan_index"], r_dev["x_offset"], r_dev["y_offset"]], sum=r_dev["sum"], score=r_dev["score"],
                          identical=True, repeats=repeats, match_gpu_ms_median=med(t_dev), match_gpu_ms_min=float(np.min(t_dev)) * 1e3,
                          match_gpu_ms_max=float(np.max(t_dev)) * 1e3, host_repeats=host_repeats, match_host_1core_ms_median=med(t_host))))
    dev.close(); host.close(); s.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.child, a.repeats, a.host_repeats))
    lines = []
    for name in ("hall", "room"):
        res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats),
                              "--host-repeats", str(a.host_repeats)], capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit(f"workload {name} ended with status {res.returncode}: nothing reported")      # and nothing more is started
        lines.append(res.stdout.strip().splitlines()[-1])
    for line in lines:
        print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
