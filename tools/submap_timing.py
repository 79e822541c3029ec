"""Laser sub-maps: one frame's insertion on the GPU against the host restatement on one core, and a laser window's solve
against the resident matching grid against the host-grid path.

The scan: ~1 000 returns over 360 degrees in a 70 m x 50 m hall (ranges capped at 30 m), 5 misses, 0.05 m cells; the
sub-maps are first grown past 1600 x 1600 cells.  Writes one JSON line (and --out FILE).

    python tools/submap_timing.py [--frames 40] [--out profiles/submap_timing.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend, synth  # noqa: E402
from visfs_amd import submap as sm  # noqa: E402
from test_gpu_submap import pose, room_scan  # noqa: E402


_hip = None


def sync():
    """hipDeviceSynchronize of the HIP runtime the library already loaded (the insertions run on the handle's stream)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--solves", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    room = (-35.0, 35.0, -25.0, 25.0)
    rng = np.random.default_rng(1)
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    dev = sm.Submaps(sm.default_params(num_range_data_limit=10 ** 6), solver=s)      # no life-cycle event inside the timed frames
    host = sm.Submaps(sm.default_params(num_range_data_limit=10 ** 6))
    # grow: scans from the corners of the hall
    for x, y in ((-30, -20), (30, 20), (-30, 20), (30, -20), (0, 0)):
        T = pose(x, y, 0.0)
        rd = [room_scan(T, room, 1000, rng, n_miss=5)]
        dev.insert(T, rd); host.insert(T, rd)
    sync()
    d = dev.describe()[0]
    assert d["num_x_cells"] >= 1600 and d["num_y_cells"] >= 1600, d
    frames = []
    for f in range(a.frames):
        T = pose(10 * math.cos(0.1 * f), 8 * math.sin(0.1 * f), 0.1 * f)
        frames.append((T, [room_scan(T, room, 1000, rng, n_miss=5)]))
    t_dev, t_host = [], []
    for T, rd in frames:
        sync()
        t0 = time.perf_counter(); dev.insert(T, rd); sync(); t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); host.insert(T, rd); t_host.append(time.perf_counter() - t0)
    ident = all(np.array_equal(dev.download(i)[0], host.download(i)[0]) for i in range(len(dev.describe())))
    # a laser window (500 points) against the resident grid vs the host grid path
    w = synth.make_laser_window(n_points=500)
    d = dev.describe()[0]
    _, cost = dev.download(0)
    w2 = dict(w); w2["grid"] = dict(resolution=d["resolution"], max_x=d["max_x"], max_y=d["max_y"], cost=cost)
    wb, wb2 = abi.WindowBuffers(w), abi.WindowBuffers(w2)
    t_res, t_hostgrid = [], []
    for i in range(a.solves + 3):
        t0 = time.perf_counter(); dev.solve_window(wb, s); t1 = time.perf_counter()
        s.solve_window(wb2); t2 = time.perf_counter()
        if i >= 3:
            t_res.append(t1 - t0); t_hostgrid.append(t2 - t1)
    med = lambda v: float(np.median(v)) * 1e3      # noqa: E731
    out = dict(tool="submap_timing", grid_cells=[d["num_x_cells"], d["num_y_cells"]], returns_per_frame=1000, misses_per_frame=5,
               frames=a.frames, insert_gpu_ms_median=med(t_dev), insert_gpu_ms_min=float(np.min(t_dev)) * 1e3,
               insert_host_1core_ms_median=med(t_host), grids_identical=bool(ident),
               solve_resident_grid_ms_median=med(t_res), solve_host_grid_ms_median=med(t_hostgrid), solves=a.solves,
               grid_mb=d["num_x_cells"] * d["num_y_cells"] * 4 / 2 ** 20)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    dev.close(); host.close(); s.close()


if __name__ == "__main__":
    main()
