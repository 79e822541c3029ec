#!/usr/bin/env python3
"""Times the laser pretreatment with its voxel filters (include/visfs_scan_filter.h): one visfs_scan_filter_process of 1, 4, 16 and
64 scans of 1 440 and of 16 384 points (a room seen from inside, 5 % beyond max_range, two subdivisions, the default filters) on the
device against the same call on the one-core host twin, the two alternating in one process.  Only the C call is timed: the scan
table is built before.  A figure is reported only if the device and the twin returned the same records, range data, match clouds
and hook data; otherwise the tool stops.  Medians of 7.  Writes profiles/scan_filter_timing.log.

usage: tools/scan_filter_timing.py [--repeats R] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                 # noqa: E402

import scan_filter_cases as fc                     # noqa: E402
from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import scan_filter as sf            # noqa: E402

SCANS, POINTS = (1, 4, 16, 64), (1440, 16384)


def table(scans):
    arr = (sf.Scan * len(scans))()
    for i, pts in enumerate(scans):
        arr[i].T_laser_to_camera[:] = list(sf.IDENTITY)
        arr[i].n = len(pts)
        arr[i].points_xyz = pts.ctypes.data_as(C.POINTER(C.c_double))
    return arr


def snapshot(f, scans):
    out = []
    for i, pts in enumerate(scans):
        d = f.download(i, len(pts))
        rd = f.range_data(i)
        out.append((f.record(i), [(o, r.tobytes(), m.tobytes()) for o, r, m in rd], f.match_cloud(i).tobytes(),
                    d["cls"].tobytes(), d["sub"].tobytes(), d["kept"].tobytes(), d["trace"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_filter_timing.log"))
    args = ap.parse_args()
    lib = sf.load()
    solver = backend.Solver(abi.default_params())
    dev, host = sf.ScanFilter(solver), sf.ScanFilter()
    prm = sf.default_params(num_subdivisions=2)
    lines = ["# tools/scan_filter_timing.py: median wall times of visfs_scan_filter_process, device and twin alternating",
             "# points_per_scan scans returns_kept_per_scan match_points_per_scan passes_per_scan launches copies waits device_ms twin_ms twin_over_device device_ms_per_scan"]
    for n in POINTS:
        rng = np.random.default_rng(n)
        clouds = [np.ascontiguousarray(fc.room_scan(rng, n, far=0.05, near=0.01)) for _ in range(max(SCANS))]
        for m in SCANS:
            scans = clouds[:m]
            arr = table(scans)
            times = {"device": [], "twin": []}
            snap = {}
            for rep in range(args.repeats + 1):                             # the first round warms both up (and makes the buffers)
                for name, f in (("device", dev), ("twin", host)):
                    t0 = time.perf_counter()
                    rc = lib.visfs_scan_filter_process(f.h, C.byref(prm), m, arr, None)
                    dt = time.perf_counter() - t0
                    if rc != abi.OK:
                        sys.exit(f"{name}: status {rc}: {f.last_error()}")
                    if rep:
                        times[name].append(dt)
                    if rep <= 1:
                        snap[name] = snapshot(f, scans)
                if rep <= 1 and snap["device"] != snap["twin"]:
                    sys.exit("the device and the twin differ; nothing is reported")
            recs = [r[0][1] for r in snap["device"]]
            d, t = statistics.median(times["device"]) * 1e3, statistics.median(times["twin"]) * 1e3
            lines.append(f"{n} {m} {sum(r['n_returns'] for r in recs) / m:.0f} {sum(r['n_match'] for r in recs) / m:.0f} "
                         f"{sum(r['passes'] for r in recs) / m:.1f} " + " ".join(str(v) for v in dev.last_counts())
                         + f" {d:.3f} {t:.3f} {t / d:.2f} {d / m:.3f}")
            print(lines[-1], flush=True)
    dev.close(); host.close(); solver.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
