#!/usr/bin/env python3
"""Times the global occupancy map (include/visfs_map.h): one visfs_map_compose of 64 tiles of 400 x 400 cells at 0.05 m placed
around a loop of 35 m radius, ODDS, on the device against the same call on the one-core host twin, the two alternating in one
process; then visfs_scan_stack_create_from_map at depth 7 against downloading the cells and calling
visfs_scan_stack_create_from_grid.  A figure is reported only if the device and the twin returned the same bytes (info, cells,
counts; the stacks' levels); otherwise the tool stops.  Medians of 5.  Writes profiles/global_map_timing.log.

usage: tools/global_map_timing.py [--repeats R] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                 # noqa: E402

import global_map_cases as gc                      # noqa: E402
from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import global_map as gm             # noqa: E402
from visfs_amd import scan_fast as sf              # noqa: E402

TILES, SIDE, RADIUS, DEPTH = 64, 400, 35.0, 7


def tiles():
    rng = np.random.default_rng(64)
    out = []
    for k in range(TILES):
        a = 2 * math.pi * k / TILES
        out.append(gc.tile(rng, SIDE, SIDE, pose=(RADIUS * math.cos(a), RADIUS * math.sin(a), a + 0.5 * math.pi), palette=True))
    return out


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_map_timing.log"))
    args = ap.parse_args()
    solver = backend.Solver(abi.default_params())
    dev, host = gm.GlobalMap(solver), gm.GlobalMap()
    for t in tiles():
        for m in (dev, host):
            rc, _ = m.add_grid(t["cells"], t["limits"], t["pose"])
            if rc != abi.OK:
                sys.exit(f"add_grid: status {rc}: {m.last_error()}")
    lines = ["# tools/global_map_timing.py: median wall times, device and twin alternating; 64 tiles of 400 x 400 cells at 0.05 m, ODDS"]
    times = {"device": [], "twin": []}
    last = {}
    for rep in range(args.repeats + 1):                                     # the first round warms both up (and makes the buffers)
        for name, m in (("device", dev), ("twin", host)):
            dt, (rc, info) = timed(lambda: m.compose(gm.ODDS))
            if rc != abi.OK:
                sys.exit(f"{name}: status {rc}: {m.last_error()}")
            if rep:
                times[name].append(dt)
            rc, cells, count = m.download()
            assert rc == abi.OK
            last[name] = (info, cells, count)
        if last["device"][0] != last["twin"][0] or any(last["device"][i].tobytes() != last["twin"][i].tobytes() for i in (1, 2)):
            sys.exit("the device and the twin differ; nothing is reported")
    info, cells, count = last["device"]
    d, t = statistics.median(times["device"]) * 1e3, statistics.median(times["twin"]) * 1e3
    lines += ["# compose: num_x_cells num_y_cells cells known_cells cells_of_two_or_more_tiles tiles_drawn launches copies waits device_ms twin_ms twin_over_device",
              f"{info['num_x_cells']} {info['num_y_cells']} {cells.size} {int((count > 0).sum())} {int((count > 1).sum())} {info['tiles_drawn']} "
              + " ".join(str(v) for v in dev.last_counts()) + f" {d:.3f} {t:.3f} {t / d:.2f}"]
    print(lines[-1], flush=True)

    # the composed grid frozen into a stack: where it lives, against a download and visfs_scan_stack_create_from_grid
    direct, round_trip = [], []
    for rep in range(args.repeats + 1):
        dt, a = timed(lambda: dev.freeze(DEPTH))

        def via_host():
            rc, c, _ = dev.download()
            assert rc == abi.OK
            return sf.ScanStack.from_grid(c, info, DEPTH, solver=solver)
        dt2, b = timed(via_host)
        if a.status != abi.OK or b.status != abi.OK:
            sys.exit(f"stack: status {a.status} / {b.status}: {dev.last_error()}")
        if rep == 0:
            for h in range(DEPTH):
                if a.download_level(h)[0].tobytes() != b.download_level(h)[0].tobytes():
                    sys.exit(f"level {h} of the two stacks differs; nothing is reported")
        else:
            direct.append(dt); round_trip.append(dt2)
        a.close(); b.close()
    d, t = statistics.median(direct) * 1e3, statistics.median(round_trip) * 1e3
    lines += ["# stack of depth 7 from the composed grid: create_from_map_ms download_and_create_from_grid_ms ratio", f"{d:.3f} {t:.3f} {t / d:.2f}"]
    print(lines[-1], flush=True)
    dev.close(); host.close(); solver.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
