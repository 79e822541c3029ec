#!/usr/bin/env python3
"""Times the Monte-Carlo localisation (include/visfs_mcl.h), the C calls only, the device and the one-core host twin alternating in
one process: visfs_mcl_field_create_from_map on a composed map of 1844 x 1844 cells at 0.05 m (R = 40), then visfs_mcl_update for
N = 100, 3000, 65536 particles with 30 and 200 beams on the field of a 400 x 400 room map: a thread per particle (lanes = 1), a
wavefront per particle (lanes = 64) and the library's choice.  A figure is reported only if the device and the twin returned the
same bytes in every array and every field of the result, every time; otherwise the tool stops.  Medians of 7.  Writes
profiles/mcl_timing.log.

usage: tools/mcl_timing.py [--repeats R] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                 # noqa: E402

from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import global_map as gm             # noqa: E402
from visfs_amd import mcl                          # noqa: E402

SIDE, TILE = 1844, 461
ROOM = 400
OCC, FREE = 2000, 30000


def limits(nx, ny, max_x, max_y):
    return dict(resolution=0.05, max_x=max_x, max_y=max_y, num_x_cells=nx, num_y_cells=ny)


def big_map(solver):
    """16 tiles of 461 x 461 cells side by side: rooms of walls, so that obstacles are as dense as in a building's map."""
    m = gm.GlobalMap(solver)
    tile = np.full((TILE, TILE), FREE, dtype=np.uint16)
    tile[::92, :] = OCC
    tile[:, ::92] = OCC
    tile[40:52, :] = FREE                                                   # doorways
    for r in range(4):
        for c in range(4):
            rc, _ = m.add_grid(tile, limits(TILE, TILE, (r + 1) * TILE * 0.05, (c + 1) * TILE * 0.05))
            assert rc == abi.OK, m.last_error()
    rc, info = m.compose(gm.ODDS, limits=limits(SIDE, SIDE, SIDE * 0.05, SIDE * 0.05))
    assert rc == abi.OK and (info["num_x_cells"], info["num_y_cells"]) == (SIDE, SIDE), m.last_error()
    return m


def room():
    c = np.zeros((ROOM, ROOM), dtype=np.uint16)
    c[40:360, 40:360] = OCC
    c[42:358, 42:358] = FREE
    c[150:170, 200:230] = OCC
    return c, limits(ROOM, ROOM, ROOM * 0.05, ROOM * 0.05)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcl_timing.log"))
    args = ap.parse_args()
    solver = backend.Solver(abi.default_params())
    lib = mcl.load()
    lines = ["# tools/mcl_timing.py: median wall times of the C calls, device and twin alternating, equal in every byte"]

    # ---- the field of a 1844 x 1844 composed map
    maps = {"device": big_map(solver), "twin": big_map(None)}
    times = {"device": [], "twin": []}
    last = {}
    for rep in range(args.repeats + 1):                                     # the first round warms both up
        for name, m in maps.items():
            dt, f = timed(lambda: mcl.Field.from_map(m))
            if f.status != abi.OK:
                sys.exit(f"{name}: field status {f.status}")
            if rep:
                times[name].append(dt)
            if rep in (0, args.repeats):
                last[name] = f.download() + (f.describe(), f.last_counts())
            f.close()
        if rep in (0, args.repeats):
            a, b = last["device"], last["twin"]
            if a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes() or a[2:4] != b[2:4]:
                sys.exit("the device's field and the twin's differ; nothing is reported")
    d, t = statistics.median(times["device"]) * 1e3, statistics.median(times["twin"]) * 1e3
    desc, counts = last["device"][4], last["device"][5]
    lines += ["# field: num_x_cells num_y_cells R T obstacle_cells launches copies waits device_ms twin_ms twin_over_device",
              f"{desc['num_x_cells']} {desc['num_y_cells']} {desc['R']} {desc['T']} {int((last['device'][0] == 0).sum())} "
              + " ".join(str(v) for v in counts) + f" {d:.3f} {t:.3f} {t / d:.2f}"]
    print(lines[-1], flush=True)
    for m in maps.values():
        m.close()

    # ---- the filter
    cells, lim = room()
    fields = {"device": mcl.Field.from_grid(cells, lim, solver=solver), "twin": mcl.Field.from_grid(cells, lim)}
    assert all(f.status == abi.OK for f in fields.values())
    rng = np.random.default_rng(5)
    lines.append("# update: particles beams lanes(0 = the library's choice) launches copies waits device_ms twin_ms twin_over_device")
    prm = mcl.default_params()
    for N in (100, 3000, 65536):
        for n in (30, 200):
            r, a = 6.0 * np.sqrt(rng.random(n)), 2.0 * np.pi * rng.random(n)
            pts = np.ascontiguousarray(np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1))
            delta = np.array([0.05, 0.0, 0.01])
            for lanes in (1, 64, 0):
                flt = {k: mcl.Filter(f, N, 11) for k, f in fields.items()}
                times = {"device": [], "twin": []}
                for k, f in flt.items():
                    assert f.status == abi.OK and f.init((10.0, 10.0, 0.3), (0.5, 0.5, 0.2)) == abi.OK
                assert flt["device"].set_lanes(lanes) == abi.OK
                for rep in range(args.repeats + 1):
                    res = {}
                    for k, f in flt.items():
                        out = abi.MclResult()
                        t0 = time.perf_counter()
                        rc = lib.visfs_mcl_update(f.h, C.byref(prm), delta.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                  pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
                        dt = time.perf_counter() - t0
                        if rc != abi.OK:
                            sys.exit(f"{k}: update status {rc}: {f.last_error()}")
                        if rep:
                            times[k].append(dt)
                        res[k] = (bytes(out), f.download())
                    if res["device"][0] != res["twin"][0] or any(res["device"][1][key].tobytes() != res["twin"][1][key].tobytes() for key in res["twin"][1]):
                        sys.exit(f"N = {N}, n = {n}, lanes = {lanes}: the device and the twin differ; nothing is reported")
                d, t = statistics.median(times["device"]) * 1e3, statistics.median(times["twin"]) * 1e3
                lines.append(f"{N} {n} {lanes} " + " ".join(str(v) for v in flt["device"].last_counts()) + f" {d:.3f} {t:.3f} {t / d:.2f}")
                print(lines[-1], flush=True)
                for f in flt.values():
                    f.close()
    for f in fields.values():
        f.close()
    solver.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
