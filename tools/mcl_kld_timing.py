#!/usr/bin/env python3
"""Times the KLD-adaptive particle counts (include/visfs_mcl_kld.h), the C call visfs_mcl_update only, at a capacity of N = 3000 with
30 and 200 beams on the field of a 400 x 400 room map:

  plain     a plain filter of 3000;
  kld_full  a KLD filter whose belief is wide (initialised again before every second update: every resampling runs all 3000 draws
            and keeps them, the count stays at N);
  kld_settled  a KLD filter of a robot that stands still with a narrow belief, read after 40 updates, at the count it has settled at.

The device and the one-core host twin run in step and a figure is reported only if they returned the same bytes in both results of
every update and in every array at the end; otherwise the tool stops.  Medians over the timed updates, and over those that
resampled and those that did not.

With --parent LIB (the library built from the parent commit) the plain update is then timed against it: fresh child processes in
turn, one library each (VISFS_BA_LIB), ROUNDS rounds; the parent's spread is the least and the largest of its medians.  Writes
profiles/mcl_kld_timing.log.

usage: tools/mcl_kld_timing.py [--updates U] [--rounds R] [--parent LIB] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                 # noqa: E402

from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import mcl                          # noqa: E402
from visfs_amd import mcl_kld as kld               # noqa: E402

ROOM, RES = 400, 0.05
OCC, FREE = 2000, 30000
N = 3000
TRUTH = (10.0, 10.0, 0.3)
BEAMS = (30, 200)


def room():
    c = np.zeros((ROOM, ROOM), dtype=np.uint16)
    c[40:360, 40:360] = OCC
    c[42:358, 42:358] = FREE
    c[150:170, 200:230] = OCC
    return c, dict(resolution=RES, max_x=ROOM * RES, max_y=ROOM * RES, num_x_cells=ROOM, num_y_cells=ROOM)


def scan(cells, lim, n):
    """n points on the room's inner wall faces as the robot at TRUTH sees them: the centres of obstacle cells, in its frame."""
    iy, ix = np.nonzero(cells[41:359, 41:359] == OCC)
    iy, ix = iy + 41, ix + 41
    pick = np.linspace(0, len(ix) - 1, n).astype(np.int64)
    X = lim["max_x"] - (iy[pick] + 0.5) * RES
    Y = lim["max_y"] - (ix[pick] + 0.5) * RES
    c, s = np.cos(TRUTH[2]), np.sin(TRUTH[2])
    dx, dy = X - TRUTH[0], Y - TRUTH[1]
    return np.ascontiguousarray(np.stack([c * dx + s * dy, -s * dx + c * dy, np.zeros(n)], axis=1))


def update(lib, f, prm, delta, pts):
    out = abi.MclResult()
    t0 = time.perf_counter()
    rc = lib.visfs_mcl_update(f.h, C.byref(prm), delta.ctypes.data_as(C.POINTER(C.c_double)), len(pts), pts.ctypes.data_as(C.POINTER(C.c_double)),
                              C.byref(out))
    dt = time.perf_counter() - t0
    if rc != abi.OK:
        sys.exit(f"update status {rc}: {f.last_error()}")
    return dt, out


def med(v):
    return statistics.median(v) * 1e3 if v else float("nan")


def scenario(lib, fields, name, pts, sigma, warm, updates, reinit=False):
    """The device and the twin in step; one line of the log for each.  reinit: visfs_mcl_init before every second update, so that
    every resampling meets the wide belief again."""
    prm = mcl.default_params()
    flt = {k: mcl.Filter(f, N, 11) for k, f in fields.items()}
    for f in flt.values():
        assert f.status == abi.OK
        if name != "plain":
            assert kld.enable(f) == abi.OK, f.last_error()
        assert f.init(TRUTH, sigma) == abi.OK
    times = {k: ([], []) for k in flt}                                     # not resampled, resampled
    counts = []
    for u in range(warm + updates):
        delta = np.array([0.02, 0.0, 0.01]) * (1.0 if u % 2 == 0 else -1.0)   # the robot stands still: the odometry only jitters
        res = {}
        for k, f in flt.items():
            if reinit and u % 2 == 0:
                assert f.init(TRUTH, sigma) == abi.OK
            dt, out = update(lib, f, prm, delta, pts)
            res[k] = bytes(out) + (json.dumps(kld.last(f)).encode() if name != "plain" else b"")
            if u >= warm:
                times[k][out.resampled].append(dt)
        if res["device"] != res["twin"]:
            sys.exit(f"{name}, update {u}: the device and the twin differ; nothing is reported")
        if u >= warm:
            counts.append(kld.count(flt["device"]))
    a, b = kld.download(flt["device"]), kld.download(flt["twin"])
    if any(a[key].tobytes() != b[key].tobytes() for key in a):
        sys.exit(f"{name}: the device's particles and the twin's differ; nothing is reported")
    lines = []
    for k in ("device", "twin"):
        skip, ran = times[k]
        lines.append(f"{name} {len(pts)} {k} {min(counts)} {max(counts)} " + " ".join(str(v) for v in flt[k].last_counts())
                     + f" {med(skip + ran):.4f} {med(ran):.4f} {med(skip):.4f}")
        print(lines[-1], flush=True)
    for f in flt.values():
        f.close()
    return lines


def child(updates):
    """The plain update of whatever library VISFS_BA_LIB names: one JSON line of medians in ms, by beams."""
    solver = backend.Solver(abi.default_params())
    lib = mcl.load()
    cells, lim = room()
    field = mcl.Field.from_grid(cells, lim, solver=solver)
    assert field.status == abi.OK
    prm = mcl.default_params()
    out = {}
    for n in BEAMS:
        pts = scan(cells, lim, n)
        f = mcl.Filter(field, N, 11)
        assert f.status == abi.OK and f.init(TRUTH, (0.3, 0.3, 0.2)) == abi.OK
        t = []
        for u in range(20 + updates):
            delta = np.array([0.02, 0.0, 0.01]) * (1.0 if u % 2 == 0 else -1.0)
            dt, _ = update(lib, f, prm, delta, pts)
            if u >= 20:
                t.append(dt)
        out[str(n)] = med(t)
        f.close()
    field.close()
    solver.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="the parent commit's libvisfs_ba_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcl_kld_timing.log"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.updates)
    solver = backend.Solver(abi.default_params())
    lib = kld.load()
    cells, lim = room()
    fields = {"device": mcl.Field.from_grid(cells, lim, solver=solver), "twin": mcl.Field.from_grid(cells, lim)}
    assert all(f.status == abi.OK for f in fields.values())
    lines = ["# tools/mcl_kld_timing.py: median wall times of visfs_mcl_update in ms, capacity 3000, the device and the twin in step, equal in every byte",
             "# scenario beams flavour count_min count_max launches copies waits all_ms resampling_ms not_resampling_ms"]
    for n in BEAMS:
        pts = scan(cells, lim, n)
        lines += scenario(lib, fields, "plain", pts, (0.3, 0.3, 0.2), 4, args.updates)
        lines += scenario(lib, fields, "kld_full", pts, (3.0, 3.0, 1.0), 4, args.updates, reinit=True)
        lines += scenario(lib, fields, "kld_settled", pts, (0.3, 0.3, 0.2), 40, args.updates)
    for f in fields.values():
        f.close()
    solver.close()

    if args.parent:
        lines.append(f"# the plain update, this library and the parent's in turn, a fresh process each, {args.rounds} rounds: library beams medians_ms")
        got = {"parent": {str(n): [] for n in BEAMS}, "this": {str(n): [] for n in BEAMS}}
        for _ in range(args.rounds):
            for name in ("parent", "this"):
                env = dict(os.environ)
                env.pop("VISFS_BA_LIB", None)
                if name == "parent":
                    env["VISFS_BA_LIB"] = os.path.abspath(args.parent)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--updates", str(args.updates)], env=env, capture_output=True,
                                   text=True, timeout=300)
                if r.returncode != 0:
                    sys.exit(f"{name}: the child failed\n{r.stdout}{r.stderr}")
                for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                    got[name][k].append(v)
        for n in BEAMS:
            p, t = got["parent"][str(n)], got["this"][str(n)]
            for name, v in (("parent", p), ("this", t)):
                lines.append(f"{name} {n} " + " ".join(f"{x:.4f}" for x in v))
            inside = statistics.median(t) <= max(p)
            lines.append(f"# {n} beams: the parent's spread {min(p):.4f} .. {max(p):.4f} ms, this library's median {statistics.median(t):.4f} ms: "
                         + ("inside (not above it)" if inside else "ABOVE the spread"))
        for l in lines[-3 * len(BEAMS) - 1:]:
            print(l, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
