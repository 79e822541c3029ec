"""The verified place query against the staged calls, on the GPU: visfs_place_query_verify (one upload, seven launches, one download,
one wait) alternated in one process, on the same library and the same store, with visfs_place_query followed by one device
visfs_pnp_solve per candidate (each: one upload, two launches, one download, one wait), for 1, 4 and 8 candidates of 100 and 500
rows.  The two paths are alternated call by call, and their stage-1 results are required equal in every byte before anything is
timed.  The one call is timed with the guided stage (which the staged path does not have) and without it (like for like).  Host wall
clocks around the C calls made through ctypes, and around those only: the staged path's gather of a candidate's rows into the
from_xyz / to_xy arrays visfs_pnp_solve takes is done in NumPy here and is left outside its timed region (a C caller pays a copy of
a few KiB there, which this figure does not hold).  Median (min .. max) of --calls calls after --warmup warm-ups.  Prints a table and
one JSON line (and --out FILE).  It needs a device: without one it fails.

With --parent LIB (the library built from the parent commit) the plain visfs_place_query (500 key-points against 8 slots of 500
entries) is then timed on this library and on the parent's: fresh child processes in turn, one library each (VISFS_BA_LIB), --rounds
rounds; the parent's spread over its rounds is the yardstick, and the tool ends with a non-zero status when this library's median
of medians lies above it.  The result blocks of the two libraries are required equal.

    python tools/place_verify_timing.py [--calls 300] [--warmup 20] [--parent LIB] [--rounds 5] [--out profiles/place_verify_timing.log]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend  # noqa: E402
from visfs_amd import flow, place, pnp  # noqa: E402
from visfs_amd import place_verify as pv  # noqa: E402
import place_cases as pc  # noqa: E402
import place_verify_cases as vc  # noqa: E402


def stats(t):
    return dict(median_ms=float(np.median(t)) * 1e3, min_ms=float(np.min(t)) * 1e3, max_ms=float(np.max(t)) * 1e3, window_s=float(np.sum(t)))


def make_case(rows, candidates):
    """`candidates` slots of the same `rows` words of a pnp_cases scene (10 % outliers): every slot is a candidate of `rows` rows."""
    s, slot, qset, qxyz, perm, rng = vc.base(rows, 300 + rows, outliers=0.1)
    slots = []
    for k in range(candidates):
        c = dict(slot)
        c["key"] = k
        slots.append(c)
    return dict(qset=qset, slots=slots, query_xyz=qxyz)


def staged(lib_place, lib_pnp, db, dset, solver, pp, prm, cam, r, bufs):
    """visfs_place_query, then visfs_pnp_solve per candidate; returns (seconds inside the C calls, per-candidate (T, inliers) bytes)."""
    t0 = time.perf_counter()
    rc = lib_place.visfs_place_query(db.h, dset.h, C.byref(pp), C.byref(r))
    spent = time.perf_counter() - t0
    assert rc == abi.OK, db.last_error()
    out = []
    T, cov, matches, inliers, nm, ni, from_xyz, to_xy = bufs
    pf, pd, pi = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for c in range(r.n_candidates):
        n = r.candidate[c].count
        rows = np.frombuffer(memoryview(r.row[c]), dtype=place.ROW_DTYPE)[:n]
        from_xyz[:n] = rows["from_xyz"]
        to_xy[:n] = rows["to_xy"]
        args = (solver.h, C.byref(prm), C.byref(cam), n, from_xyz.ctypes.data_as(pf), to_xy.ctypes.data_as(pf), None, T.ctypes.data_as(pd),
                cov.ctypes.data_as(pd), matches.ctypes.data_as(pi), C.byref(nm), inliers.ctypes.data_as(pi), C.byref(ni))
        t0 = time.perf_counter()
        rc = lib_pnp.visfs_pnp_solve(*args)
        spent += time.perf_counter() - t0
        assert rc == abi.OK, solver.last_error()
        out.append((T.tobytes(), inliers[:ni.value].tobytes()))
    return spent, out


def child(calls, warmup):
    """The plain query on whatever library VISFS_BA_LIB names: one JSON line with the median in ms and a digest of the result block."""
    s = backend.Solver(abi.default_params(iterations=10, solver=2))
    lib = place.load()
    f = flow.Flow(flow.default_params(**pc.FLOW), 160, 120, solver=s)
    case = make_case(500, 8)
    dset = place.DescriptorSet(f, 512)
    db = place.KeyFrameStore(s, 8)
    for sl in case["slots"]:
        dset.upload(np.zeros((len(sl["desc"]), 2), np.float32), sl["desc"], sl["valid"])
        db.add(dset, sl["ids"], sl["xyz"], sl["key"])
    q = case["qset"]
    dset.upload(q["xy"], q["desc"], q["valid"])
    pp, r, t = place.default_params(min_matches=1), place.Result(), []
    for i in range(calls + warmup):
        t0 = time.perf_counter()
        rc = lib.visfs_place_query(db.h, dset.h, C.byref(pp), C.byref(r))
        t1 = time.perf_counter()
        assert rc == abi.OK, db.last_error()
        if i >= warmup:
            t.append(t1 - t0)
    print(json.dumps(dict(median_ms=float(np.median(t)) * 1e3, digest=hashlib.sha256(bytes(memoryview(r))).hexdigest(), counts=db.last_counts())))
    db.close(); dset.close(); f.close(); s.close()
    return 0


def against_parent(parent, rounds, calls, warmup, lines):
    """The plain query, this library and the parent's in turn, a fresh process each.  Returns (record, within the parent's spread)."""
    got = {"parent": [], "this": []}
    digests = set()
    for _ in range(rounds):
        for name in ("parent", "this"):
            env = dict(os.environ)
            env.pop("VISFS_BA_LIB", None)
            if name == "parent":
                env["VISFS_BA_LIB"] = os.path.abspath(parent)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(calls), "--warmup", str(warmup)], env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name}: the child failed\n{r.stdout}{r.stderr}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            got[name].append(rec["median_ms"])
            digests.add(rec["digest"])
    assert len(digests) == 1, "the two libraries' result blocks differ"
    p, t = got["parent"], got["this"]
    ok = float(np.median(t)) <= max(p)
    lines.append(f"plain visfs_place_query, 500 key-points x 8 slots of 500, {rounds} rounds of fresh processes in turn: the parent's medians "
                 f"{min(p):.4f} .. {max(p):.4f} ms (median {float(np.median(p)):.4f}), this library's {min(t):.4f} .. {max(t):.4f} ms "
                 f"(median {float(np.median(t)):.4f}): {'not above' if ok else 'ABOVE'} the parent's own spread; result blocks equal")
    print(lines[-1], flush=True)
    return dict(parent_ms=p, this_ms=t, within_parent_spread=ok), ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="the parent commit's libvisfs_ba_hip.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.calls, args.warmup)
    s = backend.Solver(abi.default_params(iterations=10, solver=2))         # raises without a device
    lib_place, lib_pnp, lib_v = place.load(), pnp.load(), pv.load()
    f = flow.Flow(flow.default_params(**pc.FLOW), 160, 120, solver=s)
    cam = pnp.camera(*vc.K, Tir=vc.TIR)
    results, lines = [], []
    for rows in (100, 500):
        for candidates in (1, 4, 8):
            case = make_case(rows, candidates)
            dset, db = vc.load(case, f, s)
            v, solver = pv.Verifier(db), pnp.Pnp(512, solver=s)
            pp = place.default_params(min_matches=1)
            vp_guided, vp_plain = pv.default_params(camera=cam), pv.default_params(camera=cam, guided=0)
            r, r2, w = place.Result(), place.Result(), pv.Result()
            bufs = (np.zeros(16), np.zeros(36), np.zeros(512, np.int32), np.zeros(512, np.int32), C.c_int32(), C.c_int32(),
                    np.zeros((512, 3), np.float32), np.zeros((512, 2), np.float32))
            t = dict(one_call_guided=[], one_call=[], staged=[])
            for i in range(args.calls + args.warmup):
                for name, vp in (("one_call_guided", vp_guided), ("one_call", vp_plain)):
                    t0 = time.perf_counter()
                    rc = lib_v.visfs_place_query_verify(v.h, dset.h, C.byref(pp), C.byref(vp), None, C.byref(r2), C.byref(w))
                    t1 = time.perf_counter()
                    assert rc == abi.OK, v.last_error()
                    if i >= args.warmup:
                        t[name].append(t1 - t0)
                spent, got = staged(lib_place, lib_pnp, db, dset, solver, pp, vp_plain.pnp, cam, r, bufs)
                if i >= args.warmup:
                    t["staged"].append(spent)
                if i == 0:                                                      # the results are required equal
                    assert bytes(memoryview(r)) == bytes(memoryview(r2)) and r.n_candidates == candidates
                    for c in range(candidates):
                        assert r.candidate[c].count == rows
                        a = w.candidate[c].stage1
                        assert np.array(a.T[:]).tobytes() == got[c][0] and np.array(a.inliers[:a.n_inliers], dtype=np.int32).tobytes() == got[c][1]
            rec = dict(rows=rows, candidates=candidates, counts_one_call=v.last_counts(), **{k: stats(x) for k, x in t.items()})
            results.append(rec)
            lines.append(f"{rows:4d} rows x {candidates} candidates: " + ", ".join(
                f"{k} {rec[k]['median_ms']:.3f} ({rec[k]['min_ms']:.3f} .. {rec[k]['max_ms']:.3f}) ms" for k in ("one_call_guided", "one_call", "staged")))
            print(lines[-1], flush=True)
            for o in (v, solver, db, dset):
                o.close()
    f.close(); s.close()
    parent, ok = None, True
    if args.parent:
        parent, ok = against_parent(args.parent, args.rounds, args.calls, args.warmup, lines)
    line = json.dumps(dict(tool="place_verify_timing", calls=args.calls, warmup=args.warmup, results=results, plain_query_against_parent=parent))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + line + "\n")
    if not ok:
        sys.exit("the plain query: this library's median lies above the parent's own spread (the log is written)")


if __name__ == "__main__":
    sys.exit(main())
