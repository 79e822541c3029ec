"""Scan stack groups: one group call over m frozen sub-maps against the same m single calls issued one behind the other on the same
library in the same process, alternating (each side timed up to the return of its last call, every call ending in its own stream
wait).

Workloads, each measured in a child process of its own under a time limit:
  room m   the `room` of tools/scan_match_timing.py, 1 000 returns, 1.6 m / 0.5 rad (nl = 32, as tools/scan_fast_timing.py's nl32),
           m = 1, 4, 16, 64 stacks of the same sub-map;
  hall 4   the `hall` relocalisation of tools/scan_fast_timing.py (7 m / 30 degrees: nl = 140, S ~ 630), m = 4.
Nothing is reported unless every member's record and hook data (B, per-level counts, bounds, sorted survivors) equal the single
call's.  Writes one JSON line per workload: the times of both sides, and the launches, copies and waits the group counted.

    python tools/scan_group_timing.py [--repeats 20] [--out profiles/scan_group_timing.log]

--single-ab compares the single call of this tree's library with that of the library VISFS_BA_PARENT_LIB names (the parent commit's
build, see tools/build_variant.sh) on `room` and `hall`, each with one member: --children children per library and workload, each
loading one library through VISFS_BA_LIB, interleaved (parent, here, parent, ...); the first child that fails ends the run.  The
`single_calls` medians of the children are compared; the yardstick is the parent's own spread (max - min of its children's medians
on that workload).  The single call's record and hook arrays go into a digest, which must be the same in every child of both
libraries.

    VISFS_BA_PARENT_LIB=visfs_amd/lib/libvisfs_ba_hip_parent.so python tools/scan_group_timing.py --single-ab [--children 5]
                                                                        [--out profiles/scan_single_timing.log]
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEPTH = 7
WORKLOADS = [("room", 1), ("room", 4), ("room", 16), ("room", 64), ("hall", 4)]
AB_WORKLOADS = [("room", 1), ("hall", 1)]


def stats(ts):
    v = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), repeats=len(ts))


def same_hook(a, b):
    return ((a["S"], a["L"], a["n"], a["H"], a["B"], a["scored"], a["kept"]) == (b["S"], b["L"], b["n"], b["H"], b["B"], b["scored"], b["kept"])
            and a["bounds"].tobytes() == b["bounds"].tobytes() and a["survivors"].tobytes() == b["survivors"].tobytes())


def single_digest(rs, stacks):
    """The single calls' records and hook arrays, as bytes."""
    h = hashlib.sha256()
    for r, st in zip(rs, stacks):
        hk = st.match_download()
        h.update(json.dumps({k: (np.float64(v).tobytes().hex() if isinstance(v, float) else v) for k, v in r.items()}, sort_keys=True).encode())
        h.update(json.dumps([hk[k] for k in ("S", "L", "n", "H", "B", "scored", "kept")]).encode())
        h.update(hk["bounds"].tobytes()); h.update(hk["survivors"].tobytes())
    return h.hexdigest()


def child(name, m, repeats):
    import scan_fast_timing as sft
    from visfs_amd import abi, backend
    from visfs_amd import scan_fast as sf
    from visfs_amd import scan_group as sg
    s = backend.Solver(abi.default_params())
    dev, host, guess, pts = sft.submaps_of(name, s)
    host.close()
    if name == "room":
        lw, aw, cap = 1.6, 0.5, 1 << 16                  # m * cap stays far inside 2^26 for m = 64
    else:
        guess = (guess[0] + 5.0, guess[1] - 4.0, guess[2] + 0.3)
        lw, aw, cap = 7.0, 30.0 * np.pi / 180.0, 1 << 20
    stacks = [dev.freeze(0, DEPTH) for _ in range(m)]
    assert all(st.status == abi.OK for st in stacks), dev.last_error()
    group = sg.ScanStackGroup(stacks)
    assert group.status == abi.OK, sg.create_error()
    prm = sf.default_params(linear_search_window=lw, angular_search_window=aw, frontier_capacity=cap)
    # the members' guesses differ by a few cells, as candidates' would
    guesses = [(guess[0] + 0.05 * (i % 4), guess[1] - 0.05 * (i // 4 % 4), guess[2] + 0.002 * i) for i in range(m)]

    def run_group():
        res, status, best = group.match(guesses, pts, params=prm)
        assert group.rc == abi.OK and all(v == abi.OK for v in status), group.last_error()
        return res, best

    def run_singles():
        out = []
        for st, g in zip(stacks, guesses):
            rc, r = st.match(g, pts, prm)
            assert rc == abi.OK, st.last_error()
            out.append(r)
        return out

    t_group, t_single = [], []
    for i in range(repeats + 2):
        t0 = time.perf_counter()
        rg, best = run_group()
        t1 = time.perf_counter()
        rs = run_singles()
        t2 = time.perf_counter()
        if i >= 2:
            t_group.append(t1 - t0); t_single.append(t2 - t1)
    out = dict(tool="scan_group_timing", workload=name, members=m, depth=DEPTH, points=len(pts), frontier_capacity=cap)
    for i, st in enumerate(stacks):
        if rg[i] != rs[i] or not same_hook(group.match_download(i), st.match_download()):
            print(json.dumps(dict(out, error=f"member {i}: the group call and the single call disagree", group=rg[i], single=rs[i])))
            return 2
    sums = [r["sum"] if r["matched"] else -1 for r in rs]
    if best != (int(np.argmax(sums)) if max(sums) >= 0 else -1):
        print(json.dumps(dict(out, error="best_member is not the arg-max of the single calls' sums", best=best, sums=sums)))
        return 2
    H = rg[0]["depth_used"] - 1
    hk = group.match_download(0)
    out.update(num_scans=rg[0]["num_scans"], num_linear=rg[0]["num_linear"], H=H, identical=True, best_member=best,
               scored_member0=hk["scored"], kept_member0=hk["kept"], group_counts=group.last_counts(),
               single_counts=dict(kernel_launches=m * (H + 5), copies_and_memsets=2 * m, synchronisations=m),
               group_call=stats(t_group), single_calls=stats(t_single), single_digest=single_digest(rs, stacks))
    print(json.dumps(out))
    group.close()
    for st in stacks:
        st.close()
    dev.close(); s.close()
    return 0


def run_child(name, m, repeats, lib=None):
    """One measuring child under its time limit; anything but success ends the run, and nothing more is started."""
    env = dict(os.environ)
    if lib:
        env["VISFS_BA_LIB"] = lib
    else:
        env.pop("VISFS_BA_LIB", None)
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--members", str(m),
                          "--repeats", str(repeats)], capture_output=True, text=True, env=env)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        sys.exit(f"workload {name} m = {m} ({lib or 'the library of this tree'}) ended with status {res.returncode}: nothing reported")
    return res.stdout.strip().splitlines()[-1]


def single_ab(children, repeats, out_path):
    parent = os.environ.get("VISFS_BA_PARENT_LIB")
    if not parent:
        sys.exit("--single-ab needs VISFS_BA_PARENT_LIB: the parent commit's library (tools/build_variant.sh)")
    parent = os.path.abspath(parent)
    libs = [("parent", parent), ("here", None)]
    lines = [f"scan_single_timing: visfs_scan_stack_match on a device stack of depth {DEPTH}, ms per call up to its return; per child the median of "
             f"{repeats} timed calls after 2 warm-ups; {children} children per library and workload, interleaved; parent: "
             f"{os.path.relpath(parent, ROOT)}, here: the library of this tree"]
    rows, ok = [], True
    for name, m in AB_WORKLOADS:
        runs = {k: [] for k, _ in libs}
        for _ in range(children):
            for k, lib in libs:
                runs[k].append(json.loads(run_child(name, m, repeats, lib)))
        digests = {r["single_digest"] for rs in runs.values() for r in rs}
        if len(digests) != 1:
            sys.exit(f"{name} m = {m}: the single call's record and hook arrays differ between the libraries: {sorted(digests)}")
        med = {k: [r["single_calls"]["median_ms"] / m for r in rs] for k, rs in runs.items()}
        a, b = float(np.median(med["parent"])), float(np.median(med["here"]))
        spread = max(med["parent"]) - min(med["parent"])
        inside = b - a <= spread
        ok = ok and inside
        r0 = runs["here"][0]
        lines.append(f"{name} m = {m}  n = {r0['points']}, S = {r0['num_scans']}, nl = {r0['num_linear']}, H = {r0['H']}; record and hook digest "
                     f"{digests.pop()[:16]} in all {2 * children} children")
        for k, _ in libs:
            lines.append(f"        {k:<7} medians {[round(v, 4) for v in med[k]]}  median {float(np.median(med[k])):.4f} ms  "
                         f"min {min(r['single_calls']['min_ms'] for r in runs[k]) / m:.4f}  max {max(r['single_calls']['max_ms'] for r in runs[k]) / m:.4f}")
        lines.append(f"        here - parent = {b - a:+.4f} ms ({(b - a) / a * 100.0:+.1f} %); the parent's own spread is {spread:.4f} ms: "
                     f"{'inside' if inside else 'OUTSIDE'}")
        rows.append(dict(workload=name, members=m, parent_ms=med["parent"], here_ms=med["here"], parent_median_ms=a, here_median_ms=b,
                         parent_spread_ms=spread, inside=inside))
    lines.append(json.dumps(dict(tool="scan_group_timing --single-ab", children=children, repeats=repeats, rows=rows)))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--members", type=int, default=1)
    ap.add_argument("--single-ab", action="store_true", help="the single call here against VISFS_BA_PARENT_LIB's")
    ap.add_argument("--children", type=int, default=5)
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.child, a.members, a.repeats))
    if a.single_ab:
        sys.exit(single_ab(a.children, a.repeats, a.out))
    lines = []
    for name, m in WORKLOADS:
        lines.append(run_child(name, m, a.repeats, os.environ.get("VISFS_BA_LIB")))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
