#!/usr/bin/env python3
"""Times AMCL's pose hypotheses on the KLD filter (include/visfs_mcl_hyp.h), the C call visfs_mcl_update only, at a capacity of
N = 3000 with 30 and 200 beams, on the workloads of tools/mcl_kld_timing.py:

  kld_full     the belief is wide (initialised again before every second update): every resampling keeps all 3000 draws;
  kld_settled  a robot that stands still with a narrow belief, read after 40 updates, at the count it has settled at;

each with the hypotheses on and off.  The device and the one-core host twin run in step and a figure is reported only if they
returned the same bytes in every result of every update (the hypotheses included) and in every array at the end; otherwise the
tool stops.  Medians over the updates that resampled and over those that did not.

With --parent LIB (the library built from the parent commit) the KLD update without hypotheses is then timed against it on
kld_full: fresh child processes in turn, one library each (VISFS_BA_LIB), ROUNDS rounds; the parent's spread is the least and the
largest of its medians, and the tool ends with a failure status when this library's median lies above it.  (Two copies of the
library cannot share a process, so the parent's filter does not run in the process of the other two.)  The propagation rounds of the room scene, the snake and N = 16384 of tests/mcl_hyp_cases.py are recorded
too.  Writes profiles/mcl_hyp_timing.log.

usage: tools/mcl_hyp_timing.py [--updates U] [--rounds R] [--parent LIB] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                 # noqa: E402

import mcl_kld_timing as kt                        # noqa: E402
from visfs_amd import abi, backend                 # noqa: E402
from visfs_amd import mcl                          # noqa: E402
from visfs_amd import mcl_kld as kld               # noqa: E402

N, BEAMS, TRUTH = kt.N, kt.BEAMS, kt.TRUTH
WORKLOADS = (("kld_full", (3.0, 3.0, 1.0), 4, True), ("kld_settled", (0.3, 0.3, 0.2), 40, False))


def run(lib, flt, pts, sigma, warm, updates, reinit, extra=None):
    """The filters of `flt` in step; {name: (times of the updates that did not resample, of those that did)}, the device's counts
    and hypotheses' rounds."""
    prm = mcl.default_params()
    times = {k: ([], []) for k in flt}
    counts, rounds = [], []
    for u in range(warm + updates):
        delta = np.array([0.02, 0.0, 0.01]) * (1.0 if u % 2 == 0 else -1.0)
        res = {}
        for k, f in flt.items():
            if reinit and u % 2 == 0:
                assert f.init(TRUTH, sigma) == abi.OK
            dt, out = kt.update(lib, f, prm, delta, pts)
            res[k] = bytes(out) + json.dumps(kld.last(f)).encode() + (extra(f) if extra else b"")
            if u >= warm:
                times[k][out.resampled].append(dt)
        if len(set(res.values())) != 1:
            sys.exit(f"update {u}: the device and the twin differ; nothing is reported")
        if u >= warm and "device" in flt:
            counts.append(kld.count(flt["device"]))
            if extra and out.resampled:
                from visfs_amd import mcl_hyp as hyp
                rounds.append(hyp.rounds(flt["device"])[1])
    return times, counts, rounds


def scenario(lib, fields, name, hyp_on, pts, sigma, warm, updates, reinit):
    from visfs_amd import mcl_hyp as hyp
    flt = {k: mcl.Filter(f, N, 11) for k, f in fields.items()}
    for f in flt.values():
        assert f.status == abi.OK and kld.enable(f) == abi.OK, f.last_error()
        if hyp_on:
            assert hyp.enable(f) == abi.OK, f.last_error()
        assert f.init(TRUTH, sigma) == abi.OK
    times, counts, rounds = run(lib, flt, pts, sigma, warm, updates, reinit, (lambda f: hyp.last_bytes(f)[1]) if hyp_on else None)
    a, b = kld.download(flt["device"]), kld.download(flt["twin"])
    if any(a[key].tobytes() != b[key].tobytes() for key in a):
        sys.exit(f"{name}: the device's particles and the twin's differ; nothing is reported")
    lines, med = [], {}
    for k in ("device", "twin"):
        skip, ran = times[k]
        med[k] = (kt.med(ran), kt.med(skip))
        lines.append(f"{name} {'hyp' if hyp_on else 'off'} {len(pts)} {k} {min(counts)} {max(counts)} " + " ".join(str(v) for v in flt[k].last_counts())
                     + f" {kt.med(ran):.4f} {kt.med(skip):.4f}" + (f" rounds {min(rounds)}..{max(rounds)}" if rounds and k == "device" else ""))
        print(lines[-1], flush=True)
    for f in flt.values():
        f.close()
    return lines, med


def child(updates):
    """kld_full without hypotheses on whatever library VISFS_BA_LIB names: one JSON line, {beams: [resampling ms, not resampling ms]}."""
    solver = backend.Solver(abi.default_params())
    lib = kld.load()
    cells, lim = kt.room()
    field = mcl.Field.from_grid(cells, lim, solver=solver)
    assert field.status == abi.OK
    out = {}
    for n in BEAMS:
        f = mcl.Filter(field, N, 11)
        assert f.status == abi.OK and kld.enable(f) == abi.OK and f.init(TRUTH, WORKLOADS[0][1]) == abi.OK
        times, _, _ = run(lib, {"device": f}, kt.scan(cells, lim, n), WORKLOADS[0][1], 20, updates, True)
        out[str(n)] = [kt.med(times["device"][1]), kt.med(times["device"][0])]
        f.close()
    field.close()
    solver.close()
    print(json.dumps(out))


def case_rounds(solver):
    """The device's propagation rounds on three cases of tests/mcl_hyp_cases.py."""
    import mcl_hyp_cases as hc
    import mcl_hyp_lib as hl
    field = hl.field_of("room", solver)
    out = []
    for name, case in (("room", hc.room_case(1)), ("snake", hc.all_cases()["snake"]), ("N16384", hc.fullest_case())):
        lib = hl.Library(case, field)
        trace = hc.play(case, lib)
        r = [v for v, t in zip(lib.rounds, trace) if t[0]["resampled"]]
        out.append(f"# hook_rounds {name}: {r} (bins {[t[1]['bins'] for t in trace if t[0]['resampled']]})")
        lib.close()
    field.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="the parent commit's libvisfs_ba_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcl_hyp_timing.log"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.updates)
    solver = backend.Solver(abi.default_params())
    lib = kld.load()
    cells, lim = kt.room()
    fields = {"device": mcl.Field.from_grid(cells, lim, solver=solver), "twin": mcl.Field.from_grid(cells, lim)}
    assert all(f.status == abi.OK for f in fields.values())
    lines = ["# tools/mcl_hyp_timing.py: median wall times of visfs_mcl_update in ms, capacity 3000, the device and the twin in step, equal in every byte",
             "# workload hypotheses beams flavour count_min count_max launches copies waits resampling_ms not_resampling_ms"]
    for n in BEAMS:
        pts = kt.scan(cells, lim, n)
        for name, sigma, warm, reinit in WORKLOADS:
            med = {}
            for on in (True, False):
                got, med[on] = scenario(lib, fields, name, on, pts, sigma, warm, args.updates, reinit)
                lines += got
            for k in ("device", "twin"):
                lines.append(f"# {name} {n} beams, {k}: a resampling update with hypotheses takes {med[True][k][0] / med[False][k][0]:.3f} of one without "
                             f"({med[True][k][0]:.4f} / {med[False][k][0]:.4f} ms)")
                print(lines[-1], flush=True)
    for f in fields.values():
        f.close()
    lines += case_rounds(solver)
    print("\n".join(lines[-3:]), flush=True)
    solver.close()

    if args.parent:
        lines.append(f"# kld_full without hypotheses, this library and the parent's in turn, a fresh process each, {args.rounds} rounds: "
                     "library beams kind medians_ms")
        got = {name: {str(n): ([], []) for n in BEAMS} for name in ("parent", "this")}
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
                    got[name][k][0].append(v[0])
                    got[name][k][1].append(v[1])
        first = len(lines)
        for n in BEAMS:
            for j, kind in enumerate(("resampling", "not_resampling")):
                p, t = got["parent"][str(n)][j], got["this"][str(n)][j]
                for name, v in (("parent", p), ("this", t)):
                    lines.append(f"{name} {n} {kind} " + " ".join(f"{x:.4f}" for x in v))
                inside = statistics.median(t) <= max(p)
                lines.append(f"# {n} beams, {kind}: the parent's spread {min(p):.4f} .. {max(p):.4f} ms, this library's median "
                             f"{statistics.median(t):.4f} ms: " + ("inside (not above it)" if inside else "ABOVE the spread"))
        print("\n".join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if any("ABOVE the spread" in l for l in lines):
        sys.exit("hypotheses off: a median lies above the parent's own spread (the log is written)")


if __name__ == "__main__":
    main()
