"""Branch-and-bound scan matching over frozen grid stacks: build and match times on the GPU (each call timed with its own stream
wait) against the exhaustive device matcher and against the one-core host twin on the same machine.

Three workloads, each measured in a child process of its own under a time limit:
  build    the stack of the `room` and `hall` grids of tools/scan_match_timing.py, depth 7: device build (freeze of device sub-maps,
           device to device, up to its wait) and the one-core twin's;
  nl32     the room, 1 000 returns, the largest window the exhaustive matcher supports (1.6 m: nl = 32, L^2 = 4 225; 0.5 rad): the
           device branch and bound against the device visfs_scan_match with zero weights, alternating, same winner required;
  reloc    the hall, 7 m / 30 degrees, depth 7 (nl = 140, S ~ 630): a search only this matcher can run; device call against the twin.
Nothing is reported unless device and twin agree on the result record and on the per-level counts.  Writes one JSON line per workload.

    python tools/scan_fast_timing.py [--repeats 30] [--out profiles/scan_fast_timing.log]
"""
import argparse
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


def stats(ts):
    v = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), repeats=len(ts))


def submaps_of(name, solver):
    """Device and host sub-maps of a scan_match_timing scene, its guess and points."""
    import scan_match_timing as smt
    from visfs_amd import abi
    from visfs_amd import submap as sm
    frames, guess, pts, _ = smt.scene(name)
    dev = sm.Submaps(sm.default_params(num_range_data_limit=10 ** 6), solver=solver)
    host = sm.Submaps(sm.default_params(num_range_data_limit=10 ** 6))
    for T, rd in frames:
        assert dev.insert(T, rd) == abi.OK and host.insert(T, rd) == abi.OK
    return dev, host, guess, pts


def timed(fn, reps, warm=2):
    ts, r = [], None
    for i in range(reps + warm):
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        if i >= warm:
            ts.append(t1 - t0)
    return ts, r


def agree(sd, sh, rd, rh):
    hd, hh = sd.match_download(), sh.match_download()
    same = rd == rh and (hd["B"], hd["scored"], hd["kept"]) == (hh["B"], hh["scored"], hh["kept"])
    return same and hd["bounds"].tobytes() == hh["bounds"].tobytes() and hd["survivors"].tobytes() == hh["survivors"].tobytes(), hd


def child_build(repeats, host_repeats):
    from visfs_amd import abi, backend
    s = backend.Solver(abi.default_params())
    out = dict(tool="scan_fast_timing", workload="build", depth=DEPTH)
    for name in ("room", "hall"):
        dev, host, _, _ = submaps_of(name, s)
        d = dev.describe()[0]

        def build(sub):
            st = sub.freeze(0, DEPTH)
            assert st.status == abi.OK, sub.last_error()
            return st

        keep = []
        t_dev, _ = timed(lambda: keep.append(build(dev)), repeats)
        t_host, _ = timed(lambda: keep.append(build(host)), host_repeats, warm=1)
        sd, sh = keep[0], keep[-1]
        for h in range(DEPTH):
            if sd.download_level(h)[0].tobytes() != sh.download_level(h)[0].tobytes():
                print(json.dumps(dict(out, error=f"{name}: level {h} differs between device and twin")))
                return 2
        out[name] = dict(grid_cells=[d["num_x_cells"], d["num_y_cells"]], bytes=sd.describe()["bytes"], identical=True,
                         build_gpu=stats(t_dev), build_host_1core=stats(t_host))
        for st in keep:
            st.close()
        dev.close(); host.close()
    print(json.dumps(out))
    s.close()
    return 0


def child_match(name, repeats, host_repeats):
    from visfs_amd import abi, backend
    from visfs_amd import scan_fast as sf
    from visfs_amd import scan_match as scm
    s = backend.Solver(abi.default_params())
    if name == "nl32":
        dev, host, guess, pts = submaps_of("room", s)
        lw, aw = 1.6, 0.5
    else:
        dev, host, guess, pts = submaps_of("hall", s)
        guess = (guess[0] + 5.0, guess[1] - 4.0, guess[2] + 0.3)
        lw, aw = 7.0, 30.0 * np.pi / 180.0
    sd, sh = dev.freeze(0, DEPTH), host.freeze(0, DEPTH)
    assert sd.status == sh.status == abi.OK
    prm = sf.default_params(linear_search_window=lw, angular_search_window=aw)

    def run(st):
        rc, r = st.match(guess, pts, prm)
        assert rc == abi.OK, st.last_error()
        return r

    out = dict(tool="scan_fast_timing", workload=name, depth=DEPTH, points=len(pts))
    if name == "nl32":                                  # alternate the two device matchers, as one compares two versions
        eprm = scm.default_params(linear_search_window=lw, angular_search_window=aw, translation_delta_cost_weight=0.0, rotation_delta_cost_weight=0.0)

        def exhaustive():
            rc, r = dev.match(guess, pts, eprm)
            assert rc == abi.OK, dev.last_error()
            return r

        t_bb, t_ex = [], []
        for i in range(repeats + 2):
            a, rd = timed(lambda: run(sd), 1, warm=0)
            b, re_ = timed(exhaustive, 1, warm=0)
            if i >= 2:
                t_bb += a; t_ex += b
        keys = ("scan_index", "x_offset", "y_offset", "sum", "score", "x", "y", "yaw")
        if any(rd[k] != re_[k] for k in keys):
            print(json.dumps(dict(out, error="branch and bound and the exhaustive matcher disagree", fast=rd, exhaustive=re_)))
            return 2
        out.update(match_exhaustive_gpu=stats(t_ex), candidates=rd["num_scans"] * (2 * rd["num_linear"] + 1) ** 2)
    else:
        t_bb, rd = timed(lambda: run(sd), repeats)
    t_host, rh = timed(lambda: run(sh), host_repeats, warm=1)
    ok, hk = agree(sd, sh, rd, rh)
    if not ok:
        print(json.dumps(dict(out, error="device and host twin disagree", device=rd, host=rh)))
        return 2
    out.update(num_scans=rd["num_scans"], num_linear=rd["num_linear"], depth_used=rd["depth_used"], launches=rd["depth_used"] + 4,
               winner=[rd["scan_index"], rd["x_offset"], rd["y_offset"]], sum=rd["sum"], score=rd["score"], B=hk["B"],
               scored=hk["scored"], kept=hk["kept"], leaves=rd["num_scans"] * (2 * rd["num_linear"] + 1) ** 2, identical=True,
               match_gpu=stats(t_bb), match_host_1core=stats(t_host))
    print(json.dumps(out))
    sd.close(); sh.close(); dev.close(); host.close(); s.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        sys.exit(child_build(a.repeats, a.host_repeats) if a.child == "build" else child_match(a.child, a.repeats, a.host_repeats))
    lines = []
    for name in ("build", "nl32", "reloc"):
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
