"""Wall time of one marginal-covariance call (visfs_ba_graph_covariance) after `optimize` on the resident graph: PROD, C2 (Solver 0 and
Solver 2) and C4, with and without the landmark marginals; median over repeats (the first call, which allocates the scratch, is
reported on its own).
usage: python tools/cov_timing.py [--repeats 20] [--out profiles/cov_timing.log]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from visfs_amd import abi, backend, synth

CASES = [("PROD", 0), ("C2", 0), ("C2", 2), ("C4", 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = backend.load_library()
    lines = []
    for cfg, solver in CASES:
        prm = abi.default_params(iterations=10, solver=solver)
        wb = abi.WindowBuffers(synth.make_window(cfg))
        gb, _, _, _ = abi.pack_window_with(lib.visfs_ba_pack_window, prm, wb)
        s = backend.Solver(prm)
        s.upload(gb)
        rc, _ = s.optimize()
        assert rc == abi.OK, rc
        info = s.describe()
        t0 = time.perf_counter(); s.covariance(points=True, cross=True); first = (time.perf_counter() - t0) * 1e3
        row = dict(config=cfg, solver=solver, n_free_poses=info["n_free_poses"], n_points=info["n_points"],
                   first_call_ms=round(first, 3))
        for points in (False, True):
            ts = []
            for _ in range(a.repeats):
                t0 = time.perf_counter(); s.covariance(points=points, cross=True); ts.append((time.perf_counter() - t0) * 1e3)
            row["median_ms_points" if points else "median_ms_poses_only"] = round(float(np.median(ts)), 3)
            row["min_ms_points" if points else "min_ms_poses_only"] = round(float(np.min(ts)), 3)
        s.close()
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/cov_timing.py --repeats %d: wall time of visfs_ba_graph_covariance after optimize (host call incl. copies)\n" % a.repeats)
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
