"""Hand-off: the PnP-RANSAC pose guess against OpenCV itself, for a machine that has `cv2` (none of this project's machines does; no
test imports this file).  Runs cv2.solvePnPRansac (SOLVEPNP_P3P is not what the reference's default flag selects; both it and
SOLVEPNP_ITERATIVE are tried) and the refit cv2.solvePnP on its inliers under the reference's settings (Parameters.h: 50 iterations,
2.0 px, confidence 0.99) and the host twin of include/visfs_pnp.h on the scenes of tests/pnp_cases.py, and prints how far the two
results lie apart.  OpenCV draws its samples from its own random stream and stops early, so the hypotheses differ by construction;
what is expected to agree is the inlier set of the RANSAC stage on scenes whose outliers are far from the threshold, and then the
refit pose to the precision of the two minimisers.

    python tools/opencv_pnp_crosscheck.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cv2                                   # absent: ImportError, nothing to report
    from visfs_amd import pnp
    import pnp_cases as pc
    Kcv = np.array([[pc.K[0], 0, pc.K[2]], [0, pc.K[1], pc.K[3]], [0, 0, 1]], dtype=np.float64)
    twin = pnp.Pnp(pnp.MAX_POINTS)
    for name in sorted(pc.CASES):
        s = pc.case(name)
        twin.solve(pnp.default_params(**s["params"]), pnp.camera(*pc.K, Tir=pc.TIR), s["from_xyz"], s["to_xy"], None)
        st = twin.download()
        if st["winner"] < 0:
            print(f"{name}: the library found no hypothesis")
            continue
        ours = set(int(i) for i in np.nonzero(_errors(st["models"][st["winner"]], s) <= np.float32(2.0))[0])
        for flag_name in ("SOLVEPNP_ITERATIVE", "SOLVEPNP_P3P"):
            ok, rvec, tvec, inl = cv2.solvePnPRansac(s["from_xyz"], s["to_xy"], Kcv, None, iterationsCount=50, reprojectionError=2.0,
                                                     confidence=0.99, flags=getattr(cv2, flag_name))
            if not ok or inl is None:
                print(f"{name} [{flag_name}]: cv2.solvePnPRansac failed")
                continue
            theirs = set(int(i) for i in inl.ravel())
            R, _ = cv2.Rodrigues(rvec)
            q = st["refit_tq"]
            Rl = _quat_R(q[3:])
            ang = np.arccos(np.clip((np.trace(R.T @ Rl) - 1) / 2, -1, 1))
            print(f"{name} [{flag_name}]: RANSAC inliers cv2 {len(theirs)}, library {len(ours)}, common {len(ours & theirs)}; refit pose "
                  f"apart by {ang:.3e} rad, {np.linalg.norm(tvec.ravel() - q[:3]):.3e} m")
    twin.close()


def _errors(M, s):
    import pnp_oracle as po
    import pnp_cases as pc
    return po.errors(M[:, :3], M[:, 3], pc.K, s["from_xyz"].astype(np.float64), s["to_xy"].astype(np.float64))


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


if __name__ == "__main__":
    main()
