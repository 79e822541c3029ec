"""Hand-off: the fundamental-matrix cull against OpenCV itself, for a machine that has `cv2` (none of this project's machines does;
no test imports this file).  Runs cv2.findFundamentalMat(from, to, FM_RANSAC, 1.0, 0.99) as Tracker::rejectOutlierWithFundationMatrix
calls it and the host twin of include/visfs_fund.h on the scenes of tests/fund_cases.py, and prints how far the two results lie
apart.  OpenCV draws its samples from its own random stream and stops early at confidence 0.99, so the winning seven-point models
differ by construction; what is expected to agree is the mask on rows far from the threshold (the displaced rows out, most true rows
in) and, between the two F scaled alike, the symmetric epipolar error of the common inliers.

    python tools/opencv_fund_crosscheck.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cv2                                   # absent: ImportError, nothing to report
    from visfs_amd import fund
    import fund_cases as fc
    import fund_oracle as fo
    twin = fund.Fund(fund.MAX_POINTS)
    for name in sorted(fc.CASES):
        s = fc.case(name)
        out = twin.cull(fund.default_params(**s["params"]), s["from_xy"], s["to_xy"], s["status"])
        F, mask = cv2.findFundamentalMat(s["from_xy"], s["to_xy"], cv2.FM_RANSAC, 1.0, 0.99)
        if F is None or mask is None or F.shape != (3, 3):
            print(f"{name}: cv2.findFundamentalMat returned no single model")
            continue
        theirs, ours = mask.ravel().astype(bool), out["mask"].astype(bool)
        both = theirs & ours
        xy1, xy2 = s["from_xy"].astype(np.float64), s["to_xy"].astype(np.float64)
        e_cv = np.sqrt(fo.errors(F, xy1, xy2).astype(np.float64))
        e_us = np.sqrt(fo.errors(out["F"], xy1, xy2).astype(np.float64))
        bad = s["displaced"]
        print(f"{name}: inliers cv2 {theirs.sum()}, library {ours.sum()}, common {both.sum()}; displaced rows kept cv2 {(theirs & bad).sum()}, "
              f"library {(ours & bad).sum()} of {bad.sum()}; error of the common inliers under cv2's F {e_cv[both].mean():.3f} px, under the "
              f"library's {e_us[both].mean():.3f} px")
    twin.close()


if __name__ == "__main__":
    main()
