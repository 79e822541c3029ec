"""Hand-off: the flow front end against OpenCV itself, for a machine that has `cv2` (none of this project's machines does; no test
imports this file).  Tracks the synthetic frames of tests/flow_cases.py with cv2.calcOpticalFlowPyrLK under the reference's settings
(Tracker.cpp:257-274) and with the host twin of include/visfs_flow.h, and prints how far the two land apart.

    python tools/opencv_flow_crosscheck.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cv2                                   # absent: ImportError, nothing to report
    from visfs_amd import flow
    import flow_cases as fc
    w, h = 752, 480
    first = fc.base_image(w, h)
    second = fc.moved_pair(w, h)[0]
    pts = fc.truth_points(w, h)
    crit = (cv2.TERM_CRITERIA_COUNT + cv2.TERM_CRITERIA_EPS, 30, 0.01)
    kw = dict(winSize=(21, 21), maxLevel=3, criteria=crit, minEigThreshold=1e-4)
    to, st, err = cv2.calcOpticalFlowPyrLK(first, second, pts.reshape(-1, 1, 2), None, flags=cv2.OPTFLOW_LK_GET_MIN_EIGENVALS, **kw)
    back, rst, _ = cv2.calcOpticalFlowPyrLK(second, first, to, pts.reshape(-1, 1, 2).copy(),
                                            flags=cv2.OPTFLOW_LK_GET_MIN_EIGENVALS | cv2.OPTFLOW_USE_INITIAL_FLOW, **kw)
    keep_cv = (st.ravel() != 0) & (rst.ravel() != 0) & (np.linalg.norm(back.reshape(-1, 2) - pts, axis=1) <= 1.5)
    f = flow.Flow(flow.default_params(), w, h)
    f.push_frame(first, first)
    f.push_frame(second, second)
    to_l, st_l, err_l = f.track(pts)
    both = keep_cv & (st_l == 1)
    d = np.linalg.norm(to.reshape(-1, 2)[both] - to_l[both], axis=1)
    print(f"kept: cv2 {int(keep_cv.sum())}, library {int(st_l.sum())}, both {int(both.sum())} of {len(pts)}")
    print(f"|cv2 - library| over points both keep: max {d.max():.3e} px, median {np.median(d):.3e} px")
    print(f"minimum eigenvalue, relative difference: max {np.max(np.abs(err.ravel()[both] - err_l[both]) / err_l[both]):.3e}")


if __name__ == "__main__":
    main()
