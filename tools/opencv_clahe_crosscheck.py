"""Hand-off: the equalised push against OpenCV itself, for a machine that has `cv2` (none of this project's machines does; no test
imports this file).  Runs cv2.createCLAHE(clipLimit, tileGridSize).apply under the reference's settings (System.cpp:107-111) and the
host twin of include/visfs_clahe.h on the inputs of tests/clahe_cases.py and on one 752 x 480 pair, and prints how many bytes differ
and by how much.  Expected: none, on an OpenCV build whose 8-bit CLAHE runs the CPU path (no OpenCL); a difference is a point where
DESIGN.md section 9g restates OpenCV wrongly and belongs into that section.

    python tools/opencv_clahe_crosscheck.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cv2                                   # absent: ImportError, nothing to report
    from visfs_amd import clahe, flow
    import clahe_cases as cc
    cv2.ocl.setUseOpenCL(False)
    inputs = [(c["name"], c["params"], c["left"], c["right"], cc.FLOW_PARAMS) for c in cc.cases()]
    inputs.append(("752x480", cc.DEFAULT, *cc.big_pair(), {}))
    for name, prm, left, right, fprm in inputs:
        h, w = left.shape
        f = flow.Flow(flow.default_params(**fprm), w, h)
        clahe.push_frame(f, clahe.default_params(**prm), left, right)
        cv = cv2.createCLAHE(clipLimit=prm["clip_limit"], tileGridSize=(prm["tiles_x"], prm["tiles_y"]))
        for image, src in enumerate((left, right)):
            got = f.download_level(flow.SLOT_CURRENT, image, 0)[0]
            d = np.abs(cv.apply(src).astype(np.int32) - got.astype(np.int32))
            print(f"{name} image {image}: bytes that differ {int((d > 0).sum())} of {d.size}, largest difference {int(d.max())}")
        f.close()


if __name__ == "__main__":
    main()
