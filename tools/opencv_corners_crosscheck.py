"""Hand-off: the corner extraction against OpenCV itself, for a machine that has `cv2` (none of this project's machines does; no test
imports this file).  Runs cv2.goodFeaturesToTrack and cv2.cornerMinEigenVal under the reference's settings (Parameters.h:148-150,
Tracker.cpp:116-141, :181, :327) and the host twin of include/visfs_corners.h on the inputs of tests/corners_cases.py, and prints
where the two differ: the response map (OpenCV adds scaled floats, the library exact integers: float rounding is expected), the mask
of cv2.circle discs (expected identical), and the corners (expected identical wherever no two responses are within that rounding).

    python tools/opencv_corners_crosscheck.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cv_mask(cv2, w, h, discs):
    mask = np.full((h, w), 255, dtype=np.uint8)
    drawn = []
    for x, y, r in discs:
        c = (int(np.rint(np.float32(x))), int(np.rint(np.float32(y))))
        inside = 0 <= c[0] < w and 0 <= c[1] < h
        if inside and mask[c[1], c[0]] != 255:
            drawn.append(0)
            continue
        drawn.append(1)
        cv2.circle(mask, c, int(r), 0, -1)
    return mask, np.array(drawn, dtype=np.uint8)


def main():
    import cv2                                   # absent: ImportError, nothing to report
    from visfs_amd import corners, flow
    import corners_cases as cc
    import flow_cases as fc
    w, h = 752, 480
    inputs = [("base_image", fc.base_image(w, h), None, 300, 40.0), ("base_image, min_distance 7", fc.base_image(w, h), None, 300, 7.0),
              ("mask scenario", fc.base_image(w, h), cc.mask_scenario(w, h), 204, 40.0), ("squares", cc.squares_image()[0], None, 300, 10.0),
              ("noise", cc.noise_image(), None, 300, 7.0)]
    for name, img, discs, mc, md in inputs:
        f = flow.Flow(flow.default_params(), w, h)
        f.push_frame(img, img)
        got = corners.corners(f, discs=discs, max_corners=mc, min_distance=md)
        st = corners.download(f)
        f.close()
        mask = None
        if discs is not None:
            mask, drawn = cv_mask(cv2, w, h, discs)
            print(f"{name}: mask pixels that differ {int((mask != st['mask']).sum())}, draw decisions that differ {int((drawn != st['disc_drawn']).sum())}")
        eig = cv2.cornerMinEigenVal(img, 3, ksize=3)
        rel = np.abs(eig - st["eig"]) / max(float(st["eig"].max()), 1e-30)
        want = cv2.goodFeaturesToTrack(img, mc, 0.01, md, mask=mask)
        want = np.zeros((0, 2), np.float32) if want is None else want.reshape(-1, 2)
        n = min(len(want), len(got))
        first = next((i for i in range(n) if tuple(want[i]) != tuple(got[i])), n)
        common = len(set(map(tuple, want.tolist())) & set(map(tuple, got.tolist())))
        print(f"{name}: response |cv2 - library| / max: {rel.max():.3e}; corners cv2 {len(want)}, library {len(got)}, common {common}, "
              f"same order up to index {first}")


if __name__ == "__main__":
    main()
