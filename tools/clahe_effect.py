"""What the equalised push changes on a low-contrast scene (reported, not asserted): the synthetic scene of tools/flow_accuracy.py
(752 x 480, known motion) with its contrast cut to an eighth around grey level 112, pushed with and without CLAHE.  Per way: corners
found on the first left image (300 asked for, quality 0.01, minimum distance 20), points of them tracked into the second, and their
error against the true motion.

    python tools/clahe_effect.py [--host] [--out profiles/clahe_effect.log]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend, clahe, corners, flow  # noqa: E402
import flow_cases as fc  # noqa: E402


def squeeze(img):
    return (112 + img.astype(np.int32) // 8).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="the host twin instead of the device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = 752, 480
    first = squeeze(fc.base_image(w, h))
    left, right, motion, _ = fc.moved_pair(w, h)
    left, right = squeeze(left), squeeze(right)
    s = None if a.host else backend.Solver(abi.default_params())
    lines = [f"clahe_effect: {w} x {h}, the scene of flow_accuracy at 1/8 contrast (grey levels 112 .. 143), "
             f"{'host twin' if a.host else 'device'}; corners: 300 asked, quality 0.01, min distance 20; track gate 1.5 px"]
    for name, eq in (("plain push_frame", False), ("push_frame_clahe", True)):
        f = flow.Flow(flow.default_params(), w, h, solver=s)
        push = (lambda l, r: clahe.push_frame(f, clahe.default_params(), l, r)) if eq else f.push_frame
        push(first, first)
        xy = corners.corners(f, max_corners=300, quality_level=0.01, min_distance=20.0)
        push(left, right)
        to, st, _ = f.track(xy)
        ok = st == 1
        line = f"{name:<18} corners {len(xy):>4}, tracked {int(ok.sum()):>4}"
        if ok.any():
            err = np.sqrt(((to[ok] - motion.forward(xy[ok])) ** 2).sum(axis=1))
            line += f", error max {err.max():.4f} px, median {np.median(err):.4f} px"
        lines.append(line)
        f.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    if s is not None:
        s.close()


if __name__ == "__main__":
    main()
