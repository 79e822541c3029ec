"""Lucas-Kanade front end against the ground truth of the synthetic scenes (tests/flow_cases.py): kept points, maximum and median
error of track and of stereo on the three depth scenes, on the host twin and, with --gpu, on the device.

    python tools/flow_accuracy.py [--gpu] [--out profiles/flow_accuracy.log]
"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from visfs_amd import abi, backend  # noqa: E402
from visfs_amd import flow  # noqa: E402
import flow_cases as fc  # noqa: E402


def run(solver):
    w, h = 752, 480
    f = flow.Flow(flow.default_params(), w, h, solver=solver)
    f.push_frame(fc.base_image(w, h), fc.base_image(w, h))
    left, right, _, _ = fc.moved_pair(w, h)
    f.push_frame(left, right)
    fc.check_track_truth(f.track)
    cam = flow.camera()
    for kind in ("plane", "slant", "step"):
        l, r, d = fc.still_pair(w, h, kind)
        f.push_frame(l, r)
        fc.check_stereo_truth(lambda p: f.stereo(p, cam), kind, d.fb)
    f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        print("flow_accuracy: 752 x 480, 300 points >= 40 px from the border; motion (9, -7.5) px + 0.01 rad + zoom 1.01; depth 5 m / 5 -> 3.5 m")
        print("gates: track 1.5 px, stereo 0.5 px (Tracker.cpp:268, :364); at most 10 % of the qualifying points dropped")
        print("-- host twin")
        run(None)
        if a.gpu:
            print("-- device")
            s = backend.Solver(abi.default_params())
            run(s)
            s.close()
    text = buf.getvalue()
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
