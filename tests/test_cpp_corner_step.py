"""examples/corner_step.cpp: the pixel path of a frame in plain C++ with the tracker's own corners (VISFS::FlowTracker over
include/visfs_corners.h and include/visfs_flow.h, then visfs_window_insert)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MAX_FEATURES, MIN_DISTANCE, QUALITY = 640, 400, 300, 40, 0.01


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("corner_step") / "corner_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "corner_step.cpp"), "-L" + libdir,
                    "-lvisfs_window", "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def test_example_compiles(example):
    assert os.access(example, os.X_OK)


def _pgm(path):
    with open(path, "rb") as fp:
        assert fp.readline() == b"P5\n"
        w, h = (int(v) for v in fp.readline().split())
        assert fp.readline() == b"255\n"
        return np.frombuffer(fp.read(), dtype=np.uint8).reshape(h, w).copy()


def _host_twin_run(prefix, frames):
    """The example's loop on the host twin: per frame (words before the top-up, new corners)."""
    from visfs_amd import corners, flow
    f = flow.Flow(flow.default_params(), W, H)
    pts, cnt = np.zeros((0, 2), dtype=np.float32), []
    before, new = [], []
    for k in range(1, frames + 1):
        f.push_frame(_pgm(f"{prefix}_{k}_left.pgm"), _pgm(f"{prefix}_{k}_right.pgm"))
        if k > 1:
            to, st, _ = f.track(pts)
            ok = (st == 1) & (to[:, 0] >= 0) & (to[:, 0] < W) & (to[:, 1] >= 0) & (to[:, 1] < H)
            pts, cnt = to[ok], [c + 1 for c, o in zip(cnt, ok) if o]
        before.append(len(pts))
        added = 0
        if MAX_FEATURES - len(pts) > 0:
            order = sorted(range(len(pts)), key=lambda i: -cnt[i])                  # stable, as FlowTracker::maskDiscs
            discs = [(float(pts[i][0]), float(pts[i][1]), MIN_DISTANCE) for i in order]
            fresh = corners.corners(f, discs=discs, max_corners=MAX_FEATURES - len(pts), quality_level=QUALITY, min_distance=float(MIN_DISTANCE))
            pts = np.concatenate([pts, fresh]).astype(np.float32)
            cnt += [1] * len(fresh)
            added = len(fresh)
        new.append(added)
    f.close()
    return before, new


@pytest.mark.gpu
def test_example_makes_its_own_corners_and_inserts(example, tmp_path):
    frames = 4
    prefix = str(tmp_path / "img")
    res = subprocess.run([example, str(frames), prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(out)
    assert out["frames"] == out["inserted"] == frames
    before, new = _host_twin_run(prefix, frames)
    assert out["words_before_top_up"] == before and out["new_corners"] == new
    assert out["words_before_top_up"][0] == 0 and out["new_corners"][0] > 50       # the first frame has only its own corners
    assert out["tracked"] >= 0.9 * sum(b + n for b, n in zip(before[:-1], new[:-1]))
    assert out["words"] >= 0.9 * sum(b + n for b, n in zip(before, new))
    assert out["max_flow_err_px"] <= 1.5
    assert out["max_depth_err_m"] <= 435.2 * 0.11 / (435.2 * 0.11 / 5.0 - 0.5) - 5.0
