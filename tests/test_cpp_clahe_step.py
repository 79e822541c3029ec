"""examples/clahe_step.cpp: two equalised frames, corners and a track in plain C++ (VISFS::FlowTracker::pushFrameCLAHE over
include/visfs_clahe.h), against the same steps on the host twin."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 400


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("clahe_step") / "clahe_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "clahe_step.cpp"), "-L" + libdir,
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


def _fnv(chunks):
    h = 1469598103934665603
    for c in chunks:
        for b in c:
            h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    return f"{h:016x}"


@pytest.mark.gpu
def test_example_equals_the_host_twin(example, tmp_path):
    from visfs_amd import clahe, corners, flow
    prefix = str(tmp_path / "img")
    res = subprocess.run([example, prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(out)
    f = flow.Flow(flow.default_params(), W, H)
    clahe.push_frame(f, clahe.default_params(), _pgm(prefix + "_1_left.pgm"), _pgm(prefix + "_1_right.pgm"))
    xy = corners.corners(f, max_corners=300, quality_level=0.01, min_distance=20.0)
    clahe.push_frame(f, clahe.default_params(), _pgm(prefix + "_2_left.pgm"), _pgm(prefix + "_2_right.pgm"))
    to, st, _ = f.track(xy)
    f.close()
    assert out["corners"] == len(xy) and out["tracked"] == int(st.sum())
    assert out["digest"] == _fnv([xy.tobytes(), to.tobytes(), st.tobytes()])
    assert _pgm(prefix + "_1_left.pgm").min() >= 112 and _pgm(prefix + "_1_left.pgm").max() <= 143
    assert out["corners"] > 50 and out["tracked"] >= 0.9 * out["corners"]
    assert out["max_flow_err_px"] <= 1.5
