"""examples/tracker_step.cpp: the image front end of one frame in plain C++ (VISFS::FlowTracker over include/visfs_flow.h, then
visfs_window_insert)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("tracker_step") / "tracker_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "tracker_step.cpp"), "-L" + libdir,
                    "-lvisfs_window", "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def test_example_compiles(example):
    assert os.access(example, os.X_OK)


@pytest.mark.gpu
def test_example_tracks_triangulates_and_inserts(example):
    res = subprocess.run([example, "4"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["frames"] == out["inserted"] == 4
    # 300 words, at most 10 % lost over the run; flow within the 1.5 px gate; depth within what 0.5 px of disparity makes at 5 m
    assert out["words"] >= 0.9 * 4 * 300 and out["tracked"] >= 0.9 * 3 * 300
    assert out["max_flow_err_px"] <= 1.5
    assert out["max_depth_err_m"] <= 435.2 * 0.11 / (435.2 * 0.11 / 5.0 - 0.5) - 5.0
