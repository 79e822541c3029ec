"""examples/frame_step.cpp: one frame from the images to the window in plain C++ (VISFS::ResidentTracker over
include/visfs_tracker.h, then visfs_pnp_solve on the covisible rows and visfs_window_insert)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("frame_step") / "frame_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "frame_step.cpp"), "-L" + libdir,
                    "-lvisfs_window", "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def _check(out, frames):
    assert out["frames"] == frames and out["inserted"] == frames - 1 and out["bootstrapped"] == 1
    # the first guess is the identity and the one after the first call still is: the wrapper hands neither on (Tracker.cpp:237)
    assert out["identity_guesses"] == 2
    # 300 words asked for, at most 10 % missing over the run; every PnP call finds Estimator/MinInliers inliers
    assert out["words"] >= 0.9 * (frames - 1) * 300 and out["covisible"] >= 0.9 * (frames - 1) * 300
    assert out["min_pnp_inliers"] >= 12
    # the pose within what the 2 px reprojection gate of PnP is at 5 m; depth within what 0.5 px of disparity makes there
    assert out["max_translation_err_m"] <= 2.0 * 5.0 / 435.2
    assert out["max_depth_err_m"] <= 435.2 * 0.11 / (435.2 * 0.11 / 5.0 - 0.5) - 5.0


def test_example_compiles_and_runs_on_the_host_twins(example):
    assert os.access(example, os.X_OK)
    res = subprocess.run([example, "3", "host"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    _check(json.loads(res.stdout.strip().splitlines()[-1]), 3)


@pytest.mark.gpu
def test_example_tracks_solves_and_inserts(example):
    res = subprocess.run([example, "5"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    _check(json.loads(res.stdout.strip().splitlines()[-1]), 5)
