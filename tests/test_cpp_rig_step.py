"""examples/rig_step.cpp: four cameras per frame through one call of VISFS::ResidentTrackerGroup (include/visfs_tracker_group.h), each
camera's words into a window of its own, the four windows through one visfs_ba_solve_batch, in plain C++."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import build
    build.build_host()
    exe = str(tmp_path_factory.mktemp("rig_step") / "rig_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "rig_step.cpp"), "-L" + libdir,
                    "-lvisfs_window", "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def _check(out, frames):
    assert out["cameras"] == 4 and out["frames"] == frames
    assert out["inserted"] == 4 * (frames - 1) and out["bootstrapped"] == 4          # every camera bootstraps once, in frame 2
    assert out["words"] >= 0.9 * 4 * (frames - 1) * 300                               # 300 words asked for, at most 10 % missing
    # depth within what 0.5 px of disparity makes at 5 m (the stereo gate)
    assert out["max_depth_err_m"] <= 435.2 * 0.11 / (435.2 * 0.11 / 5.0 - 0.5) - 5.0


def test_example_compiles_and_runs_on_the_host_twins(example):
    assert os.access(example, os.X_OK)
    res = subprocess.run([example, "3", "host"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    _check(out, 3)
    assert out["kernel_launches_max"] == 0 and out["synchronisations_last"] == 0 and out["windows_solved"] == 0


@pytest.mark.gpu
def test_example_tracks_four_cameras_and_solves_their_windows(example):
    res = subprocess.run([example, "5"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    _check(out, 5)
    assert out["windows_solved"] == 4
    # the poses handed to the BA are the true ones: it moves them by less than the 2 px reprojection gate is at 5 m
    assert out["max_pose_shift_m"] <= 2.0 * 5.0 / 435.2
    assert 0 < out["kernel_launches_last"] < out["kernel_launches_max"] and out["synchronisations_last"] <= 2
