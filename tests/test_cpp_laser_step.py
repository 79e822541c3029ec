"""examples/laser_step.cpp: one laser-strategy frame in plain C++ (VISFS::Map::ActiveSubmaps2D over include/visfs_submap.h)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(src, exe):
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), src, "-L" + libdir, "-lvisfs_ba_hip",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def binaries(tmp_path_factory, hiplib):
    d = tmp_path_factory.mktemp("laser_step")
    return (_build(os.path.join(ROOT, "examples", "laser_step.cpp"), str(d / "laser_step")),
            _build(os.path.join(ROOT, "tests", "cpp", "laser_driver.cpp"), str(d / "laser_driver")))


def test_example_and_driver_compile(binaries):
    for exe in binaries:
        assert os.access(exe, os.X_OK)


@pytest.mark.gpu
def test_driver_runs_three_frames(binaries):
    res = subprocess.run([binaries[1]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["frames"] == 3 and out["solved"] == 2


@pytest.mark.gpu
def test_example_runs_through_the_submap_life_cycle(binaries):
    res = subprocess.run([binaries[0], "24"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["frames"] == 24 and out["solved"] == 23 and out["submaps"] == 2 and out["max_err_m"] < 0.3
