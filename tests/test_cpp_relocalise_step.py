"""examples/relocalise_step.cpp: a lost pose recovered by the branch-and-bound search over a frozen sub-map (VISFS::ScanStack and
ActiveSubmaps2D::freeze over include/visfs_scan_fast.h), settled by the weighted local match and handed to the window
solve; `host` runs the one-core twins."""
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
def binary(tmp_path_factory, hiplib):
    d = tmp_path_factory.mktemp("relocalise_step")
    return _build(os.path.join(ROOT, "examples", "relocalise_step.cpp"), str(d / "relocalise_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert out["inserted"] == 5 and out["matched"] == 1 and out["refined"] == 1
    assert (out["num_linear"], out["depth_used"]) == (30, 7)           # 1.5 m at 0.05 m: L = 61, H = 6
    assert out["err_before_m"] > 1.0                                   # (1.1, -0.7): far beyond the exhaustive matcher's default reach
    # within one 0.05 m cell per axis and two angular steps of the truth, after the search and after the local match
    assert out["err_reloc_m"] <= 0.05 and out["yaw_err_reloc"] <= 2 * out["angular_step"]
    assert out["err_refined_m"] <= 0.05 and out["yaw_err_refined"] <= 2 * out["angular_step"]
    assert out["score"] >= 0.4                                         # the example's min_score


def test_example_on_the_host_twins(binary):
    out = _run(binary, "host")
    assert out["mode"] == "host" and out["solved"] == 0
    _check(out)


@pytest.mark.gpu
def test_example_on_the_device_equals_the_twins_and_solves(binary):
    host = _run(binary, "host")
    out = _run(binary)
    assert out["mode"] == "device"
    _check(out)
    for k in ("num_scans", "num_linear", "depth_used", "angular_step", "score", "err_reloc_m", "yaw_err_reloc", "err_refined_m", "yaw_err_refined"):
        assert out[k] == host[k], k                                    # the same winners and the same score bits
    assert out["solved"] == 1 and out["solve_err_m"] < 0.3            # (the bound of the laser example's window solves)
