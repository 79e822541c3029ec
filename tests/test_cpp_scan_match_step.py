"""examples/scan_match_step.cpp: a wheel-slip guess corrected by the correlative scan match (VISFS::Map::ActiveSubmaps2D::match
over include/visfs_scan_match.h) and handed to the window solve; `host` runs the one-core twin."""
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
    d = tmp_path_factory.mktemp("scan_match_step")
    return _build(os.path.join(ROOT, "examples", "scan_match_step.cpp"), str(d / "scan_match_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check_match(out):
    assert out["inserted"] == 5 and out["matched"] == 1 and out["num_linear"] == 6
    assert out["err_before_m"] > 0.14                                  # (0.12, -0.08): well beyond a cell or two
    # within one 0.05 m cell per axis and two angular steps of the truth
    assert out["err_after_m"] <= 0.05 and out["yaw_err_after"] <= 2 * out["angular_step"]


def test_example_on_the_host_twin(binary):
    out = _run(binary, "host")
    assert out["mode"] == "host" and out["solved"] == 0
    _check_match(out)


@pytest.mark.gpu
def test_example_on_the_device_equals_the_twin_and_solves(binary):
    host = _run(binary, "host")
    out = _run(binary)
    assert out["mode"] == "device"
    _check_match(out)
    for k in ("num_scans", "num_linear", "angular_step", "score", "err_after_m", "yaw_err_after"):
        assert out[k] == host[k], k                                    # the same winner and the same score bits
    assert out["solved"] == 1 and out["solve_err_m"] < 0.3            # (the bound of the laser example's window solves)
