"""examples/pose_graph_step.cpp: two dead-reckoned laps of a circle, the odometry chain and nine closures made into edges through
visfs_pose_graph_edge_from_refine, optimised by VISFS::PoseGraph2D (visfs_amd/host/PoseGraph2D.h); `host` runs the one-core twin."""
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
    d = tmp_path_factory.mktemp("pose_graph_step")
    return _build(os.path.join(ROOT, "examples", "pose_graph_step.cpp"), str(d / "pose_graph_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert (out["vertices"], out["edges"], out["closures"]) == (200, 199 + 9, 9)
    assert out["calls"] >= 1 and out["termination"] in (0, 1, 2)
    assert out["cost_after"] < 0.01 * out["cost_before"]
    # The dead-reckoned second lap is off by decimetres.  The closures tie it to the first lap, whose own drift nothing measures, so
    # the worst error falls to the first lap's share (less than half here) and not to the measurement noise.
    assert out["err_before_m"] > 0.5
    assert out["err_after_m"] < 0.5 * out["err_before_m"]
    assert out["yaw_err_after"] < 0.5 * out["yaw_err_before"]
    assert out["pcg_iterations"] <= out["trials"] * (6 * out["closures"] + 1 + 4)      # the iteration bound of section 9p, a little rounding allowed


def test_example_on_the_host_twin(binary):
    out = _run(binary, "host")
    assert out["mode"] == "host" and (out["launches"], out["copies"], out["waits"]) == (0, 0, 0)
    _check(out)


@pytest.mark.gpu
def test_example_on_the_device_equals_the_twin(binary):
    host = _run(binary, "host")
    out = _run(binary)
    assert out["mode"] == "device"
    _check(out)
    for k in host:
        if k not in ("mode", "launches", "copies", "waits"):
            assert out[k] == host[k], k                                    # the same bits
    assert (out["launches"], out["copies"], out["waits"]) == (1, 2, 1)
