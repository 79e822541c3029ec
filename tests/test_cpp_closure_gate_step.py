"""examples/closure_gate_step.cpp: a lap and six tenths of a circle with three closures, optimised by VISFS::PoseGraph2D, then the
search window of one candidate closure from the relative covariance of its two vertices (VISFS::PoseGraph2D::searchWindow over
include/visfs_pose_graph_cov.h); `host` runs the one-core twin."""
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
    d = tmp_path_factory.mktemp("closure_gate_step")
    return _build(os.path.join(ROOT, "examples", "closure_gate_step.cpp"), str(d / "closure_gate_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert (out["vertices"], out["edges"], out["closures"]) == (160, 159 + 3, 3)
    assert (out["anchor"], out["scan"], out["sigmas"]) == (59, 159, 3)
    assert (out["sources"], out["columns"], out["unconverged_columns"]) == (3, 9, 0)
    assert out["cost_after"] < out["cost_before"]
    # the window is far inside the blanket one, wider than that of two neighbours on the chain, and it covers what it has to: the
    # error of the graph's relative pose of the pair
    assert 0.0 < out["linear_window_m"] < 0.1 * out["blanket_linear_m"]
    assert 0.0 < out["angular_window_rad"] < 0.5 * out["blanket_angular_rad"]
    assert out["neighbour_linear_window_m"] < out["linear_window_m"] and out["neighbour_angular_window_rad"] < out["angular_window_rad"]
    assert abs(out["neighbour_linear_window_m"] - 3 * 0.004) < 1e-6 and abs(out["neighbour_angular_window_rad"] - 3 * 0.002) < 1e-6
    assert out["miss_m"] < out["linear_window_m"] and out["miss_rad"] < out["angular_window_rad"]


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
    assert (out["launches"], out["copies"], out["waits"]) == (3, 2, 1)
