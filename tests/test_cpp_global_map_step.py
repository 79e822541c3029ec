"""examples/global_map_step.cpp: a lap on drifting odometry, every finished sub-map added to a VISFS::GlobalMap2D as a tile, the pose
graph optimised with the closures, and the tiles moved with their anchors (visfs_map_pose_from_anchor -> setPoses -> compose): the
cells that one tile knows as occupied and a later one as free must become fewer; `host` runs the one-core twins."""
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
    d = tmp_path_factory.mktemp("global_map_step")
    return _build(os.path.join(ROOT, "examples", "global_map_step.cpp"), str(d / "global_map_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert (out["frames"], out["tiles"], out["closures"]) == (48, 11, 8)
    assert out["cost_after"] < out["cost_before"] and out["end_error_after_m"] < out["end_error_before_m"]
    assert 0 < out["known_before"] <= out["cells_before"] and 0 < out["known_after"] <= out["cells_after"]
    assert out["conflicts_before"] > 0
    assert out["conflicts_after"] < out["conflicts_before"]                 # the corrected map contradicts itself less
    assert out["hash_before"] != out["hash_after"]


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
    assert (out["launches"], out["copies"], out["waits"]) == (1, 1, 1)
