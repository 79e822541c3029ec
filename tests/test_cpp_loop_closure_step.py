"""examples/loop_closure_step.cpp: three finished sub-maps frozen as they go, a later scan matched against all three in one group
call (VISFS::ScanStackGroup over include/visfs_scan_group.h) from a guess off by (1.1 m, -0.7 m, 0.35 rad), the best member's
pose settled by the weighted local match; `host` runs the one-core twins."""
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
    d = tmp_path_factory.mktemp("loop_closure_step")
    return _build(os.path.join(ROOT, "examples", "loop_closure_step.cpp"), str(d / "loop_closure_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert out["inserted"] == 12 and out["frozen"] == 3 and len(out["scores"]) == 3
    assert all(nx < 200 for nx in out["cells_x"])                      # finished sub-maps: cropped grids
    assert out["matched"] == [1, 1, 1] and all(s >= 0.4 for s in out["scores"])          # the example's min_score
    assert out["best_member"] == max(range(3), key=lambda i: (out["scores"][i], -i))     # one n for all: the score is monotone in the sum
    assert (out["num_linear"], out["depth_used"]) == (30, 7)           # 1.5 m at 0.05 m: L = 61, H = 6
    assert out["err_before_m"] > 1.0
    # within one 0.05 m cell per axis and two angular steps of the truth, after the group search and after the local match
    assert out["err_closure_m"] <= 0.05 and out["yaw_err_closure"] <= 2 * out["angular_step"]
    assert out["refined"] == 1 and out["err_refined_m"] <= 0.05 and out["yaw_err_refined"] <= 2 * out["angular_step"]


def test_example_on_the_host_twins(binary):
    out = _run(binary, "host")
    assert out["mode"] == "host" and (out["launches"], out["copies"], out["waits"]) == (0, 0, 0)
    _check(out)


@pytest.mark.gpu
def test_example_on_the_device_equals_the_twins(binary):
    host = _run(binary, "host")
    out = _run(binary)
    assert out["mode"] == "device"
    _check(out)
    for k in ("cells_x", "scores", "matched", "best_member", "num_linear", "depth_used", "angular_step", "err_closure_m", "yaw_err_closure",
              "err_refined_m", "yaw_err_refined"):
        assert out[k] == host[k], k                                    # the same winners and the same score bits
    assert (out["launches"], out["copies"], out["waits"]) == (6 + 5, 2, 1)     # H + 5 launches for the three members together
