"""examples/localise_step.cpp: sub-maps composed into a global map, a likelihood field and a scan stack made from that map, a
VISFS::MonteCarloLocalizer initialised from a stack match of a wrong pose guess and stepped twenty times on noisy odometry; the
estimate must end nearer the truth than the guess began, and the device must print the twin's bits; `host` runs the one-core twins."""
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
    d = tmp_path_factory.mktemp("localise_step")
    return _build(os.path.join(ROOT, "examples", "localise_step.cpp"), str(d / "localise_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert out["tiles"] >= 2 and out["obstacle_cells"] > 100 and (out["steps"], out["particles"]) == (20, 2000)
    assert out["match_error_m"] < out["guess_error_m"]                       # the stack match corrected the guess
    assert out["final_error_m"] < 0.1 and out["final_yaw_error_rad"] < 0.05  # two cells of the map, and the filter kept the track
    assert out["first_n_eff"] < out["particles"] and out["last_trace"] < out["first_trace"]
    assert out["resampled"] == 10                                            # every second update


def test_example_on_the_host_twin(binary):
    out = _run(binary, "host")
    assert out["mode"] == "host" and (out["field_launches"], out["launches"], out["copies"], out["waits"]) == (0, 0, 0, 0)
    _check(out)


@pytest.mark.gpu
def test_example_on_the_device_equals_the_twin(binary):
    host = _run(binary, "host")
    out = _run(binary)
    assert out["mode"] == "device"
    _check(out)
    for k in host:
        if k not in ("mode", "field_launches", "launches", "copies", "waits"):
            assert out[k] == host[k], k                                      # the same bits
    assert (out["field_launches"], out["launches"], out["copies"], out["waits"]) == (2, 4, 2, 1)
