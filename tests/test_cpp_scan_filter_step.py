"""examples/scan_filter_step.cpp: dense scans of a room through VISFS::ScanFilter (five in one call), the filtered range data
inserted into the sub-maps, a sixth scan's match cloud matched with visfs_scan_match, with and without the filter; `host` runs the
one-core twins, which print the same bits."""
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
    d = tmp_path_factory.mktemp("scan_filter_step")
    return _build(os.path.join(ROOT, "examples", "scan_filter_step.cpp"), str(d / "scan_filter_step"))


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    assert out["raw_points"] == 7200 and out["inserted_raw"] == 5 * 7200
    assert 200 <= out["match_points"] <= out["in_range"] <= out["returns"] < out["raw_points"] // 4      # the filter thins the scan
    assert out["misses"] > 0 and out["returns"] + out["misses"] < out["raw_points"]
    assert 0 < out["inserted_returns"] < out["inserted_raw"] // 4
    assert 1 <= out["passes"] <= 12 and 0.0 < out["match_length"] <= 0.5
    for k in ("filtered", "unfiltered"):
        assert out[k]["matched"] == 1 and out[k]["err_m"] < 0.05, k       # from a guess 0.144 m off
    assert abs(out["filtered"]["yaw"] - out["unfiltered"]["yaw"]) < 0.02


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
