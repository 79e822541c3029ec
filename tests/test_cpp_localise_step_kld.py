"""examples/localise_step.cpp with `kld`: the same chain with VISFS::MonteCarloLocalizer::enableKld(100, 0.01, 0.99) on the filter of
2000; the line gains the particle count after every step.  The count starts at 2000, falls below it, the filter keeps the track,
and the device prints the twin's bits.  Without `kld` the line has no such fields (tests/test_cpp_localise_step.py holds it)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binary(tmp_path_factory, hiplib):
    d = tmp_path_factory.mktemp("localise_step_kld")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    exe = str(d / "localise_step")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "localise_step.cpp"), "-L" + libdir,
                    "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def _check(out):
    counts = out["counts"]
    assert out["kld"] == 1 and len(counts) == out["steps"] == 20 and out["particles"] == 2000
    assert counts[0] == 2000                                                   # the first update does not resample
    assert all(100 <= c <= 2000 for c in counts) and min(counts) < 2000        # the count moved, inside min_particles .. N
    assert all(counts[k] == counts[k - 1] for k in range(2, 20, 2))            # ... and only where the filter resampled
    assert out["resampled"] == 10
    assert out["match_error_m"] < out["guess_error_m"]
    assert out["final_error_m"] < 0.1 and out["final_yaw_error_rad"] < 0.05    # as tests/test_cpp_localise_step.py asks of the fixed count
    assert out["last_trace"] < out["first_trace"]


def test_kld_example_on_the_host_twin(binary):
    out = _run(binary, "host", "kld")
    assert out["mode"] == "host" and (out["field_launches"], out["launches"], out["copies"], out["waits"]) == (0, 0, 0, 0)
    _check(out)
    plain = _run(binary, "host")
    assert "kld" not in plain and "counts" not in plain


@pytest.mark.gpu
def test_kld_example_on_the_device_equals_the_twin(binary):
    host = _run(binary, "host", "kld")
    out = _run(binary, "kld")
    assert out["mode"] == "device"
    _check(out)
    for k in host:
        if k not in ("mode", "field_launches", "launches", "copies", "waits"):
            assert out[k] == host[k], k                                        # the same bits, the same counts
    assert (out["field_launches"], out["launches"], out["copies"], out["waits"]) == (2, 4, 2, 1)
