"""examples/localise_step.cpp with `hyp`: the `kld` chain with VISFS::MonteCarloLocalizer::enableHypotheses(); for every step that
resampled the line gains the number of clusters and the best hypothesis beside the mean.  The filter itself is the `kld` one (the
same hash and counts), the best hypothesis keeps the track, and the device prints the twin's bits.  The other modes' lines have no
such fields (tests/test_cpp_localise_step.py and tests/test_cpp_localise_step_kld.py hold them)."""
import json
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binary(tmp_path_factory, hiplib):
    d = tmp_path_factory.mktemp("localise_step_hyp")
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
    hyps = out["hypotheses"]
    assert out["hyp"] == 1 and out["kld"] == 1 and out["resampled"] == len(hyps) == 10
    assert [h["step"] for h in hyps] == list(range(1, 20, 2))                 # the steps that resampled
    for h, n in zip(hyps, (out["counts"][h["step"]] for h in hyps)):
        assert h["clusters"] >= 1 and 1 <= h["count"] <= n
        if h["clusters"] == 1:                                                 # one cluster: every particle, and the mean of the set before the draw
            assert h["count"] == n and math.hypot(h["best"][0] - h["mean"][0], h["best"][1] - h["mean"][1]) < 0.05
    assert hyps[0]["clusters"] == 1
    assert out["hyp_final_error_m"] < 0.1                                      # as the mean is held in tests/test_cpp_localise_step.py


def test_hyp_example_on_the_host_twin(binary):
    out = _run(binary, "host", "hyp")
    assert out["mode"] == "host" and (out["field_launches"], out["launches"], out["copies"], out["waits"]) == (0, 0, 0, 0)
    _check(out)
    kld = _run(binary, "host", "kld")
    assert "hyp" not in kld and "hypotheses" not in kld and "hyp_hash" not in kld
    for k in kld:
        assert out[k] == kld[k], k                                             # the hypotheses leave the filter alone


@pytest.mark.gpu
def test_hyp_example_on_the_device_equals_the_twin(binary):
    host = _run(binary, "host", "hyp")
    out = _run(binary, "hyp")
    assert out["mode"] == "device"
    _check(out)
    for k in host:
        if k not in ("mode", "field_launches", "launches", "copies", "waits"):
            assert out[k] == host[k], k                                        # the same bits
    assert (out["field_launches"], out["launches"], out["copies"], out["waits"]) == (2, 4, 2, 1)
