"""The optional `refine` argument of examples/relocalise_step.cpp and examples/loop_closure_step.cpp: the sub-cell refinement of
include/visfs_scan_refine.h after the relocalisation's local match (on the live sub-map) and inside the loop closure's group call
(visfs_scan_group_match_refine).  Without the argument the examples print what they printed before."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ("subcell", "subcell_iterations", "cost_before", "cost_after", "err_subcell_m", "yaw_err_subcell")


def _build(src, exe):
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), src, "-L" + libdir, "-lvisfs_ba_hip",
                    "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def binaries(tmp_path_factory, hiplib):
    d = tmp_path_factory.mktemp("refine_steps")
    return {name: _build(os.path.join(ROOT, "examples", name + ".cpp"), str(d / name)) for name in ("relocalise_step", "loop_closure_step")}


def _run(binary, *args):
    res = subprocess.run([binary, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


def _common(plain, fine):
    """The refinement adds fields and changes none."""
    assert not set(EXTRA) & set(plain)
    assert {k: v for k, v in fine.items() if k in plain} == plain and set(EXTRA) <= set(fine)
    assert fine["cost_after"] <= fine["cost_before"] and 1 <= fine["subcell_iterations"] <= 20


def test_relocalise_step_with_refine_on_the_host_twins(binaries):
    plain, fine = _run(binaries["relocalise_step"], "host"), _run(binaries["relocalise_step"], "host", "refine")
    _common(plain, fine)
    assert fine["subcell"] == 1
    # held to the settled pose's translation with weight 10 and to its yaw with weight 40: it moves by less than a cell
    assert fine["err_subcell_m"] <= 0.05 and fine["yaw_err_subcell"] <= fine["yaw_err_refined"] + 1e-3


def test_loop_closure_step_with_refine_on_the_host_twins(binaries):
    plain, fine = _run(binaries["loop_closure_step"], "host"), _run(binaries["loop_closure_step"], "host", "refine")
    _common(plain, fine)
    assert fine["subcell"] == [1, 1, 1] and fine["information_trace"] > 0.0
    assert fine["err_subcell_m"] <= 0.05 and fine["yaw_err_subcell"] <= 2 * fine["angular_step"]


@pytest.mark.gpu
def test_examples_with_refine_on_the_device_equal_the_twins(binaries):
    for name in ("relocalise_step", "loop_closure_step"):
        host, out = _run(binaries[name], "host", "refine"), _run(binaries[name], "refine")
        assert out["mode"] == "device"
        for k in EXTRA:
            assert out[k] == host[k], (name, k)                         # the same bits through %.17g
    assert (out["launches"], out["copies"], out["waits"]) == (6 + 5 + 1, 2, 1)       # the group call: one launch more
