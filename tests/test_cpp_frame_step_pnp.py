"""examples/frame_step.cpp in its `pnp` mode: the pose guess comes out of the resident tracker call
(VISFS::ResidentTracker::enablePnP / poseGuess over include/visfs_tracker_pnp.h) and no visfs_pnp object is created.  The run passes
the checks of the default mode (test_cpp_frame_step.py), and on the host twins its pose and inlier fields are those of the default
mode: the same rows go through the same arithmetic."""
import json
import os
import subprocess

import pytest

import test_cpp_frame_step as base

example = base.example                           # the module-scoped fixture that compiles the example with -Werror


def _run(exe, *args):
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_pnp_mode_on_the_host_twins(example):
    out = _run(example, "3", "host", "pnp")
    base._check(out, 3)
    staged = _run(example, "3", "host")
    for key in ("frames", "inserted", "words", "covisible", "new_words", "bootstrapped", "identity_guesses", "min_pnp_inliers",
                "max_translation_err_m", "max_depth_err_m", "cull"):
        assert out[key] == staged[key], (key, out[key], staged[key])


@pytest.mark.gpu
def test_pnp_mode_on_the_device(example):
    base._check(_run(example, "5", "pnp"), 5)
