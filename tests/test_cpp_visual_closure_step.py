"""examples/visual_closure_step.cpp: a visual loop closure in plain C++ (VISFS::PlaceRecognizer::queryVerify and closureEdge over
include/visfs_place_verify.h behind the tracker's own corners, flow and stereo, then include/visfs_pose_graph.h on an odometry chain
with drift), on the one-core twins and on the device."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOMS, REVISITED = 4, 0


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    exe = str(tmp_path_factory.mktemp("visual_closure_step") / "visual_closure_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "visual_closure_step.cpp"), "-L" + libdir,
                    "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def host_run(example):
    res = subprocess.run([example, str(ROOMS), str(REVISITED), "host"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_the_closure_pulls_the_drifted_chain_back(host_run):
    """Four rooms on an arc, every odometry edge 0.08 m too long, so the revisit's vertex starts 0.31 m off; the revisit sees room 0
    again from 0.161 m to the right.  The bound on the error after optimisation is a sum stated here, from the gates and not from a run.
    (a) The closure pose: an inlier's reprojection error is at most 2 px (Estimator/PnPReprojError), so, as in
    tests/test_cpp_place_step.py, a sideways error of e moves every point by e * 435.2 / 5 px: e <= 0.023 m; an error of e along the
    optical axis moves a point 150 px from the centre by 150 e / 5 px: e <= 0.067 m; together below 0.1 m.  (b) The chain's share: the
    revisit's vertex is measured twice, by the closure from the fixed vertex 0 with information lc (the smallest of the closure's two
    translational entries) and by the chain of 4 edges of information lo each, which together weigh at most lo / 4 (the yaw
    uncertainty of the chain only lowers that), so at most (lo / 4) / (lc + lo / 4) of the chain's error before is left.
    Bound: 0.1 + share * err_before.  The twins give 0.308 m before and 1.8e-5 m after, z within 1.7e-5 m of (0, -0.1608, 0),
    197 guided rows, all inliers."""
    out = host_run
    print(out)
    assert out["mode"] == "host" and out["rooms"] == out["keyframes"] == ROOMS and min(out["words"]) >= 150 and out["query_points"] >= 150
    assert out["best"] == 0 and out["recognised_slot"] == REVISITED and out["key"] == 1000 * REVISITED + 1
    assert out["guided"] == 1 and out["inliers"] >= 12 and out["rows"] >= out["inliers"]
    assert out["vertices"] == ROOMS + 1 and out["edges"] == ROOMS + 1
    lc, lo = min(out["information"][0], out["information"][4]), out["odometry_information"]
    share = (lo / ROOMS) / (lc + lo / ROOMS)
    assert out["err_before_m"] >= 0.25                                          # the drift is there to be removed
    assert out["err_after_m"] <= 0.1 + share * out["err_before_m"]
    assert out["err_after_m"] < out["err_before_m"]
    dz = [a - b for a, b in zip(out["z"], out["z_true"])]
    assert (dz[0] ** 2 + dz[1] ** 2) ** 0.5 <= 0.1 and abs(dz[2]) <= 0.02      # (a), and the roll bound of the place step for the yaw
    assert abs(out["out_of_plane"][0]) <= 0.1 and max(abs(v) for v in out["out_of_plane"][1:]) <= 0.02


@pytest.mark.gpu
def test_the_device_gives_what_the_twins_give(example, host_run):
    res = subprocess.run([example, str(ROOMS), str(REVISITED)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(out)
    assert out.pop("mode") == "device"
    want = dict(host_run)
    want.pop("mode")
    assert out == want
