"""examples/place_step.cpp: a revisited room in plain C++ (VISFS::PlaceRecognizer over include/visfs_place.h behind the tracker's own
corners, flow and stereo, then include/visfs_pnp.h on the rows of the top candidate), on the one-core twins and on the device."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOMS, REVISITED = 3, 1


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    exe = str(tmp_path_factory.mktemp("place_step") / "place_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "place_step.cpp"), "-L" + libdir,
                    "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def host_run(example):
    res = subprocess.run([example, str(ROOMS), str(REVISITED), "host"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_the_twins_recognise_the_room_and_find_the_pose(host_run):
    """The revisit is rolled by 0.6 rad and shifted by (14, -9) px, 0.19 m at the wall's 5 m.  Tolerances, from the PnP gate and not
    from a run: an inlier's reprojection error is at most 2 px, so a pose error cannot move the image points by more than that.  A
    roll error of a moves a point 150 px from the centre by 150 a px: a <= 0.0133 rad, asserted as 0.02.  A sideways error of e moves
    every point by e * 435.2 / 5 px: e <= 0.023 m; an error of e along the optical axis moves a point 150 px from the centre by
    150 e / 5 px: e <= 0.067 m; together below 0.1 m.  The twins give 0.00096 rad and 0.0050 m, 84 matches against at most 23 in the
    other rooms, 83 of them inliers."""
    out = host_run
    print(out)
    assert out["mode"] == "host" and out["rooms"] == out["keyframes"] == ROOMS and len(out["words"]) == ROOMS
    assert min(out["words"]) >= 150 and out["query_points"] >= 150
    assert out["recognised_slot"] == REVISITED and out["key"] == 1000 * REVISITED + 1
    others = [c for k, c in enumerate(out["counts"]) if k != REVISITED]
    assert out["counts"][REVISITED] == out["matches"] >= 3 * max(others)
    assert out["inliers"] >= 12                                                # Estimator/MinInliers: a pose was found
    assert out["rot_err_rad"] <= 0.02 and out["trans_err_m"] <= 0.1


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
