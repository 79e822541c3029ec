"""examples/pnp_step.cpp: the pose guess of a frame in plain C++ (VISFS::estimateMotion3DTo2D of visfs_amd/host/MotionEstimator.h
over include/visfs_pnp.h, then visfs_window_insert)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import build, pnp
    pnp.load()
    build.build_host()
    exe = str(tmp_path_factory.mktemp("pnp_step") / "pnp_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "pnp_step.cpp"), "-L" + libdir,
                    "-lvisfs_window", "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def test_example_compiles(example):
    assert os.access(example, os.X_OK)


def _words(path):
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    return {int(r[0]): r[1:].astype(np.float32) for r in rows}


def _host_twin_run(prefix, frames):
    """The example's loop on the host twin: per frame from the second (matches, inlier ids, transform)."""
    from visfs_amd import pnp
    twin = pnp.Pnp(1024)
    prm, cam = pnp.default_params(), pnp.camera()
    out, before = [], _words(f"{prefix}_0.txt")
    for k in range(1, frames):
        now = _words(f"{prefix}_{k}.txt")
        ids = [i for i in sorted(now) if i in before]                            # MultiviewGeometry.cpp:113-129
        res = twin.solve(prm, cam, np.array([before[i][4:7] for i in ids]), np.array([now[i][0:2] for i in ids]),
                         np.array([now[i][4:7] for i in ids]))
        out.append((len(res["matches"]), [ids[j] for j in res["inliers"]], res["T"]))
        before = now
    twin.close()
    return out


@pytest.mark.gpu
def test_example_guesses_the_poses_the_host_twin_guesses(example, tmp_path):
    frames = 5
    prefix = str(tmp_path / "words")
    res = subprocess.run([example, str(frames), prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print({k: v for k, v in out.items() if k not in ("inliers", "transforms")})
    assert out["frames"] == out["inserted"] == frames and len(out["transforms"]) == frames - 1
    want = _host_twin_run(prefix, frames)
    for k, (matches, inliers, T) in enumerate(want):
        assert out["matches"][k] == matches and matches > 100
        assert out["inliers"][k] == inliers and len(inliers) >= 12
        assert np.array(out["transforms"][k]).reshape(4, 4).tobytes() == T.tobytes()
    assert out["max_rot_err_rad"] < 0.01 and out["max_trans_err_m"] < 0.05
