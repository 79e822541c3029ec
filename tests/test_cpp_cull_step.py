"""examples/cull_step.cpp: the outlier cull of a tracked frame in plain C++ (VISFS::rejectOutlierWithFundationMatrix of
visfs_amd/host/EpipolarCull.h over include/visfs_fund.h, then the compaction of Tracker.cpp:285-301)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEIGHT = 752, 480


@pytest.fixture(scope="module")
def example(tmp_path_factory, hiplib):
    from visfs_amd import fund
    fund.load()
    exe = str(tmp_path_factory.mktemp("cull_step") / "cull_step")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "visfs_amd", "host"), os.path.join(ROOT, "examples", "cull_step.cpp"), "-L" + libdir,
                    "-lvisfs_ba_hip", "-Wl,-rpath," + libdir, "-o", exe], check=True, capture_output=True)
    return exe


def test_example_compiles(example):
    assert os.access(example, os.X_OK)


def _host_twin_run(prefix, frames):
    """The example's loop on the host twin: per frame the ids that survive the cull and the compaction."""
    from visfs_amd import fund
    twin = fund.Fund(1024)
    out = []
    for f in range(1, frames + 1):
        rows = np.loadtxt(f"{prefix}_{f}.txt", dtype=np.float64, ndmin=2)
        frm, to = rows[:, 1:3].astype(np.float32), rows[:, 3:5].astype(np.float32)
        res = twin.cull(fund.default_params(pixel_error=1.0), frm, to, rows[:, 5].astype(np.uint8))
        assert res["applied"] == 1
        keep = (res["status"] != 0) & (to[:, 0] >= 0) & (to[:, 0] < WIDTH) & (to[:, 1] >= 0) & (to[:, 1] < HEIGHT)
        out.append([int(i) for i in rows[keep, 0]])
    twin.close()
    return out


@pytest.mark.gpu
def test_example_keeps_the_corners_the_host_twin_keeps(example, tmp_path):
    frames = 4
    prefix = str(tmp_path / "corners")
    res = subprocess.run([example, str(frames), prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print({k: v for k, v in out.items() if k != "kept_ids"})
    assert out["frames"] == frames and len(out["kept_ids"]) == frames
    want = _host_twin_run(prefix, frames)
    for k, ids in enumerate(want):
        assert out["kept_ids"][k] == ids and out["kept"][k] == len(ids)
        assert out["tracked"][k] > 100 and out["mistracks_in"][k] > 20
        # a displacement of 20 .. 60 px in a random direction ends within 1 px of its epipolar line with probability ~ 2 / (40 pi):
        # under 2 % of the mistracks; 10 % is five times that.  Most true corners stay.
        assert out["mistracks_kept"][k] <= 0.1 * out["mistracks_in"][k]
        assert out["kept"][k] - out["mistracks_kept"][k] >= 0.5 * (out["tracked"][k] - out["mistracks_in"][k])
