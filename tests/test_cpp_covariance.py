"""`VISFS::Optimizer::Optimizer::lastCovariance` (visfs_amd/host/Optimizer.{h,cpp}) through tests/cpp/cov_driver.cpp: the reference's
std::map signature in, covariances keyed by signature / feature id out — the same bytes as visfs_ba_window_covariance on the same
window (backend.Solver.window_covariance), root pose zeros, unused points NaN, refusals as `false`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import ragged_window
from test_cpp_shim import dump_window
from visfs_amd import abi, backend, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cov_driver(tmp_path_factory, hiplib):
    exe = str(tmp_path_factory.mktemp("cov") / "cov_driver")
    libdir = os.path.join(ROOT, "visfs_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "visfs_amd", "host"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cov_driver.cpp"),
           os.path.join(ROOT, "visfs_amd", "host", "Optimizer.cpp"), "-L" + libdir, "-lvisfs_ba_hip",
           "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


def _run(exe, tmp_path, w, args):
    dump_window(tmp_path / "in.bin", w)
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + args, check=True, capture_output=True)
    b = open(tmp_path / "out.bin", "rb").read()
    status, before, ok, n_pose, n_pt = struct.unpack_from("5q", b, 0)
    off = 40
    poses, pts = {}, {}
    for _ in range(n_pose):
        k, = struct.unpack_from("Q", b, off); off += 8
        poses[k] = np.frombuffer(b, np.float64, 36, off).reshape(6, 6).copy(); off += 288
    for _ in range(n_pt):
        k, = struct.unpack_from("Q", b, off); off += 8
        pts[k] = np.frombuffer(b, np.float64, 9, off).reshape(3, 3).copy(); off += 72
    return status, before, ok, poses, pts


@pytest.mark.parametrize("cfg,solver", [("PROD", 2), ("RAGGED", 0)])
def test_last_covariance_equals_the_window_layer(cov_driver, tmp_path, cfg, solver):
    w = synth.make_window("PROD") if cfg == "PROD" else ragged_window(seed=11)
    status, before, ok, poses, pts = _run(cov_driver, tmp_path, w, ["Optimizer/Iterations=10", "Optimizer/Solver=%d" % solver])
    assert status == abi.OK and before == 0 and ok == 1
    s = backend.Solver(abi.default_params(iterations=10, solver=solver))
    wb = abi.WindowBuffers(w)
    rc, _ = s.solve_window(wb)
    assert rc == abi.OK
    pose_wr, pt_cov = s.window_covariance(wb.struct.n_poses, wb.struct.n_points)
    s.close()
    ids = [int(i) for i in w["pose_ids"]]
    assert sorted(poses) == ids
    for i, k in enumerate(ids):
        assert np.array_equal(poses[k], pose_wr[i], equal_nan=True)
    assert not poses[int(w["root_id"])].any()                            # the fixed pose: zeros
    pids = [int(i) for i in w["point_ids"]]
    assert sorted(pts) == pids
    for l, k in enumerate(pids):
        assert np.array_equal(pts[k], pt_cov[l], equal_nan=True)
    if cfg == "RAGGED":
        feats = set(int(f) for f in w["ref_feature"])
        unused = [k for k in pids if k not in feats]
        assert unused and all(np.isnan(pts[k]).all() for k in unused)   # never a vertex: NaN


def test_last_covariance_refusals(cov_driver, tmp_path):
    w = synth.make_window("PROD")
    w["root_id"] = int(max(w["pose_ids"])) + 100                         # no fixed pose: the gauge is free
    status, before, ok, poses, pts = _run(cov_driver, tmp_path, w, ["Optimizer/Iterations=10"])
    assert status == abi.OK and ok == 0 and poses == {} and pts == {}
    w = synth.make_window("PROD")                                        # the Ceres branch
    status, before, ok, poses, pts = _run(cov_driver, tmp_path, w, ["Optimizer/Iterations=10", "Optimizer/Framework=1"])
    assert status == abi.OK and ok == 0 and poses == {}
    status, before, ok, poses, pts = _run(cov_driver, tmp_path, w, ["Optimizer/Iterations=0"])   # passthrough
    assert status == abi.PASSTHROUGH and ok == 0 and poses == {}
