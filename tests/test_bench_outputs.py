"""bench.py's plain run and `--dump-outputs DIR`: the arrays a caller of the timed path receives, written as DIR/<name>.npy in
float32 / float64 so that two builds can be compared output for output on the same seeded inputs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from visfs_amd import abi, backend, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(k):
    return types.SimpleNamespace(status=0, iterations_run=[10, 10], trials_run=[11, 12], pcg_iterations=100 + k, n_outliers=7,
                                 chi2_initial=5.0, chi2_phase1=2.0, chi2_final=1.0, n_active_edges=[300, 290],
                                 pcg_iterations_phase=[60, 40 + k], solver_fallback=0)


def _result(n_poses, n_points, n_obs, k):
    rng = np.random.default_rng(k)
    return (rng.standard_normal((n_poses, 7)), rng.standard_normal((n_points, 3)), (rng.random(n_obs) < 0.1).astype(np.uint8),
            rng.random(n_obs))


def test_dump_writes_every_window_as_float_arrays(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    results = [_result(10, 50, 300, k) for k in range(2)]
    bench.dump_outputs(str(tmp_path), results, [_stats(0), _stats(1)])
    assert sorted(os.listdir(tmp_path)) == sorted(f"window{b}_{n}.npy" for b in range(2)
                                                  for n in ("poses", "points", "outliers", "edge_chi2", "stats"))
    for b, (pose, pt, outl, chi2) in enumerate(results):
        got = {n: np.load(tmp_path / f"window{b}_{n}.npy") for n in ("poses", "points", "outliers", "edge_chi2", "stats")}
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert np.array_equal(got["poses"], pose) and np.array_equal(got["points"], pt) and np.array_equal(got["edge_chi2"], chi2)
        assert np.array_equal(got["outliers"], outl.astype(np.float32))
        assert got["stats"][0] == 0 and list(got["stats"][1:5]) == [10, 10, 11, 12] and got["stats"][5] == 100 + b


def test_dump_above_the_budget_keeps_the_same_seeded_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    results = [_result(40, 2000, 20000, 3)]
    budget = 100000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), results, [_stats(0)], budget=budget)
    names = sorted(os.listdir(tmp_path / "a"))
    assert sum(np.load(tmp_path / "a" / n).nbytes for n in names) <= budget
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))      # the sample is fixed
    chi2 = np.load(tmp_path / "a" / "window0_edge_chi2.npy")
    assert 0 < len(chi2) < 20000 and np.isin(chi2, results[0][3]).all()                       # rows of the output, not a resize
    assert len(np.load(tmp_path / "a" / "window0_stats.npy")) == 15                           # the statistics are never sampled


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_the_last_step_computed(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--config", "C1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "BA iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert not {"roofline", "config5", "cpu_baseline", "per_frame_call", "result_gather"} & set(d)       # those need --full
    # the same window solved once more on a handle of its own
    prm = abi.default_params(iterations=20, solver=2)
    lib = backend.load_library()
    gb, *_ = abi.pack_window_with(lib.visfs_ba_pack_window, prm, abi.WindowBuffers(synth.make_window("C1", window_index=0)))
    s = backend.Solver(prm, device=0, tuning=abi.TUNE_LATENCY)
    s.upload(gb)
    s.reset()
    rc, st = s.optimize()
    pose, pt, outl, chi2 = s.download()
    s.close()
    assert rc == abi.OK
    np.testing.assert_allclose(np.load(out / "window0_poses.npy"), pose, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.load(out / "window0_points.npy"), pt, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.load(out / "window0_edge_chi2.npy"), chi2, rtol=1e-12, atol=1e-12)
    assert np.array_equal(np.load(out / "window0_outliers.npy"), outl.astype(np.float32))
    stats = np.load(out / "window0_stats.npy")
    assert list(stats[1:5]) == [st.iterations_run[0], st.iterations_run[1], st.trials_run[0], st.trials_run[1]]
