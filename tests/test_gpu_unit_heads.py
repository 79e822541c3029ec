"""GPU: the head arguments of the lone-window LM unit.

k_schur_partial, k_schur_finalize, k_pcg1 and k_backsub<LINA> of a window on its own take the pointers and counts of their heads as
leading scalar kernel parameters (preloaded into user SGPRs) in front of the by-value graph.  What can go wrong: a head value that
differs from the graph's, a head value baked into a captured launch sequence that outlives its upload, a front load in a gated-off
launch.  The windows are the smallest that still take the four-launch fused unit with k_pcg1 (more than 10 free poses: below,
k_small_solve takes over), with and without odometry (the ODOSPEC instantiation of k_backsub).

The bit-for-bit yardstick is the same window solved as a batch of one: the batched (Many) kernels are not touched by the head
arguments.  On the parent commit that identity holds for all four windows and for the golden graph (measured with the parent's
library on the same box before the change), so every case keeps both comparisons."""
import os

import numpy as np
import pytest

import oracle_lib
from helpers import graph_of
from test_gpu_parity import _stats_tuple, check_optimize, check_stages
from visfs_amd import abi, graphio, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(iterations=20, solver=2)
SHAPES = {"K12": dict(n_kf=12, n_lm=150, n_obs=1200), "K30": dict(n_kf=30, n_lm=300, n_obs=3000),
          "K12_ODO": dict(n_kf=12, n_lm=150, n_obs=1200, odo=True), "K30_ODO": dict(n_kf=30, n_lm=300, n_obs=3000, odo=True)}


def _window(case):
    return synth.make_window("C2", seed=31, **SHAPES[case])


def _is_head_unit(s):
    info = s.describe()
    assert info["unit_form"] == 2 and info["solver_kernel"] == 1, (info["unit_form"], info["solver_kernel"])     # fused speculative unit, k_pcg1


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _lone_first_solve(prm, gb):
    """(stats tuple, outputs) of a fresh latency-tuned handle's first solve of the graph."""
    from visfs_amd import backend
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_head_unit(s)
    rc, st = s.optimize()
    assert rc == abi.OK
    out = s.download()
    s.close()
    return _stats_tuple(st), out


def _batch_of_one(prm, gb):
    from visfs_amd import backend
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.batch_upload([gb])
    rc, sts = s.batch_optimize()
    assert rc == abi.OK
    out = s.batch_download(0)
    s.close()
    return _stats_tuple(sts[0]), out


@pytest.fixture(scope="module")
def graphs(olib):
    prm = abi.default_params(**KW)
    return prm, {case: graph_of(olib.oracle_pack_window, prm, _window(case))[1] for case in SHAPES}


@pytest.mark.parametrize("case", list(SHAPES))
def test_lone_window_equals_the_oracle_and_its_batch_of_one(olib, graphs, case):
    """Each window alone on a latency-tuned handle: against the oracle (check_optimize: iteration, trial and PCG counts, outlier
    lists, poses to 1e-6) and bit for bit against the batch of one."""
    from visfs_amd import backend
    prm, gbs = graphs
    gb = gbs[case]
    o = oracle_lib.OracleSystem(olib, prm, gb)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_head_unit(s)
    st = check_optimize(o, s)
    out = s.download()
    s.close(); o.close()
    st_b, out_b = _batch_of_one(prm, gb)
    assert _stats_tuple(st) == st_b
    assert _same(out, out_b)


def test_rejected_trials_and_the_replayed_launch_sequence(olib):
    """tests/golden/graphs/hard_rejected_steps.vbag rejects trials, so units are gated off: a gated-off launch must read nothing it
    may not and write nothing.  Lone solve == batch of one; the third optimise on the handle is a hipGraph replay and equals the first."""
    from visfs_amd import backend
    prm0, gb = graphio.load_graph(os.path.join(HERE, "golden", "graphs", "hard_rejected_steps.vbag"))
    prm = abi.default_params(**KW)                      # (the dump names the solver of the cross-check; the unit under test is the PCG one)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_head_unit(s)
    rc, st = s.optimize()
    assert rc == abi.OK
    assert sum(st.trials_run) > sum(st.iterations_run), "the graph no longer rejects a trial"
    first = (_stats_tuple(st), s.download())
    st_b, out_b = _batch_of_one(prm, gb)
    assert first[0] == st_b and _same(first[1], out_b)
    for k in (2, 3):
        s.reset(); rc, st = s.optimize()
        assert rc == abi.OK and _stats_tuple(st) == first[0] and _same(s.download(), first[1]), k
    assert s.describe()["graph_replayed"] == 1          # the third call replayed the captured sequence
    s.close()


def test_no_head_value_survives_an_upload(olib, graphs):
    """One handle: A three times (the third a replay), B of another size three times, A again — every result is a fresh handle's
    first solve of that window, so nothing captured with A's heads serves B and nothing of B's serves A."""
    from visfs_amd import backend
    prm, gbs = graphs
    fresh = {c: _lone_first_solve(prm, gbs[c]) for c in ("K12_ODO", "K30")}
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    for case, n in (("K12_ODO", 3), ("K30", 3), ("K12_ODO", 1)):
        s.upload(gbs[case]); _is_head_unit(s)
        for k in range(n):
            if k:
                s.reset()
            rc, st = s.optimize()
            assert rc == abi.OK and _stats_tuple(st) == fresh[case][0] and _same(s.download(), fresh[case][1]), (case, k)
    s.close()


def test_stage_hooks_launch_the_same_heads(olib, graphs):
    """visfs_ba_stage_* reach the head kernels from another call site (check_stages: every stage buffer against the oracle)."""
    from visfs_amd import backend
    prm, gbs = graphs
    gb = gbs["K12_ODO"]
    o = oracle_lib.OracleSystem(olib, prm, gb)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_head_unit(s)
    check_stages(o, s, lambdas=(None, 1e-2, 10.0))
    s.close(); o.close()
