"""GPU: the phase and step edges of a lone window's solve.

Three launches left a lone window's step: the second k_reset of reset + optimise (skipped while the workspace is provably as a reset
left it), k_phase_end (its work rides on the k_eval launch as one more workgroup, fed through tagged hand-off words) and the copy of
the LM state (the last launch of every sequence writes it into the host's pinned copy).  What can go wrong: a partial that the
on-board phase end adds in another order or misses, a stale hand-off word that matches, a gated-off launch that waits or writes, a
reset skipped although something touched the workspace, a state read that sees an old mirror.

The bit-for-bit yardstick is the same window solved as a batch of one: the batched (Many) launches keep k_phase_end, their own reset
and the copy.  Every case also goes through the oracle (check_optimize).  The windows are the smallest that still take the
multi-launch unit with k_pcg1 (more than 10 free poses)."""
import os

import numpy as np
import pytest

import oracle_lib
from helpers import graph_of
from test_gpu_parity import _stats_tuple, check_optimize
from visfs_amd import abi, graphio, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(iterations=20, solver=2)
# partials of the phase-end fan-in = k_eval's working workgroups = ceil(n_obs / 256) + 1 (the last one: odometry / laser edges)
SHAPES = {"P2": dict(n_kf=12, n_lm=60, n_obs=240),            # two partials
          "P6": dict(n_kf=12, n_lm=150, n_obs=1200),          # six
          # 257: the second slot of a decider thread.  (7 847 Schur chunks: outside the 1 024 .. 6 144 in which a lone window is chunked in two
          # passes and a batch member in one — test_gpu_workloads.py — so lone solve and batch of one still run the same arithmetic)
          "P257": dict(n_kf=20, n_lm=3300, n_obs=65400),
          "K30": dict(n_kf=30, n_lm=300, n_obs=3000)}
PARTS = {"P2": 2, "P6": 6, "P257": 257}


def _window(case):
    return synth.make_window("C2", seed=31, **SHAPES[case])


def _is_multi_launch(s):
    info = s.describe()
    assert info["fused_path"] == 0 and info["unit_form"] == 2 and info["solver_kernel"] == 1, (info["fused_path"], info["unit_form"], info["solver_kernel"])
    return info


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _full(rc, st):
    """Every field the host takes from the LM state: the statistics tuple of the parity tests plus status and the per-phase counts."""
    return (rc, st.status, _stats_tuple(st), list(st.n_active_edges), list(st.pcg_iterations_phase))


def _lone_first_solve(prm, gb):
    from visfs_amd import backend
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_multi_launch(s)
    rc, st = s.optimize()
    out = s.download()
    s.close()
    return _full(rc, st), out


def _batch_of_one(prm, gb):
    from visfs_amd import backend
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.batch_upload([gb])
    rc, sts = s.batch_optimize()
    out = s.batch_download(0)
    s.close()
    return _full(rc, sts[0]), out


@pytest.fixture(scope="module")
def graphs(olib):
    prm = abi.default_params(**KW)
    return prm, {case: graph_of(olib.oracle_pack_window, prm, _window(case))[1] for case in SHAPES}


def _oracle_and_batch(olib, prm, gb):
    """check_optimize against the oracle on a latency-tuned handle, then the same solve bit for bit against the batch of one."""
    from visfs_amd import backend
    o = oracle_lib.OracleSystem(olib, prm, gb)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); info = _is_multi_launch(s)
    st = check_optimize(o, s)
    lone = (_full(st.status, st), s.download())          # (visfs_ba_optimize returns the status it reports)
    after = s.describe()
    s.close(); o.close()
    ref = _batch_of_one(prm, gb)
    assert lone[0] == ref[0]
    assert _same(lone[1], ref[1])
    assert after["state_mirrored"] >= 1             # the solve's state came back without a copy
    return info, st


@pytest.mark.parametrize("case", list(PARTS))
def test_partial_count_edges_of_the_phase_end_fan_in(olib, graphs, case):
    """Two, six and 257 partials (a decider thread's first slot alone, and its second)."""
    prm, gbs = graphs
    info, st = _oracle_and_batch(olib, prm, gbs[case])
    assert (info["n_obs"] + 255) // 256 + 1 == PARTS[case], info["n_obs"]
    if case == "P2":
        assert info["n_obs"] <= 256
    assert info["n_free_poses"] > 10
    assert st.iterations_run[0] > 0 and st.iterations_run[1] > 0


def test_gate_off_phase_ends_and_the_replayed_sequence(olib):
    """tests/golden/graphs/hard_rejected_steps.vbag rejects trials: its phase ends are enqueued before the phase is over (workers publish
    nothing, the decider must not wait) and the host tops up.  Lone solve == batch of one; the second and third optimise equal the first,
    the third as a hipGraph replay."""
    from visfs_amd import backend
    prm0, gb = graphio.load_graph(os.path.join(HERE, "golden", "graphs", "hard_rejected_steps.vbag"))
    prm = abi.default_params(**KW)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_multi_launch(s)
    rc, st = s.optimize()
    assert rc == abi.OK
    assert sum(st.trials_run) > sum(st.iterations_run), "the graph no longer rejects a trial"
    first = (_full(rc, st), s.download())
    assert s.describe()["state_mirrored"] >= 2, "no phase end was enqueued before its phase was over"     # one read per enqueued sequence
    ref = _batch_of_one(prm, gb)
    assert first[0] == ref[0] and _same(first[1], ref[1])
    for k in (2, 3):
        s.reset(); rc, st = s.optimize()
        assert _full(rc, st) == first[0] and _same(s.download(), first[1]), k
    assert s.describe()["graph_replayed"] == 1
    s.close()


@pytest.mark.parametrize("name,kw", [("no_second_phase", dict(iterations=20, solver=2, robust_kernel_delta=0.0)),
                                     ("no_iteration", dict(iterations=0, solver=2)),
                                     ("one_iteration", dict(iterations=2, solver=2)),
                                     ("gauss_newton", dict(iterations=20, solver=2, trust_region=1))])
def test_remaining_phase_end_branches(olib, name, kw):
    """robust_kernel_delta <= 0 (no second phase: next_max_iter = 0), phases of 0 and 1 iterations, Gauss-Newton."""
    prm = abi.default_params(**kw)
    gb = graph_of(olib.oracle_pack_window, prm, _window("P6"))[1]
    info, st = _oracle_and_batch(olib, prm, gb)
    if name == "no_second_phase":
        assert st.iterations_run[1] == 0 and st.n_outliers == 0
    if name == "no_iteration":
        assert list(st.iterations_run) == [0, 0]
    if name == "one_iteration":
        assert list(st.iterations_run) == [1, 1]


def test_reset_is_skipped_only_behind_a_reset(olib, graphs):
    """Upload then optimise == reset then optimise, three times in a row, each without a reset launch of its own; a stage hook or a
    covariance call between reset() and optimize() takes the skip away and the result is still a fresh handle's."""
    from visfs_amd import backend
    prm, gbs = graphs
    gb = gbs["P6"]
    fresh = _lone_first_solve(prm, gb)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb)
    for k in range(3):
        if k:
            s.reset()
        rc, st = s.optimize()
        assert _full(rc, st) == fresh[0] and _same(s.download(), fresh[1]), k
        assert s.describe()["resets_skipped"] == k + 1
    # no reset in front: the estimates are the optimised ones, the solve arms itself
    rc, st = s.optimize()
    assert rc == abi.OK and s.describe()["resets_skipped"] == 3
    for what in ("linearize", "mark_outliers", "begin_phase", "covariance"):
        s.reset()
        if what == "covariance":
            s.covariance(points=False)
        else:
            getattr(s, what)()
        rc, st = s.optimize()
        assert s.describe()["resets_skipped"] == 3, what
        assert _full(rc, st) == fresh[0] and _same(s.download(), fresh[1]), what
    s.close()


def test_uploads_of_two_sizes_on_one_handle(olib, graphs):
    """A / B / A on one handle against fresh handles: no hand-off word, tag, armed reset or mirror of one upload serves the next."""
    from visfs_amd import backend
    prm, gbs = graphs
    fresh = {c: _lone_first_solve(prm, gbs[c]) for c in ("P6", "K30")}
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    for case, n in (("P6", 3), ("K30", 3), ("P6", 1)):
        s.upload(gbs[case]); _is_multi_launch(s)
        for k in range(n):
            if k:
                s.reset()
            rc, st = s.optimize()
            assert _full(rc, st) == fresh[case][0] and _same(s.download(), fresh[case][1]), (case, k)
    s.close()


def test_state_read_through_the_stream_equals_the_read_from_the_mirror(olib, graphs, monkeypatch):
    """The host normally waits for the mirror's count in pinned memory; VISFS_BA_STATE_POLL=0 makes it wait for the stream (the path a solve
    longer than the poll's bound also takes).  Same statistics, same outputs, and the mirror serves the read either way — also on the
    top-up reads of a solve that rejects trials."""
    from visfs_amd import backend
    prm, gbs = graphs
    prm0, hard = graphio.load_graph(os.path.join(HERE, "golden", "graphs", "hard_rejected_steps.vbag"))
    for gb in (gbs["P6"], hard):
        got = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("VISFS_BA_STATE_POLL", mode)
            s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
            s.upload(gb); _is_multi_launch(s)
            res = []
            for k in range(3):
                if k:
                    s.reset()
                rc, st = s.optimize()
                res.append((_full(rc, st), s.download()))
            assert s.describe()["state_mirrored"] >= 3
            s.close()
            assert all(r[0] == res[0][0] and _same(r[1], res[0][1]) for r in res), mode
            got[mode] = res[0]
        assert got["1"][0] == got["0"][0] and _same(got["1"][1], got["0"][1])


def test_no_stale_mirror_after_close(olib, graphs):
    """A handle is closed and a new one solves another window: its statistics are that window's (batch of one), in every field."""
    prm, gbs = graphs
    a = _lone_first_solve(prm, gbs["K30"])
    b = _lone_first_solve(prm, gbs["P2"])
    ref = _batch_of_one(prm, gbs["P2"])
    assert b[0] == ref[0] and _same(b[1], ref[1])
    assert a[0] != b[0]
