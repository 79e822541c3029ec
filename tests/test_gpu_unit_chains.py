"""GPU: the windowed loads of the lone-window Schur finalisation, and the gather in front of it.

k_schur_finalize_head sums a block's gather partials, its pose-major partials and its odometry entries from WINDOWS of loads (FIN_W = 8
partials, FIN_WO = 4 odometry entries in flight before the first add; the first window of the gather partials and of the odometry codes
leaves in front of the gate).  What can go wrong: a window edge (a load or an add too many or too few at W - 1, W, W + 1, 2 W + 1
chunks), an add out of order, an operand of the wrong linearisation set after a rejected trial, a load in a gated-off launch, a value
that survives an upload.  The pass-edge cases were written for a prefetch of the gather's operands one pass ahead (lanes with and
without a pair in the prefetched pass); that prefetch measured no faster and is not in the code, the cases stay as tests of the
k_schur_partial_head kernels at 1 to 4 passes a chunk.

Every case solves its window alone on a latency-tuned handle (the fused speculative unit with k_pcg1: the four head kernels), compares
with the oracle (check_optimize) and, bit for bit — stats tuple and every output — with the same graph as a batch of one: the batched
(Many) kernels keep their code.  Each case asserts from the host plan (tests/upload_plan_oracle.py, the statement tests/test_upload_plan.py
holds the C++ plan to) that the window contains what it is there for.

On the parent commit the lone-window / batch-of-one identity holds for every case of this file (run with the parent's library on the
same box before the change), so a difference here comes from this change."""
import os

import numpy as np
import pytest

import oracle_lib
import upload_plan_oracle
from helpers import graph_of
from test_gpu_parity import _stats_tuple, check_optimize, check_stages
from visfs_amd import abi, graphio, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(iterations=20, solver=2)
FIN_W = 8                                    # ba_kernels.hip: partials per window of the finalisation
FULL = 1 << 30


def _thin(gb, ranges, drop_odo_of=(), dup_odo=None):
    """The graph with every free pose's observations cut down to the landmarks [lo, hi) of `ranges` (one pair per free pose, in pose
    order; a fixed pose keeps everything), without the odometry edges that touch the free poses listed in drop_odo_of and, dup_odo =
    (k, n), with n more copies of the odometry edge between free poses k and k + 1 (measured n + 1 times)."""
    free = [p for p in range(gb.n_poses) if not gb.pose_fixed[p]]
    lo = np.zeros(gb.n_poses, np.int64); hi = np.full(gb.n_poses, FULL, np.int64)
    for p, (a, b) in zip(free, ranges):
        lo[p], hi[p] = a, b
    keep = (gb.obs_point >= lo[gb.obs_pose]) & (gb.obs_point < hi[gb.obs_pose])
    gone = [free[k] for k in drop_odo_of]
    ok = ~(np.isin(gb.odo_from, gone) | np.isin(gb.odo_to, gone))
    s = gb.struct
    idx = np.flatnonzero(ok)
    if dup_odo is not None:
        k, n = dup_odo
        e = [i for i in idx if {int(gb.odo_from[i]), int(gb.odo_to[i])} == {free[k], free[k + 1]}]
        assert len(e) == 1
        idx = np.concatenate([idx, np.full(n, e[0], idx.dtype)])
    return abi.GraphBuffers(gb.pose_tq, gb.pose_fixed, gb.point_xyz, gb.point_fixed, gb.obs_point[keep], gb.obs_pose[keep], gb.obs_uvr[keep],
                            gb.odo_from[idx], gb.odo_to[idx], gb.odo_tq[idx], s.fx, s.fy, s.cx, s.cy, s.bf, Tcr=[s.Tcr[i] for i in range(12)])


def _plan(gb, passes=0):
    """The host plan of the graph as upload_plan_oracle states it: per stored block its pair count, its gather chunks, its odometry
    entries and (diagonal blocks) its pose-major chunks."""
    g = dict(pose_fixed=[int(x) for x in gb.pose_fixed], point_fixed=[int(x) for x in gb.point_fixed], obs_point=[int(x) for x in gb.obs_point],
             obs_pose=[int(x) for x in gb.obs_pose], odo_from=[int(x) for x in gb.odo_from], odo_to=[int(x) for x in gb.odo_to], n_laser=0, laser_pose=0)
    p = upload_plan_oracle.plan(g, dict(solver=2, sch_passes=passes))
    assert p["status"] == 0 and p["run_n"] == 0
    bd = np.asarray(p["blk_desc"]).reshape(-1, 8)
    diag = bd[:, 4] == bd[:, 5]
    return dict(pairs=set(np.diff(p["blk_ptr"]).tolist()), gather=set((bd[:, 1] - bd[:, 0]).tolist()), pose_major=set((bd[diag, 7] - bd[diag, 6]).tolist()),
                odo_diag=set((bd[diag, 3] - bd[diag, 2]).tolist()), odo_off=set((bd[~diag, 3] - bd[~diag, 2]).tolist()),
                odo_only=bool(np.any(~diag & (bd[:, 1] == bd[:, 0]) & (bd[:, 3] > bd[:, 2]))), sch_chunk=p["sch_chunk"], n_sch=p["n_sch"],
                bare_pose=bool(np.any(diag & (bd[:, 1] == bd[:, 0]) & (bd[:, 3] == bd[:, 2]) & (bd[:, 7] == bd[:, 6]))))


def _is_head_unit(s):
    info = s.describe()
    assert info["unit_form"] == 2 and info["solver_kernel"] == 1, (info["unit_form"], info["solver_kernel"])     # fused speculative unit, k_pcg1


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _lone_first_solve(prm, gb):
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


def _oracle_and_batch_of_one(olib, prm, gb, n_sch=None):
    """n_sch: the number of gather chunks the handle must report (describe): the plan the case asserted from is the plan that was uploaded."""
    from visfs_amd import backend
    o = oracle_lib.OracleSystem(olib, prm, gb)
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gb); _is_head_unit(s)
    if n_sch is not None:
        assert s.describe()["n_schur_chunks"] == n_sch, (s.describe()["n_schur_chunks"], n_sch)
    st = check_optimize(o, s)
    out = s.download()
    s.close(); o.close()
    st_b, out_b = _batch_of_one(prm, gb)
    assert _stats_tuple(st) == st_b
    assert _same(out, out_b)


@pytest.fixture(scope="module")
def graphs(olib):
    """EDGES: 12 key-frames that all see 2304 landmarks, thinned so that the free poses keep 64, 448, 512, 576, 1088, 2048, 2049 and (four of
    them) all 2304 landmarks: at one pass a block of poses a, b has ceil(min(n_a, n_b) / 64) gather chunks — 1, 7, 8, 9, 17, 32, 33, 36 — and
    pose a has ceil(n_a / 256) pose-major chunks — 1, 2, 3, 5, 8, 9.
    ODO: 12 key-frames, 150 landmarks, odometry; poses 3 and 4 share no landmark (their block holds the odometry edge only), free pose 7 has
    no observation and no odometry edge (pinned).
    ODO5: ODO with the odometry edge between free poses 5 and 6 five times over: their block has 5 odometry entries, pose 5 has 6 and
    pose 6 has 5 — more than one window of FIN_WO = 4, on a diagonal and on an off-diagonal block.
    PAIRS: 12 key-frames, 300 landmarks; free pose 0 keeps [0, 63), pose 1 [62, 127) — one landmark in common — and poses 2..7 the first 64,
    127, 128, 129, 193, 257: block pair counts 1, 63, 64, 65, 127, 128, 129, 193, 257."""
    prm = abi.default_params(**KW)
    full = lambda n, **k: graph_of(olib.oracle_pack_window, prm, synth.make_window("C2", seed=31, n_kf=12, n_lm=n, n_obs=12 * n, fixed_frac=0.0, **k))[1]
    edges = _thin(full(2304), [(0, n) for n in (64, 448, 512, 576, 1088, 2048, 2049)])
    odo = _thin(full(150, odo=True), [(0, FULL)] * 3 + [(0, 70), (70, FULL)] + [(0, FULL)] * 2 + [(0, 0)], drop_odo_of=(7,))
    odo5 = _thin(full(150, odo=True), [(0, FULL)] * 3 + [(0, 70), (70, FULL)] + [(0, FULL)] * 2 + [(0, 0)], drop_odo_of=(7,), dup_odo=(5, 4))
    pairs = _thin(full(300), [(0, 63), (62, 127)] + [(0, n) for n in (64, 127, 128, 129, 193, 257)])
    return prm, dict(EDGES=edges, ODO=odo, ODO5=odo5, PAIRS=pairs)


@pytest.mark.parametrize("passes", [1, 2])
def test_window_edges_of_the_finalisation(olib, graphs, monkeypatch, passes):
    """Blocks with 1, W - 1, W, W + 1, 2 W + 1 and 4 W + 1 gather chunks, poses with 1, W and W + 1 pose-major chunks (one pass a chunk:
    k_schur_partial_head<false>); the same window at two passes a chunk (1, 9, 16, 17 and 18 gather chunks among them)."""
    prm, gbs = graphs
    monkeypatch.setenv("VISFS_BA_SCH_PASSES", str(passes))
    p = _plan(gbs["EDGES"], passes)
    assert p["sch_chunk"] == 64 * passes
    if passes == 1:
        assert {1, FIN_W - 1, FIN_W, FIN_W + 1, 2 * FIN_W + 1, 4 * FIN_W + 1} <= p["gather"], p["gather"]
    else:
        assert {1, FIN_W + 1, 2 * FIN_W, 2 * FIN_W + 1, 2 * FIN_W + 2} <= p["gather"], p["gather"]
    assert {1, FIN_W, FIN_W + 1} <= p["pose_major"], p["pose_major"]
    other = _plan(gbs["EDGES"], 3 - passes)["n_sch"]
    assert p["n_sch"] != other                          # (so the chunk count the handle reports tells the pass count it planned with)
    _oracle_and_batch_of_one(olib, prm, gbs["EDGES"], n_sch=p["n_sch"])


@pytest.mark.parametrize("case", ["ODO", "ODO5"])
def test_a_window_with_odometry(olib, graphs, case):
    """Diagonal blocks with one and two odometry entries, off-diagonal blocks with one and with none, a block that holds an odometry
    edge and no gather chunk, a free pose without any edge (the pinned path); ODO5: blocks with 5 and 6 entries, diagonal and
    off-diagonal — the loop over further windows of odometry codes and operands."""
    prm, gbs = graphs
    p = _plan(gbs[case])
    assert {1, 2} <= p["odo_diag"] and {0, 1} <= p["odo_off"] and p["odo_only"] and p["bare_pose"], p
    if case == "ODO5":
        assert {5, 6} <= p["odo_diag"] and 5 in p["odo_off"], p
    _oracle_and_batch_of_one(olib, prm, gbs[case], n_sch=p["n_sch"])


@pytest.mark.parametrize("passes", [1, 2, 3, 4])
def test_pass_edges_of_the_gather(olib, graphs, monkeypatch, passes):
    """Block pair counts 1, 63, 64, 65, 127, 128, 129, 193 and 257 (64 passes + 1 for every pass count run here) at 1, 2, 3 and 4 passes a
    chunk: lanes with and without a pair in the pass that is fetched ahead, chunks that end inside, at and one behind a pass."""
    prm, gbs = graphs
    monkeypatch.setenv("VISFS_BA_SCH_PASSES", str(passes))
    p = _plan(gbs["PAIRS"], passes)
    assert p["sch_chunk"] == 64 * passes
    assert {1, 63, 64, 65, 127, 128, 129, 193, 257} <= p["pairs"], p["pairs"]
    assert all(_plan(gbs["PAIRS"], q)["n_sch"] != p["n_sch"] for q in (1, 2, 3, 4) if q != passes)     # the chunk count tells the pass count
    _oracle_and_batch_of_one(olib, prm, gbs["PAIRS"], n_sch=p["n_sch"])


def test_rejected_trials_and_the_replayed_launch_sequence(olib):
    """tests/golden/graphs/hard_rejected_steps.vbag rejects trials: units are gated off (their front loads must be harmless) and the
    linearisation set changes hands.  Lone solve == batch of one; the second and third optimise equal the first, the third is a replay."""
    from visfs_amd import backend
    prm0, gb = graphio.load_graph(os.path.join(HERE, "golden", "graphs", "hard_rejected_steps.vbag"))
    prm = abi.default_params(**KW)
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
    assert s.describe()["graph_replayed"] == 1
    s.close()


def test_no_window_survives_an_upload(olib, graphs):
    """One handle: A twice, B (other chunk counts per block, odometry) twice, A again — every result is a fresh handle's first solve."""
    from visfs_amd import backend
    prm, gbs = graphs
    fresh = {c: _lone_first_solve(prm, gbs[c]) for c in ("PAIRS", "ODO")}
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    for case, n in (("PAIRS", 2), ("ODO", 2), ("PAIRS", 1)):
        s.upload(gbs[case]); _is_head_unit(s)
        for k in range(n):
            if k:
                s.reset()
            rc, st = s.optimize()
            assert rc == abi.OK and _stats_tuple(st) == fresh[case][0] and _same(s.download(), fresh[case][1]), (case, k)
    s.close()


@pytest.mark.parametrize("case", ["EDGES", "ODO"])
def test_stage_hooks_on_the_windowed_kernels(olib, graphs, case):
    """visfs_ba_stage_* reach the head kernels from another call site (check_stages: every stage buffer against the oracle)."""
    from visfs_amd import backend
    prm, gbs = graphs
    o = oracle_lib.OracleSystem(olib, prm, gbs[case])
    s = backend.Solver(prm, tuning=abi.TUNE_LATENCY)
    s.upload(gbs[case]); _is_head_unit(s)
    check_stages(o, s, lambdas=(None, 1e-2, 10.0))
    s.close(); o.close()
