"""The host plan of a graph upload (visfs_amd/csrc/ba_plan.hpp: summary of the observations, index structure of S, kernel forms) without
a GPU: tests/cpp/plan_driver.cpp, compiled with plain g++, against the independent statement in tests/upload_plan_oracle.py — every
array and scalar integer-equal, over small graphs that hit the places this code can go wrong."""
import os
import re
import subprocess

import numpy as np
import pytest

import upload_plan_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visfs_amd", "csrc")
ERR_UNSUPPORTED = 7


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "plan_driver.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def graph(fixed, tracks, point_fixed=(), odo=(), n_laser=0, laser_pose=0):
    """fixed: one flag per pose; tracks: per landmark the poses that see it; odo: (from, to) pairs."""
    obs = [(l, p) for l, t in enumerate(tracks) for p in sorted(t)]
    pf = np.zeros(len(tracks), int); pf[list(point_fixed)] = 1
    return dict(pose_fixed=list(fixed), point_fixed=list(pf), obs_point=[l for l, _ in obs], obs_pose=[p for _, p in obs],
                odo_from=[a for a, _ in odo], odo_to=[b for _, b in odo], n_laser=n_laser, laser_pose=laser_pose)


def run_driver(exe, g, d):
    lines = [f"{k} {len(v)} " + " ".join(str(int(x)) for x in v) for k, v in g.items() if isinstance(v, list)]
    lines += [f"{k} 1 {int(v)}" for k, v in list(g.items()) + list(d.items()) if not isinstance(v, list)]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = {}
    for ln in r.stdout.splitlines():
        name, rest = ln.split(" ", 1)
        if name == "msg": out["msg"] = rest; continue
        n, *vals = rest.split()
        out[name] = int(vals[0]) if n == "1" and not name_is_array(name) else [int(v) for v in vals]
    return out


SCALARS = set("pairs_seen n_edges_ok status sizeof_sch_desc sizeof_blk_desc sizeof_blk_slot run_LR run_M run_n run_cap run_wmax run_lds run_total Npf n_pose_obs n_chunks "
              "n_blk n_sch npairs sch_chunk max_row pcg_rpw pcg_lds lds_srow cu_T cu_max_row pcg1 pcg_cu small_fits band_B band_rows band_lds group n_lin_a n_parts "
              "chol_np n_hist".split())


def name_is_array(name):
    return name not in SCALARS


def check(exe, g, d, s=None):
    """Driver against checker, every entry of the checker's answer; returns the driver's."""
    got = run_driver(exe, g, d)
    if s is None:
        s = oracle.summary(g)
        f = oracle.summary_fast(g)
        assert all(np.array_equal(np.asarray(s[k]), np.asarray(f[k])) for k in s), "the two statements of the summary disagree"
    want = oracle.plan(g, d, s)
    assert got["status"] == want["status"], got.get("msg")
    for k, v in want.items():
        if isinstance(v, (list, np.ndarray)):
            assert got[k] == [int(x) for x in v], k
        else:
            assert got[k] == v, k
    return got


def window(n_poses, n_fixed, n_lm, span=3, seed=0):
    """A sliding window: landmark ids grow with time, every track a run of `span` consecutive poses; the first n_fixed poses fixed."""
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.integers(0, n_poses - span + 1, n_lm))
    return [1] * n_fixed + [0] * (n_poses - n_fixed), [list(range(s, s + span)) for s in starts]


PCG = dict(solver=2)


def test_all_poses_fixed_every_array_at_its_minimum(driver):
    fixed, tracks = window(4, 4, 10)
    got = check(driver, graph(fixed, tracks), PCG)
    assert got["Npf"] == 0 and got["n_blk"] == 0 and got["n_chunks"] == 0 and got["chunk_ptr"] == [0] and got["blk_ptr"] == [0] and got["row_ptr"] == [0]
    assert (got["sizeof_sch_desc"], got["sizeof_blk_desc"], got["sizeof_blk_slot"]) == (1, 2, 1) and got["band_B"] == -1 and got["pcg1"] == 0


def test_one_free_pose_among_fixed_ones(driver):
    got = check(driver, graph([1, 1, 0, 1, 1], window(5, 0, 30)[1]), PCG)
    assert got["Npf"] == 1 and got["blk_i"] == [0] and got["blk_j"] == [0] and got["pcg1_code"] == [0] and got["small_fits"] == 1


@pytest.mark.parametrize("kind", ["runs", "gap", "both"])
def test_tracks_that_are_runs_and_tracks_with_gaps(driver, kind):
    runs = window(6, 1, 24)[1]
    gaps = [[0, 2, 5], [1, 3], [1, 2, 4, 5], [2, 5]]
    tracks = {"runs": runs, "gap": gaps[:1], "both": runs[:12] + gaps + runs[12:]}[kind]
    got = check(driver, graph([1, 0, 0, 0, 0, 0], tracks), PCG)
    if kind == "gap":
        assert got["blk_i"] == [0, 1, 1, 2, 3, 4] and got["blk_j"] == [0, 1, 4, 2, 3, 4] and got["pairs_seen"] == 3 and got["npairs"] == 3


def test_fixed_landmarks_and_landmarks_of_fixed_poses_only(driver):
    fixed, tracks = window(6, 2, 20)
    tracks += [[0, 1], [2, 3, 4]]                     # seen only by the two fixed poses; a fixed landmark seen by free ones
    got = check(driver, graph(fixed, tracks, point_fixed=[3, 21]), PCG)
    assert got["n_edges_ok"] == sum(1 for l, t in enumerate(tracks) for p in t if not (fixed[p] and l in (3, 21))) < sum(len(t) for t in tracks)


def test_odometry_edges_transposed_fixed_and_block_only(driver):
    fixed = [1, 0, 0, 0, 0, 0]
    tracks = [[0, 1, 2], [1, 2], [2, 3], [3, 4], [4, 5], [1, 2, 3]]
    odo = [(3, 1), (0, 2), (1, 5), (2, 1), (4, 3)]    # from > to; fixed - free; two free poses without a common landmark; ...
    got = check(driver, graph(fixed, tracks, odo=odo), dict(solver=0))
    b = got["blk_of"][0 * 5 + 4]                      # block (pose 1, pose 5): exists through the edge alone
    assert b >= 0 and got["blk_ptr"][b + 1] == got["blk_ptr"][b] and got["blk_odo"][got["blk_odo_ptr"][b]:got["blk_odo_ptr"][b + 1]] == [4]
    assert 1 in got["blk_odo"] and 7 in got["blk_odo"] and 3 in got["pose_odo"] and 2 not in got["pose_odo"]


@pytest.mark.parametrize("laser_pose", [5, 0])
def test_laser_edges_on_a_free_and_on_a_fixed_pose(driver, laser_pose):
    fixed, tracks = window(6, 1, 20)
    got = check(driver, graph(fixed, tracks, odo=[(4, 5), (5, 3)], n_laser=7, laser_pose=laser_pose), dict(solver=0))
    last = got["pose_odo"][got["pose_odo_ptr"][4]:got["pose_odo_ptr"][5]]
    assert last == ([1, 2, 4] if laser_pose == 5 else [1, 2])            # the pseudo edge 2 Ne comes last in its pose's list


@pytest.mark.parametrize("passes", [0, 1, 2])
def test_chunk_cuts_of_poses_and_blocks(driver, passes):
    # pose 1: 65 + 129 + 63 = 257 observations (two pose-major chunks); block (0, 1): 65 pairs, block (1, 2): 129 pairs
    tracks = [[0, 1]] * 65 + [[1, 2]] * 129 + [[1]] * 63
    got = check(driver, graph([0, 0, 0, 1], tracks), dict(solver=2, sch_passes=passes))
    assert got["pose_chunk_ptr"] == [0, 1, 3, 4] and got["chunk_ptr"] == [0, 65, 65 + 256, 65 + 257, 65 + 257 + 129]
    b01, b12 = got["blk_of"][1], got["blk_of"][5]
    per = lambda b: got["blk_chunk_ptr"][b + 1] - got["blk_chunk_ptr"][b]
    assert (per(b01), per(b12)) == ((1, 2) if passes == 2 else (2, 3)) and got["sch_chunk"] == (128 if passes == 2 else 64)


@pytest.mark.parametrize("npf,cu", [(64, -1), (65, -1), (64, 1), (65, 1), (65, 0)])
def test_pcg_code_table_and_slot_table(driver, npf, cu):
    fixed, tracks = window(npf + 1, 1, 90)
    got = check(driver, graph(fixed, tracks), dict(solver=2, pcg_cu=cu, throughput=1 if cu < 0 and npf == 65 else 0))
    assert got["pcg1"] == (npf <= 64) and len(got["pcg1_code"]) == (npf * npf if npf <= 64 else 0)
    assert got["pcg_cu"] == int(cu == 1 or (cu < 0 and npf == 65)) and (set(got["blk_slot"]) == {255 | 255 << 8}) == (got["pcg_cu"] == 0)
    assert check(driver, graph(fixed, tracks), dict(solver=2, pcg_cu=1, pcg_cu_fits=0))["pcg_cu"] == 0
    assert check(driver, graph(fixed, tracks), dict(solver=0, pcg_cu=1))["pcg1_code"] == []


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("answer", [1, 0])
def test_band_plan_of_a_banded_and_of_a_full_width_window(driver, wide, answer):
    fixed, tracks = window(13, 1, 60)
    if wide: tracks += [[1, 12]]                      # the widest block is (0, Npf - 1)
    got = check(driver, graph(fixed, tracks), dict(solver=0, band_plan_ok=answer))
    assert got["band_B"] == ((11 if wide else 2) if answer else -1) and len(got["band_code"]) == (12 * (got["band_B"] + 1) if answer else 0)
    forced = check(driver, graph(fixed, tracks), dict(solver=0, band_plan_ok=answer, band_rows=6))
    assert forced["band_rows"] == (6 if answer and not wide else got["band_rows"])           # accepted from B + 3 rows on, below the planned rows
    assert check(driver, graph(fixed, tracks), dict(solver=0, band=0))["band_B"] == -1


def test_run_plan_taken_refused_and_overridden(driver):
    fixed, tracks = window(12, 1, 100, span=4)
    g = graph(fixed, tracks)
    plain = check(driver, g, PCG)
    got = check(driver, g, dict(solver=2, schur_runs=1))
    assert plain["run_n"] == 0 and got["run_n"] > 0 and got["n_sch"] == 0 and got["run_k0"][-1] == len(g["obs_pose"]) and got["Npf"] == 11
    over = check(driver, g, dict(solver=2, schur_runs=1, run_lr=8, run_m=3))
    assert (over["run_LR"], over["run_M"], over["run_n"]) == (8, 3, (100 + 23) // 24)
    assert check(driver, g, dict(solver=2, schur_runs=1, run_lr=128, run_m=17))["run_desc"] == got["run_desc"]       # out of range: ignored
    # one landmark spanning more than RUN_MAX_W poses: refused, and the pair-list structures are the ordinary ones
    fixed = [1] * 59 + [0] * 11
    tracks = [[0, 69]] + [[59 + p for p in t if p < 11] for t in window(11, 0, 100, span=4)[1]]
    wide = graph(fixed, tracks)
    refused = check(driver, wide, dict(solver=2, schur_runs=1))
    ordinary = check(driver, wide, PCG)
    assert refused["Npf"] == 11 and refused == ordinary and refused["run_n"] == 0 and refused["n_sch"] > 0


def test_threaded_summary_matches_the_single_thread(driver):
    rng = np.random.default_rng(3)
    n_poses, n_lm = 40, 3000
    starts = np.sort(rng.integers(0, n_poses - 6, n_lm))
    tracks = [list(range(s, s + 6)) for s in starts]
    for l in range(0, n_lm, 97): tracks[l] = tracks[l][:2] + tracks[l][4:]          # some tracks with a gap
    g = graph([1, 1] + [0] * (n_poses - 2), tracks, point_fixed=range(0, n_lm, 50))
    assert len(g["obs_pose"]) >= 16384
    s = oracle.summary_fast(g)
    one = check(driver, g, dict(solver=0, threads=1), s)
    three = check(driver, g, dict(solver=0, threads=3), s)
    assert one == three


def test_refusals_return_their_status_and_message(driver):
    fixed, tracks = window(6, 1, 20)
    got = check(driver, graph(fixed, tracks), dict(solver=2, pairs_seen=2 ** 31))
    assert (got["status"], got["msg"]) == (ERR_UNSUPPORTED, "window too large (pair list)")
    assert check(driver, graph(fixed, tracks), dict(solver=2, pairs_seen=2 ** 31 - 1))["status"] == 0
    got = check(driver, graph([0] * 1025, []), PCG)
    assert (got["status"], got["msg"]) == (ERR_UNSUPPORTED, "Optimizer/Solver=2 (PCG) supports at most 1024 free poses; use the direct solver")
    assert check(driver, graph([0] * 1025, []), dict(solver=0))["status"] == 0
    star = graph([0] * 1024, [], odo=[(0, p) for p in range(1, 1024)])              # one block row of 1024 blocks
    got = check(driver, star, PCG)
    assert (got["status"], got["msg"]) == (ERR_UNSUPPORTED, "reduced camera system too large for the persistent PCG (LDS); use the direct solver")
    assert check(driver, star, dict(solver=0))["status"] == 0


def test_plan_header_stays_free_of_hip():
    """ba_plan.hpp and everything it includes from csrc/ must compile without HIP: no hip_runtime.h, no ba_math.hpp."""
    seen, todo = set(), ["ba_plan.hpp"]
    while todo:
        name = todo.pop()
        if name in seen: continue
        seen.add(name)
        for inc in re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, name)).read()):
            assert "hip/" not in inc and os.path.basename(inc) != "ba_math.hpp", f"{name} includes {inc}"
            if os.path.exists(os.path.join(CSRC, inc)) and os.path.dirname(inc) == "": todo.append(inc)
    assert {"ba_plan.hpp", "ba_limits.hpp", "worker_pool.hpp"} <= seen
