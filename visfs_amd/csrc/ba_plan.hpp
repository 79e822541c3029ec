// ba_plan.hpp — the host plan of a graph upload: the switches an upload reads, the O(N_obs) summary of the graph and the whole index
// structure of the reduced camera matrix S (DeviceGraph's static section, ba_device.hpp).  Pure integer work on host memory and free of
// HIP: ba_api.cpp stages what this header computes, tests/cpp/plan_driver.cpp runs it without a GPU (tests/test_upload_plan.py).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../include/visfs_ba.h"
#include "ba_limits.hpp"
#include "worker_pool.hpp"

namespace visfs_ba {

// ------------------------------------------------------------------ switches
inline bool env_set(const char* name) { return std::getenv(name) != nullptr; }
inline bool env_is_1(const char* name) { const char* e = std::getenv(name); return e && e[0] == '1'; }          // on when set and starting with 1
inline bool env_not_0(const char* name) { const char* e = std::getenv(name); return !(e && e[0] == '0'); }      // on unless set and starting with 0
inline int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }

// Every environment variable an upload reads, read once at its top (per upload, not per process: tests change them between uploads).
// Integers hold what was given (0: not set); the range checks sit where the value is used.  -1 in a three-state field: not set.
struct UploadSwitches {
    bool timing = false;           // VISFS_BA_TIMING (set at all)
    bool schur_runs = false;       // VISFS_BA_SCHUR_RUNS=1
    int run_lr = 0;                // VISFS_BA_RUN_LR
    int run_m = 0;                 // VISFS_BA_RUN_M
    int sch_passes = 0;            // VISFS_BA_SCH_PASSES
    bool pcg1 = true;              // VISFS_BA_PCG1 not 0
    int pcg_cu = -1;               // VISFS_BA_PCG_CU: 1 on, set to anything else off, -1 the handle's tuning decides
    bool band = true;              // VISFS_BA_BAND not 0
    int band_rows = 0;             // VISFS_BA_BAND_ROWS
    int group = 0;                 // VISFS_BA_GROUP
    bool fin_pcg = false;          // VISFS_BA_FIN_PCG=1
    int pcg_gather = 1;            // VISFS_BA_PCG_GATHER (fin_pcg needs 1)
    bool fin_arrive = false;       // VISFS_BA_FIN_ARRIVE=1
    int stamp_wg = 0;              // VISFS_BA_STAMP_WG
    bool fault_pcg = false;        // VISFS_BA_FAULT_PCG_TIMEOUT=1
    bool small_solve = true;       // VISFS_BA_SMALL_SOLVE not 0
    bool fused = false;            // VISFS_BA_FUSED=1
    int spec = -1;                 // VISFS_BA_SPEC: 1 on, set to anything else off, -1 the window's size decides
    bool spec_fused = true;        // VISFS_BA_SPEC_FUSED not 0
    bool batch_spec = false;       // VISFS_BA_BATCH_SPEC=1
    int decide_fused = -1;         // VISFS_BA_DECIDE_FUSED: 0 off, set to anything else on, -1 on unless a batch member
};
inline UploadSwitches read_upload_switches() {
    UploadSwitches s;
    s.timing = env_set("VISFS_BA_TIMING");
    s.schur_runs = env_is_1("VISFS_BA_SCHUR_RUNS");
    s.run_lr = env_int("VISFS_BA_RUN_LR", 0);
    s.run_m = env_int("VISFS_BA_RUN_M", 0);
    s.sch_passes = env_int("VISFS_BA_SCH_PASSES", 0);
    s.pcg1 = env_not_0("VISFS_BA_PCG1");
    s.pcg_cu = env_set("VISFS_BA_PCG_CU") ? env_is_1("VISFS_BA_PCG_CU") : -1;
    s.band = env_not_0("VISFS_BA_BAND");
    s.band_rows = env_int("VISFS_BA_BAND_ROWS", 0);
    s.group = env_int("VISFS_BA_GROUP", 0);
    s.fin_pcg = env_is_1("VISFS_BA_FIN_PCG");
    s.pcg_gather = env_int("VISFS_BA_PCG_GATHER", 1);
    s.fin_arrive = env_is_1("VISFS_BA_FIN_ARRIVE");
    s.stamp_wg = env_int("VISFS_BA_STAMP_WG", 0);
    s.fault_pcg = env_is_1("VISFS_BA_FAULT_PCG_TIMEOUT");
    s.small_solve = env_not_0("VISFS_BA_SMALL_SOLVE");
    s.fused = env_is_1("VISFS_BA_FUSED");
    s.spec = env_set("VISFS_BA_SPEC") ? env_is_1("VISFS_BA_SPEC") : -1;
    s.spec_fused = env_not_0("VISFS_BA_SPEC_FUSED");
    s.batch_spec = env_is_1("VISFS_BA_BATCH_SPEC");
    s.decide_fused = env_set("VISFS_BA_DECIDE_FUSED") ? env_not_0("VISFS_BA_DECIDE_FUSED") : -1;
    return s;
}

// ------------------------------------------------------------------ graph summary
// What the run-based Schur kernel (k_schur_runs) needs to know about 8 consecutive landmarks: how many observations they have and
// which poses (index space of the window, fixed ones included) those touch.
struct RunGroup { int32_t cnt = 0; int32_t lo = 0x7fffffff, hi = -1; };
constexpr int RUN_GROUP = 8;
struct alignas(128) SummaryPart {          // (one per thread, updated per observation: no two may share a cache line)
    std::vector<int32_t> cnt, run, pc, track;
    std::vector<RunGroup> grp;
    int64_t pairs = 0; int ok = 0; bool any_run = false, used = false; const char* bad = nullptr;
    int npf = 0; int cur = -1; bool cur_fixed = false;
    int first = -1, last = -1, c = 0; bool gap = false;         // the current landmark's free poses: a contiguous run unless `gap`
    void begin(int Npf, int Nl) {
        used = true; npf = Npf; cnt.assign(Npf + 1, 0); run.assign((size_t)Npf * Npf, 0); pc.clear(); track.clear();
        grp.assign((size_t)(Nl + RUN_GROUP - 1) / RUN_GROUP + 1, RunGroup());
        pairs = 0; ok = 0; any_run = false; bad = nullptr; cur = -1; first = last = -1; c = 0; gap = false;
    }
    // observations arrive landmark by landmark (a landmark never straddles two accumulators), poses ascending inside a landmark
    inline void add(int landmark, bool landmark_fixed, int a /* free index of the pose, -1: fixed */, int pose /* its index in the window */) {
        if (landmark != cur) { flush(); cur = landmark; cur_fixed = landmark_fixed; }
        { RunGroup& G = grp[(size_t)landmark / RUN_GROUP]; G.cnt++; G.lo = std::min(G.lo, pose); G.hi = std::max(G.hi, pose); }
        ok += !(a < 0 && landmark_fixed);
        if (a < 0) return;
        cnt[a + 1]++;
        if (c == 0) { first = last = a; c = 1; return; }
        if (!gap && a != last + 1) { gap = true; track.clear(); for (int q = first; q <= last; ++q) track.push_back(q); }   // (rare) the members so far were a run
        if (gap) track.push_back(a);
        last = a; ++c;
    }
    void flush() {
        if (cur >= 0 && !cur_fixed && c > 0) {
            pairs += (int64_t)c * (c + 1) / 2;
            if (!gap) { run[(size_t)first * npf + last]++; any_run = true; }
            else {
                if (pc.empty()) pc.assign((size_t)npf * npf, 0);      // tracks with gaps are rare: their pairwise table only exists when one shows up
                for (int i = 0; i < c; ++i) { int32_t* row = pc.data() + (size_t)track[i] * npf; for (int j = i; j < c; ++j) row[track[j]]++; }
            }
        }
        c = 0; gap = false; first = last = -1;
    }
};

// What the host has to know about the O(N_obs) part of the graph: observations per free pose and co-observation pairs per block of S.
struct GraphSummary {
    std::vector<int32_t> cnt;          // [Npf + 1] prefix: observations of free pose a at pose-major positions [cnt[a], cnt[a + 1])
    std::vector<int32_t> pcount;       // [Npf][Npf] (a <= b): free landmarks observed by both
    int64_t pairs_seen = 0;
    int n_edges_ok = 0;
    const char* bad = nullptr;
    std::vector<RunGroup> grp;         // per RUN_GROUP consecutive landmarks
};
// One pass over the observations (landmark-major), shared out over the pool at landmark boundaries.
// A landmark seen by the free poses {a_1 < ... < a_k} adds one pair to every block (a_i, a_j), i <= j.  Tracks are runs of consecutive
// key-frames almost always (a feature is tracked frame to frame and never re-acquired), so a landmark whose free poses form the
// contiguous range [s, e] only bumps run[s][e]; the blocks are then counted by one 2-D inclusion sum, pcount[a][b] = sum over s <= a,
// e >= b of run[s][e] — O(Nl + Npf^2) instead of O(sum k^2).  Landmarks with gaps in their track take the pairwise loop.
inline void merge_summary(std::vector<SummaryPart>& part, const int NT, const int Npf, GraphSummary& S, std::vector<int32_t>& run) {
    const size_t nn = (size_t)Npf * Npf;
    S.cnt.assign(Npf + 1, 0); S.pcount.assign(nn, 0); S.pairs_seen = 0; S.n_edges_ok = 0; S.bad = nullptr;
    run.assign(nn, 0);
    bool any_run = false;
    for (int t = 0; t < NT; ++t) {
        const SummaryPart& P = part[t];
        if (!P.used) continue;
        if (P.bad) { S.bad = P.bad; return; }
        for (int a = 0; a <= Npf; ++a) S.cnt[a] += P.cnt[a];
        if (!P.pc.empty()) for (size_t q = 0; q < nn; ++q) S.pcount[q] += P.pc[q];
        for (size_t q = 0; q < nn; ++q) run[q] += P.run[q];
        S.pairs_seen += P.pairs; S.n_edges_ok += P.ok; any_run = any_run || P.any_run;
    }
    for (int a = 0; a < Npf; ++a) S.cnt[a + 1] += S.cnt[a];
    S.grp.clear();
    for (int t = 0; t < NT; ++t) {
        const SummaryPart& P = part[t];
        if (!P.used) continue;
        if (S.grp.size() < P.grp.size()) S.grp.resize(P.grp.size());
        for (size_t q = 0; q < P.grp.size(); ++q) { RunGroup& G = S.grp[q]; G.cnt += P.grp[q].cnt; G.lo = std::min(G.lo, P.grp[q].lo); G.hi = std::max(G.hi, P.grp[q].hi); }
    }
    if (any_run) {
        // in place: run[a][b] <- sum_{s <= a, e >= b} run[s][e]
        for (int a = 0; a < Npf; ++a)
            for (int b2 = Npf - 1; b2 >= 0; --b2) {
                int64_t v = run[(size_t)a * Npf + b2];
                if (a > 0) v += run[(size_t)(a - 1) * Npf + b2];
                if (b2 + 1 < Npf) v += run[(size_t)a * Npf + b2 + 1];
                if (a > 0 && b2 + 1 < Npf) v -= run[(size_t)(a - 1) * Npf + b2 + 1];
                run[(size_t)a * Npf + b2] = (int32_t)v;
            }
        for (int a = 0; a < Npf; ++a) for (int b2 = a; b2 < Npf; ++b2) S.pcount[(size_t)a * Npf + b2] += run[(size_t)a * Npf + b2];
    }
}
inline void summarize_graph(const visfs_ba_graph* gr, const int32_t* pose_free, const int Npf, WorkerPool* pool, const bool check, GraphSummary& S,
                            std::vector<SummaryPart>& part, std::vector<int32_t>& run) {
    const int No = gr->n_obs, Nl = gr->n_points, Np = gr->n_poses;
    const size_t nn = (size_t)Npf * Npf;
    // several tasks per thread (a worker that wakes late still finds work); accumulators per THREAD, not per task
    const int NT = (pool && No >= 16384 && nn <= ((size_t)1 << 17)) ? pool->size() : 1;
    const int T = NT > 1 ? 4 * NT : 1;
    std::vector<int> cut(T + 1, No);
    cut[0] = 0;
    for (int t = 1; t < T; ++t) {
        int k = (int)((int64_t)No * t / T);
        k = std::max(k, cut[t - 1]);
        while (k > 0 && k < No && gr->obs_point[k] == gr->obs_point[k - 1]) ++k;     // a landmark's observations stay with one task
        cut[t] = k;
    }
    if ((int)part.size() < NT) part.resize(NT);
    for (int t = 0; t < NT; ++t) part[t].used = false;
    auto body = [&](int t, int slot) {
        SummaryPart& P = part[slot];
        if (!P.used) P.begin(Npf, Nl);
        if (P.bad) return;
        for (int k = cut[t]; k < cut[t + 1]; ++k) {
            const int l = gr->obs_point[k], cp = gr->obs_pose[k];
            if (check) {
                if (l < 0 || l >= Nl || cp < 0 || cp >= Np) { P.bad = "observation index out of range"; return; }
                if (k > 0 && (l < gr->obs_point[k - 1] || (l == gr->obs_point[k - 1] && cp <= gr->obs_pose[k - 1]))) { P.bad = "observations must be sorted by (point, pose) and unique"; return; }
            }
            P.add(l, gr->point_fixed[l] != 0, pose_free[cp], cp);
        }
        P.flush();
    };
    if (T > 1) pool->run(T, body); else body(0, 0);
    merge_summary(part, NT, Npf, S, run);
}

// ------------------------------------------------------------------ the plan
// A descriptor of the index section: the device reads it as one int4 (ba_api.cpp asserts the layout).
struct alignas(16) Desc4 { int32_t x, y, z, w; };
inline Desc4 desc4(int x, int y, int z, int w) { return Desc4{ x, y, z, w }; }

// What the plan cannot decide itself: the handle's choices, the switches, and what the kernels' own size predicates (ba_kernels.hip) answer.
struct PlanDecisions {
    int solver = 0;                    // visfs_ba_params::solver
    bool batch_member = false;
    bool throughput = false;           // the handle's tuning is VISFS_BA_TUNE_THROUGHPUT
    int index_blocks = 0;              // workgroups of the upload's index-building launch (its histogram is [index_blocks][Npf])
    UploadSwitches sw;
    bool (*band_plan)(int npf, int B, int* rows, int* lds_bytes) = nullptr;
    size_t (*band_lds_bytes)(int npf, int B, int rows) = nullptr;
    bool (*pcg_cu_fits)(int npf, int max_row) = nullptr;
};

// The graph as the plan sees it (the summary carries everything of size N_obs).
struct PlanGraph {
    int Np = 0, Nl = 0, No = 0, Ne = 0, Nz = 0;        // Ne: odometry edges in use, Nz: laser points in use (0 when their pose is fixed)
    const int32_t* odo_from = nullptr; const int32_t* odo_to = nullptr;
    int laser_pose = 0;
};

struct RunPlan { int LR = 0, M = 1, n = 0, cap = 0, wmax = 0; size_t lds = 0; int64_t total = 0; std::vector<Desc4> desc; std::vector<int32_t> first, last, k0; };

struct UploadPlan {
    int status = VISFS_BA_OK; const char* msg = nullptr;        // a refusal: the error code and text of the upload
    int Np = 0, Nl = 0, No = 0, Ne = 0, Nz = 0, Npf = 0, n_pose_obs = 0, n_edges_ok = 0, solver = 0;
    std::vector<int32_t> pose_free, free_pose;
    std::vector<int32_t> chunk_pose, chunk_ptr, pose_chunk_ptr;
    std::vector<int32_t> pose_odo_ptr, pose_odo;
    std::vector<int32_t> blk_i, blk_j, blk_ptr, blk_of;
    std::vector<int32_t> blk_odo_ptr, blk_odo;
    std::vector<int32_t> row_ptr, row_col, row_blk;
    std::vector<int32_t> blk_chunk_ptr, sch_blk;
    std::vector<Desc4> sch_desc, blk_desc;                      // [max(n_sch, 1)], [2 max(n_blk, 1)]
    std::vector<int32_t> fin_exp, diag_blk;
    std::vector<int32_t> pcg1_code, blk_slot, band_code;        // blk_slot: [max(n_blk, 1)]
    RunPlan run;
    int n_chunks = 0, n_blk = 0, n_sch = 0, sch_chunk = SCH_CHUNK, max_row = 0;
    int64_t npairs = 0;
    int pcg_rpw = 1, lds_srow = 0, cu_T = 0, cu_max_row = 0;
    size_t pcg_lds = 0;
    bool pcg1 = false, pcg_cu = false, small_fits = false;      // small_fits: 6 Npf <= SM_MAX_N6, k_small_solve can serve the window
    int band_B = -1, band_rows = 0, band_lds = 0;
    int group = 4, n_lin_a = 1, n_parts = 1;
    size_t chol_np = 32, n_hist = 1;
    bool run_path() const { return run.n > 0; }
    bool refuse(int code, const char* text) { status = code; msg = text; return false; }
};

// buildIndexMapping: free poses in index (= id) order
inline void plan_poses(UploadPlan& P, const uint8_t* pose_fixed, const int Np) {
    P.pose_free.assign(Np, -1); P.free_pose.clear();
    for (int i = 0; i < Np; ++i) if (!pose_fixed[i]) { P.pose_free[i] = (int32_t)P.free_pose.size(); P.free_pose.push_back(i); }
    P.Np = Np; P.Npf = (int)P.free_pose.size();
}

// pose-major chunks
inline bool plan_chunks(UploadPlan& P, const std::vector<int32_t>& cnt) {
    const int Npf = P.Npf;
    P.chunk_pose.clear(); P.chunk_ptr.clear(); P.pose_chunk_ptr.assign(Npf + 1, 0);
    P.chunk_pose.reserve((size_t)cnt[Npf] / LIN_CHUNK + Npf + 1); P.chunk_ptr.reserve((size_t)cnt[Npf] / LIN_CHUNK + Npf + 2);
    for (int a = 0; a < Npf; ++a) {
        P.pose_chunk_ptr[a] = (int32_t)P.chunk_pose.size();
        for (int s = cnt[a]; s < cnt[a + 1]; s += LIN_CHUNK) { P.chunk_pose.push_back(a); P.chunk_ptr.push_back(s); }
    }
    P.pose_chunk_ptr[Npf] = (int32_t)P.chunk_pose.size();
    P.n_chunks = (int)P.chunk_pose.size();
    P.chunk_ptr.push_back(cnt[Npf]);
    // k_linearize reads [chunk_ptr[c], chunk_ptr[c+1]) — consecutive chunks are contiguous: chunk c of pose a ends where the next starts
    for (int c = 0; c + 1 < P.n_chunks; ++c)
        if (P.chunk_ptr[c + 1] != std::min(P.chunk_ptr[c] + LIN_CHUNK, cnt[P.chunk_pose[c] + 1])) return P.refuse(VISFS_BA_ERR_BAD_ARGUMENT, "internal: chunk layout");
    return true;
}

// odometry incidence (per free pose: its edges in edge order, 2e = as `from`, 2e + 1 = as `to`; counting pass, then fill — no
// per-pose containers: this section runs on the caller's thread between the graph build and the first launch)
inline void plan_odo_incidence(UploadPlan& P, const PlanGraph& G) {
    const int Npf = P.Npf, Ne = G.Ne;
    const std::vector<int32_t>& pose_free = P.pose_free;
    P.pose_odo_ptr.assign(Npf + 1, 0);
    for (int e = 0; e < Ne; ++e) {
        const int a = pose_free[G.odo_from[e]], b = pose_free[G.odo_to[e]];
        if (a >= 0) P.pose_odo_ptr[a + 1]++;
        if (b >= 0) P.pose_odo_ptr[b + 1]++;
    }
    // the laser edges' aggregate lives in slot Ne of odo_blk as the "from" side of a pseudo edge (added last, as g2o does)
    if (G.Nz > 0) P.pose_odo_ptr[pose_free[G.laser_pose] + 1]++;
    for (int a = 0; a < Npf; ++a) P.pose_odo_ptr[a + 1] += P.pose_odo_ptr[a];
    P.pose_odo.assign(P.pose_odo_ptr[Npf], 0);
    std::vector<int32_t> at(P.pose_odo_ptr.begin(), P.pose_odo_ptr.end() - 1);
    for (int e = 0; e < Ne; ++e) {
        const int a = pose_free[G.odo_from[e]], b = pose_free[G.odo_to[e]];
        if (a >= 0) P.pose_odo[at[a]++] = 2 * e;
        if (b >= 0) P.pose_odo[at[b]++] = 2 * e + 1;
    }
    if (G.Nz > 0) P.pose_odo[at[pose_free[G.laser_pose]]++] = 2 * Ne;
}

// S block structure (g2o buildStructure analogue): per block (i<=j) the co-observation pairs, and the odometry edges that add to it
inline bool plan_blocks(UploadPlan& P, const PlanGraph& G, const GraphSummary& sum) {
    const int Npf = P.Npf, Ne = G.Ne;
    const std::vector<int32_t>& pose_free = P.pose_free;
    const std::vector<int32_t>& pcount = sum.pcount;
    std::vector<uint8_t> has_odo((size_t)Npf * Npf, 0);
    if (sum.pairs_seen > 0x7fffffff) return P.refuse(VISFS_BA_ERR_UNSUPPORTED, "window too large (pair list)");
    for (int e = 0; e < Ne; ++e) {
        int a = pose_free[G.odo_from[e]], b = pose_free[G.odo_to[e]];
        if (a < 0 || b < 0) continue;
        if (a > b) std::swap(a, b);
        has_odo[(size_t)a * Npf + b] = 1;
    }
    P.blk_i.clear(); P.blk_j.clear(); P.blk_ptr.assign(1, 0); P.blk_of.assign((size_t)Npf * Npf, -1);
    P.blk_i.reserve((size_t)Npf * 16); P.blk_j.reserve((size_t)Npf * 16); P.blk_ptr.reserve((size_t)Npf * 16 + 1);
    P.npairs = 0;
    for (int a = 0; a < Npf; ++a)
        for (int b = a; b < Npf; ++b) {
            const size_t key = (size_t)a * Npf + b;
            if (a == b || pcount[key] > 0 || has_odo[key]) {
                P.blk_of[key] = (int32_t)P.blk_i.size();
                P.blk_i.push_back(a); P.blk_j.push_back(b);
                P.npairs += pcount[key];
                if (P.npairs > 0x7fffffff) return P.refuse(VISFS_BA_ERR_UNSUPPORTED, "window too large (pair list)");
                P.blk_ptr.push_back((int32_t)P.npairs);
            }
        }
    const int n_blk = P.n_blk = (int)P.blk_i.size();
    P.blk_odo_ptr.assign(n_blk + 1, 0); P.blk_odo.clear();
    if (Ne > 0) {
        // Aij is (row = from, col = to): stored block is (min,max); transposed when from > to
        auto slot = [&](int e, int& code) {
            const int a = pose_free[G.odo_from[e]], b = pose_free[G.odo_to[e]];
            if (a < 0 || b < 0) return -1;
            if (a < b) { code = 2 * e; return (int)P.blk_of[(size_t)a * Npf + b]; }
            code = 2 * e + 1; return (int)P.blk_of[(size_t)b * Npf + a];
        };
        int code = 0;
        for (int e = 0; e < Ne; ++e) { const int b = slot(e, code); if (b >= 0) P.blk_odo_ptr[b + 1]++; }
        for (int b = 0; b < n_blk; ++b) P.blk_odo_ptr[b + 1] += P.blk_odo_ptr[b];
        P.blk_odo.assign(P.blk_odo_ptr[n_blk], 0);
        std::vector<int32_t> at(P.blk_odo_ptr.begin(), P.blk_odo_ptr.end() - 1);
        for (int e = 0; e < Ne; ++e) { const int b = slot(e, code); if (b >= 0) P.blk_odo[at[b]++] = code; }
    }
    return true;
}

// block-row adjacency of the symmetric S for the mat-vec: row r = its transposed blocks (i < r, code 2b + 1) in ascending i, then its
// own blocks (j >= r, code 2b) in ascending j — the blocks are enumerated in (i, j) order, so both halves arrive sorted by column
inline void plan_rows(UploadPlan& P) {
    const int Npf = P.Npf, n_blk = P.n_blk;
    const std::vector<int32_t>& blk_i = P.blk_i; const std::vector<int32_t>& blk_j = P.blk_j;
    P.row_ptr.assign(Npf + 1, 0);
    for (int b = 0; b < n_blk; ++b) { P.row_ptr[blk_i[b] + 1]++; if (blk_i[b] != blk_j[b]) P.row_ptr[blk_j[b] + 1]++; }
    for (int a = 0; a < Npf; ++a) P.row_ptr[a + 1] += P.row_ptr[a];
    P.row_col.assign(P.row_ptr[Npf], 0); P.row_blk.assign(P.row_ptr[Npf], 0);
    std::vector<int32_t> at(P.row_ptr.begin(), P.row_ptr.end() - 1);
    for (int b = 0; b < n_blk; ++b) if (blk_i[b] != blk_j[b]) { const int r = blk_j[b]; P.row_col[at[r]] = blk_i[b]; P.row_blk[at[r]] = 2 * b + 1; at[r]++; }
    for (int b = 0; b < n_blk; ++b) { const int r = blk_i[b]; P.row_col[at[r]] = blk_j[b]; P.row_blk[at[r]] = 2 * b; at[r]++; }
    P.max_row = 0;
    for (int a = 0; a < Npf; ++a) P.max_row = std::max(P.max_row, P.row_ptr[a + 1] - P.row_ptr[a]);
}

// most observations of any sub-batch of LR consecutive landmarks
inline int run_batch_cap(const std::vector<RunGroup>& grp, const int ng, const int LR) {
    const int gper = LR / RUN_GROUP;
    int maxc = 0;
    for (int g0 = 0; g0 < ng; g0 += gper) { int c = 0; for (int q = g0; q < std::min(ng, g0 + gper); ++q) c += grp[q].cnt; maxc = std::max(maxc, c); }
    return maxc;
}

// ---- Schur complement by RUNS OF LANDMARKS (k_schur_runs, ba_kernels.hip): the plan.  A workgroup owns run_lr x run_m consecutive
// landmarks; run_lr is the largest of 64 / 32 / 16 / 8 whose sub-batches never hold more than RUN_MAX_TILES observations (their tiles are
// staged in LDS); a run's blocks are those of its pose span [lo, lo + W) — from the structure summary, which has seen every observation's
// landmark and pose.  Windows it does not fit (a span above RUN_MAX_W poses: landmarks whose ids do not grow with time; reduced systems
// that k_small_solve serves; VISFS_BA_SCHUR_RUNS=0) keep the pair-list gather.  A property of the window alone.
inline void plan_runs(UploadPlan& P, const GraphSummary& sum, const UploadSwitches& sw) {
    // Measured (profiles/r04_schur_lds_tiles.log): a third of the gather's VALU instructions per pair, but every workgroup is a chain
    // of barrier-separated phases (descriptors, global loads, D_l / R_i, tiles, accumulate, three reduction passes: 12 us stamped at C2)
    // at two to three waves per SIMD — 15.7 us per launch against the gather's 8.7 at C2, 34 against 29.5 at the 200-key-frame window,
    // 16 resident windows 78.6 k against 79.0 k it/s at best.  The gather stays the default; VISFS_BA_SCHUR_RUNS=1 selects this kernel
    // (tests, A/B runs).
    RunPlan& rp = P.run;
    rp = RunPlan();
    const int Np = P.Np, Nl = P.Nl, No = P.No, Npf = P.Npf, n_blk = P.n_blk;
    const int ng = (Nl + RUN_GROUP - 1) / RUN_GROUP;
    if (!(sw.schur_runs && Npf >= 1 && No > 0 && Nl > 0 && (size_t)6 * Npf > (size_t)SM_MAX_N6 && (int)sum.grp.size() >= ng && Np < 65536)) return;
    // (first choice: sub-batches of at most 176 tiles — 30 KB of LDS, three workgroups and more per CU; else whatever fits at all)
    for (int limit : { 176, RUN_MAX_TILES }) {
        for (int LR : { 64, 32, 16, 8 }) {
            const int maxc = run_batch_cap(sum.grp, ng, LR);
            if (maxc <= limit) { rp.LR = LR; rp.cap = maxc; break; }
        }
        if (rp.LR) break;
    }
    { const int q = sw.run_lr;                                                                                        // tuning override (never above what fits)
      if (rp.LR && (q == 8 || q == 16 || q == 32 || q == 64) && q < rp.LR) { rp.LR = q; rp.cap = run_batch_cap(sum.grp, ng, q); } }
    if (!rp.LR) return;
    // sub-batches per workgroup: one, until the window has so many landmarks that a partial per run and block costs more traffic
    // than the workgroups it keeps busy (a 200-key-frame window: ~940 runs of 32 landmarks at M = 1)
    rp.M = std::max(1, 32 / rp.LR);                 // at least 32 landmarks per workgroup: a partial per run and block is traffic
    while ((Nl + rp.LR * rp.M - 1) / (rp.LR * rp.M) > 1024 && rp.M < 16) rp.M *= 2;
    if (sw.run_m >= 1 && sw.run_m <= 16) rp.M = sw.run_m;
    const int per = rp.LR * rp.M, gper = per / RUN_GROUP;
    rp.n = (Nl + per - 1) / per;
    rp.desc.assign(rp.n, desc4(0, 0, 0, 0));
    bool ok = rp.n < (1 << 20);
    int nbmax = 0;
    for (int r = 0; r < rp.n && ok; ++r) {
        int lo = 0x7fffffff, hi = -1;
        for (int q = r * gper; q < std::min(ng, (r + 1) * gper); ++q) if (sum.grp[q].cnt > 0) { lo = std::min(lo, sum.grp[q].lo); hi = std::max(hi, sum.grp[q].hi); }
        const int W = hi >= lo ? hi - lo + 1 : 0;
        if (W > RUN_MAX_W) { ok = false; break; }
        rp.desc[r] = desc4(W ? lo : 0, W, (int)rp.total, 0);
        rp.total += (int64_t)W * (W + 1) / 2;
        rp.wmax = std::max(rp.wmax, W); nbmax = std::max(nbmax, W * (W + 1) / 2);
        if (rp.total > 0x3fffffff) ok = false;
    }
    if (ok) {
        // per stored block of S: the range of runs whose span holds both of its poses (k_schur_finalize walks it)
        rp.first.assign(n_blk, 0x7fffffff); rp.last.assign(n_blk, -1);
        for (int r = 0; r < rp.n; ++r) {
            const int lo = rp.desc[r].x, W = rp.desc[r].y;
            for (int li = 0; li < W; ++li) {
                const int a = P.pose_free[lo + li];
                if (a < 0) continue;
                for (int lj = li; lj < W; ++lj) {
                    const int b2 = P.pose_free[lo + lj];
                    if (b2 < 0) continue;
                    const int bk = P.blk_of[(size_t)a * Npf + b2];
                    if (bk >= 0) { rp.first[bk] = std::min(rp.first[bk], r); rp.last[bk] = std::max(rp.last[bk], r); }
                }
            }
        }
        for (int b = 0; b < n_blk && ok; ++b) if (rp.last[b] >= 0 && rp.last[b] - rp.first[b] + 1 > 4095) ok = false;
    }
    if (!ok) { rp = RunPlan(); return; }
    rp.lds = (((size_t)std::max(rp.cap, (256 * 14 + RUN_TILE - 1) / RUN_TILE) * RUN_TILE + 9 * (size_t)rp.LR + 9 * (size_t)rp.wmax) * 8 + (((size_t)rp.LR * rp.wmax + 3) & ~size_t(3)) * 2 + (size_t)nbmax * 2 + 15) & ~size_t(15);
    // first observation of every sub-batch of run_lr landmarks (observations are landmark-major: a prefix sum of the groups' counts)
    const int nsub = rp.n * rp.M, gl = rp.LR / RUN_GROUP;
    rp.k0.assign((size_t)nsub + 1, 0);
    int acc = 0;
    for (int sb = 0; sb < nsub; ++sb) { rp.k0[sb] = acc; for (int q = sb * gl; q < std::min(ng, (sb + 1) * gl); ++q) acc += sum.grp[q].cnt; }
    rp.k0[nsub] = acc;
    if (acc != No) rp = RunPlan();                 // (cannot happen: every observation was counted once)
}

// Schur chunks: <= SCH_CHUNK co-observation pairs of one block per wavefront; the chunk and block descriptors; what fin_arrive expects
// A lane may take several pairs of its chunk (64 per pass) and add them serially before the wave's reduce-scatter.  Measured
// (profiles/r01_v8_schur_passes.log): two passes win 4-5 % on a lone mid-size window (C2: half the waves, half the partials
// for k_schur_finalize to sum, all of them still resident in one round) and lose 4-7 % once the launch fills the machine
// (C4, batched windows: the serial variant needs 216 VGPRs, 2 waves per SIMD instead of 4).  Results differ from the
// one-pass chunking in the last bits only (summation order).
inline void plan_schur(UploadPlan& P, const PlanDecisions& D) {
    const int n_blk = P.n_blk;
    const bool run_path = P.run_path();
    const RunPlan& rp = P.run;
    const std::vector<int32_t>& blk_i = P.blk_i; const std::vector<int32_t>& blk_j = P.blk_j; const std::vector<int32_t>& blk_ptr = P.blk_ptr;
    int64_t chunks64 = 0;
    for (int b = 0; b < n_blk; ++b) chunks64 += (blk_ptr[b + 1] - blk_ptr[b] + SCH_CHUNK - 1) / SCH_CHUNK;
    int sch_passes = (!D.batch_member && chunks64 >= 1024 && chunks64 <= 6144) ? 2 : 1;
    if (D.sw.sch_passes >= 1 && D.sw.sch_passes <= 8) sch_passes = D.sw.sch_passes;
    const int sch_chunk = P.sch_chunk = SCH_CHUNK * sch_passes;
    std::vector<int32_t> sch_ptr;
    P.blk_chunk_ptr.assign(n_blk + 1, 0); P.sch_blk.clear();
    if (!run_path) { P.sch_blk.reserve((size_t)(P.npairs / sch_chunk) + n_blk + 1); sch_ptr.reserve((size_t)(P.npairs / sch_chunk) + n_blk + 1); }
    for (int b = 0; b < n_blk; ++b) {
        P.blk_chunk_ptr[b] = (int32_t)P.sch_blk.size();
        if (run_path) continue;                             // (no pair lists, no chunks: the runs replace them)
        for (int e = blk_ptr[b]; e < blk_ptr[b + 1]; e += sch_chunk) { P.sch_blk.push_back(b); sch_ptr.push_back(e); }
    }
    P.blk_chunk_ptr[n_blk] = (int32_t)P.sch_blk.size();
    const int n_sch = P.n_sch = (int)P.sch_blk.size();
    P.sch_desc.assign(std::max(n_sch, 1), desc4(0, 0, 0, 0)); P.blk_desc.assign(2 * (size_t)std::max(n_blk, 1), desc4(0, 0, 0, 0));
    for (int c = 0; c < n_sch; ++c) {
        const int b = P.sch_blk[c];
        P.sch_desc[c] = desc4(sch_ptr[c], std::min(sch_ptr[c] + sch_chunk, blk_ptr[b + 1]), P.free_pose[blk_i[b]], P.free_pose[blk_j[b]]);
    }
    P.fin_exp.assign(n_blk, 0); P.diag_blk.assign(P.Npf, 0);
    for (int b = 0; b < n_blk; ++b) {
        const int a = blk_i[b];
        const bool dg = (a == blk_j[b]);
        P.blk_desc[2 * b] = desc4(P.blk_chunk_ptr[b], P.blk_chunk_ptr[b + 1], dg ? P.pose_odo_ptr[a] : P.blk_odo_ptr[b], dg ? P.pose_odo_ptr[a + 1] : P.blk_odo_ptr[b + 1]);
        if (run_path) {
            const int cnt_r = rp.last[b] >= 0 ? rp.last[b] - rp.first[b] + 1 : 0;
            P.blk_desc[2 * b].x = (int)((unsigned)(cnt_r ? rp.first[b] : 0) | ((unsigned)cnt_r << 20));
            P.blk_desc[2 * b].y = (int)((unsigned)P.free_pose[a] | ((unsigned)P.free_pose[blk_j[b]] << 16));
        }
        P.blk_desc[2 * b + 1] = desc4(a, blk_j[b], P.pose_chunk_ptr[a], P.pose_chunk_ptr[a + 1]);
        P.fin_exp[b] = (P.blk_chunk_ptr[b + 1] - P.blk_chunk_ptr[b]) | ((dg ? P.pose_chunk_ptr[a + 1] - P.pose_chunk_ptr[a] : 0) << 16);
        if (dg) P.diag_blk[a] = b;
    }
}

// the PCG forms: the LDS plan of the persistent kernel, k_pcg1's code table, k_pcg_cu's slot table
inline bool plan_pcg(UploadPlan& P, const PlanDecisions& D) {
    const int Npf = P.Npf, n_blk = P.n_blk, max_row = P.max_row;
    if (D.solver == 2 && Npf > MAX_PCG_FREE_POSES) return P.refuse(VISFS_BA_ERR_UNSUPPORTED, "Optimizer/Solver=2 (PCG) supports at most 1024 free poses; use the direct solver");
    // persistent PCG: LDS plan.  d, q, scalars, the rows' column/code tables always; s = Minv r when an owner thread holds several
    // blocks; the own block rows of S when they fit.  Co-residency of the hand-off needs every workgroup resident: one block row
    // per workgroup up to 256 free poses, ceil(Npf / 256) rows per workgroup beyond (at most 256 workgroups, one per CU).
    const int pcg_rpw = P.pcg_rpw = Npf > MAX_PCG_ONE_ROW_POSES ? (Npf + MAX_PCG_ONE_ROW_POSES - 1) / MAX_PCG_ONE_ROW_POSES : 1;
    P.pcg_lds = (size_t)(2 * 6 * Npf + 32 + 32 * pcg_rpw + (Npf > MAX_PCG_ONE_ROW_POSES ? 6 * Npf : 0)) * 8 + (size_t)8 * max_row * pcg_rpw + 16;
    P.lds_srow = 0;                                       // (Minv: registers — one block per owner — or, beyond 256 free poses, read from HBM)
    {
        const size_t budget = (size_t)150 * 1024;        // one workgroup per CU may own most of its 160 KiB
        if (P.pcg_lds + (size_t)288 * max_row * pcg_rpw <= budget) { P.lds_srow = 1; P.pcg_lds += (size_t)288 * max_row * pcg_rpw; }
    }
    if (D.solver == 2 && P.pcg_lds > (size_t)160 * 1024) return P.refuse(VISFS_BA_ERR_UNSUPPORTED, "reduced camera system too large for the persistent PCG (LDS); use the direct solver");

    // k_pcg1 (one wavefront per block row, <= 64 free poses): the block of S at (i, a) as a dense code table
    P.pcg1 = D.solver == 2 && Npf >= 1 && Npf <= 64 && D.sw.pcg1;
    P.pcg1_code.clear();
    if (P.pcg1) {
        P.pcg1_code.assign((size_t)Npf * Npf, -1);
        for (int a = 0; a < Npf; ++a)
            for (int n = P.row_ptr[a]; n < P.row_ptr[a + 1]; ++n) P.pcg1_code[(size_t)a * Npf + P.row_col[n]] = P.row_blk[n];
    }
    // k_pcg_cu: the whole PCG in one workgroup when every block row is short enough to sit in registers (3 threads per scalar row)
    // One window: slower than k_pcg1 (34.7 vs 21.6 us per solve at C2, profiles/r02_pcg_cu_vs_handoff.log).  Many windows sharing every
    // launch: nothing spins and no hand-off is paid — 16 C2 windows 68.0 -> 70.6 k it/s, 32 windows 66.6 -> 74.3 k, but 8 windows
    // 58.8 -> 55.6 k (profiles/r02_v3_pcg_cu_batches.log).  Its mat-vec sums associate differently from k_pcg1's, so a window's result
    // would depend on how many OTHER windows were submitted with it if the kernel followed the batch size: it follows the HANDLE
    // (visfs_ba_set_tuning(THROUGHPUT), ABI 8; VISFS_BA_PCG_CU=0|1 overrides), never the batch — every window is bit-identical to
    // its solve as a batch of one through the same handle however a batch is cut or sharded.
    const bool want_cu = D.sw.pcg_cu >= 0 ? D.sw.pcg_cu == 1 : D.throughput;      // (the environment overrides every handle)
    P.pcg_cu = D.solver == 2 && D.pcg_cu_fits(Npf, max_row) && 6 * Npf > 64 && want_cu;
    // ... and where each stored block sits in the row lists: k_schur_finalize writes S a second time by scalar row for that kernel
    P.cu_T = (int)((6 * (size_t)Npf + 63) / 64 * 64);
    P.cu_max_row = max_row;
    P.blk_slot.assign(std::max(n_blk, 1), 255 | (255 << 8));
    if (P.pcg_cu)
        for (int a = 0; a < Npf; ++a)
            for (int n = P.row_ptr[a]; n < P.row_ptr[a + 1]; ++n) {
                const int b = P.row_blk[n] >> 1, k = n - P.row_ptr[a];
                if (P.row_blk[n] & 1) P.blk_slot[b] = (P.blk_slot[b] & 0xff) | (k << 8); else P.blk_slot[b] = (P.blk_slot[b] & ~0xff) | k;
            }
    return true;
}

// direct solver (Optimizer/Solver 0, 1, 3 and every solve of the Ceres branch): S of a sliding window is block-banded — the banded
// factorisation in one workgroup (k_band_chol) when the band is narrow enough, the dense blocked Cholesky otherwise (VISFS_BA_BAND=0 forces it)
// (Optimizer/Solver=2 windows get the plan too: it is what a solve falls back to when the persistent PCG's hand-off times out — a GPU
// kept busy by another process —, so that the call still returns a solution as the reference's solver always does, Optimizer.cpp:76-91)
inline void plan_band(UploadPlan& P, const PlanDecisions& D) {
    const int Npf = P.Npf, n_blk = P.n_blk;
    P.band_B = -1; P.band_rows = 0; P.band_lds = 0; P.band_code.clear();
    if (Npf < 1) return;
    int Bw = 0;
    for (int b = 0; b < n_blk; ++b) Bw = std::max(Bw, P.blk_j[b] - P.blk_i[b]);
    if (!(D.sw.band && D.band_plan(Npf, Bw, &P.band_rows, &P.band_lds))) return;
    { const int q = D.sw.band_rows;                                                                    // tests: force the streaming form
      if (q >= Bw + 3 && q < P.band_rows) { P.band_rows = q; P.band_lds = (int)D.band_lds_bytes(Npf, Bw, q); } }
    P.band_B = Bw;
    P.band_code.assign((size_t)Npf * (Bw + 1), -1);
    for (int b = 0; b < n_blk; ++b) P.band_code[(size_t)P.blk_j[b] * (Bw + 1) + (P.blk_j[b] - P.blk_i[b])] = b;
}

// launch shapes that follow from the sizes alone
inline void plan_shapes(UploadPlan& P, const PlanDecisions& D) {
    const int Nl = P.Nl, No = P.No, Npf = P.Npf;
    // lanes per landmark: smallest power of two >= mean track length, in [4, 64] — but at most 8 once the window has a thousand landmarks:
    // the landmark-major kernels of a 200-key-frame window or of a batch of 50-key-frame windows need more than one round of resident
    // waves at 16 lanes per landmark (k_backsub: 121 VGPRs, four waves per SIMD), and a lane that loops twice over a track of ten costs
    // less than the second round (measured: C4 5 631 -> 6 007 it/s, C4R 5 040 -> 5 330, 16 resident C2 windows 73.0 k -> 80.9 k,
    // 8 windows 63.1 k -> 66.2 k; one C2 window flat: 20.3 k / 20.2 k).  A property of the WINDOW alone: a window's result never
    // depends on what it is batched with.
    int group = 4;
    const double mean_track = Nl > 0 ? (double)No / Nl : 1.0;
    while (group < 64 && group < mean_track) group *= 2;
    if (Nl >= 1024 && group > 8) group = 8;
    { const int gq = D.sw.group; if (gq == 4 || gq == 8 || gq == 16 || gq == 32 || gq == 64) group = gq; }   // tuning override
    P.group = group;
    P.n_lin_a = std::max(1, (Nl + (256 / group) - 1) / (256 / group));
    const int n_eval = (No + 255) / 256 + 1;
    P.n_parts = std::max(P.n_lin_a + 1, n_eval);
    const size_t n6 = (size_t)6 * Npf;
    P.chol_np = std::max<size_t>(32, (n6 + 31) / 32 * 32);
    P.small_fits = Npf >= 1 && n6 <= (size_t)SM_MAX_N6;
    P.n_hist = (size_t)std::max(D.index_blocks, 1) * std::max(Npf, 1);
}

// The whole plan of an upload, after plan_poses and the summary.  false: refused (P.status, P.msg).
inline bool plan_upload(UploadPlan& P, const PlanGraph& G, const GraphSummary& sum, const PlanDecisions& D) {
    P.status = VISFS_BA_OK; P.msg = nullptr;
    P.Nl = G.Nl; P.No = G.No; P.Ne = G.Ne; P.Nz = G.Nz; P.solver = D.solver;
    P.n_pose_obs = sum.cnt[P.Npf]; P.n_edges_ok = sum.n_edges_ok;
    if (!plan_chunks(P, sum.cnt)) return false;
    plan_odo_incidence(P, G);
    if (!plan_blocks(P, G, sum)) return false;
    plan_rows(P);
    plan_runs(P, sum, D.sw);
    plan_schur(P, D);
    if (!plan_pcg(P, D)) return false;
    plan_band(P, D);
    plan_shapes(P, D);
    return true;
}

}  // namespace visfs_ba
