// One scan matched against many frozen grid stacks in one call (include/visfs_scan_group.h).
//
// The launch sequence is that of the single call (ba_scan_fast.hip) with the member as blockIdx.y: every kernel runs the single
// call's body (ba_scan_stack.hpp) on member blockIdx.y's slices of the group's arenas, its levels and limits read from the member
// table.  One call is one upload from a pinned buffer (points, a rotation table per member [m][S][2], the member table), H + 5
// launches for any m, one download (Ctrl[m]) and one stream wait:
//   k_group_cells   grid (S n / 256, m): cells[m][S][n], and every member's Ctrl zeroed;
//   k_group_bounds  grid (x, m): one wavefront per level-H node, striding: bounds[m][S m_H^2];
//   k_group_seeds   grid (S, m): member i's incumbent into Ctrl[i].B through the int32 atomic maximum;
//   k_group_keep    grid (x, m): the level-H nodes with U >= B_i appended to member i's frontier segment;
//   k_group_level   grid (x, m), for h = H .. 1: frontier segments [m][cap] of two working arenas, counters in Ctrl[i]; overflow is
//                   decided per member as in the single kernel;
//   k_group_best    grid (1, m): each member's winner among its level-0 survivors.
// x is the single call's fixed grid divided by m, at least 1; no result depends on it (integer sums, integer atomics, the total order
// of `better`).  The members share nothing but the scan, so member i's bytes are the single call's on that stack.  A group of
// host-twin stacks runs the one-core twin (host_search) per member.
//
// visfs_scan_group_match_refine (include/visfs_scan_refine.h, section 9o) is the same sequence with the members' refinement jobs
// appended to the upload, k_scan_refine (ba_scan_refine.hip) launched after k_group_best with the member as blockIdx.x, reading each
// member's winner from its Ctrl, and the refinement records behind the Ctrl records in the one download.
#include "ba_scan_refine.hpp"
#include "../../include/visfs_scan_group.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>

#pragma clang fp contract(off)

using namespace scanfast;
using scan::Plan;

namespace scanfast {

// what the kernels read of one member
struct Member {
    double gx, gy;                            // the guess
    double res, max_x, max_y;                 // the limits frozen with the grid
    Levels lv;
};

__global__ __launch_bounds__(kThreads) void k_group_cells(const double* __restrict__ pts, const double* __restrict__ rot, const Member* __restrict__ mt,
                                                          int32_t n, int32_t S, int64_t total, int2* __restrict__ cells, Ctrl* __restrict__ ctrl) {
    const int32_t mi = blockIdx.y;
    const Member& M = mt[mi];
    cells_body(pts, rot + (int64_t)mi * 2 * S, n, total, M.gx, M.gy, M.res, M.max_x, M.max_y, cells + (int64_t)mi * total, ctrl + mi);
}

__global__ __launch_bounds__(kThreads) void k_group_bounds(const int2* __restrict__ cells, int64_t ncell, int32_t n, const Member* __restrict__ mt,
                                                           int32_t nl, int32_t H, int32_t mH, int32_t total, int32_t* __restrict__ bounds) {
    const int32_t mi = blockIdx.y;
    const LevelView vH = mt[mi].lv.v[H];
    bounds_body(cells + (int64_t)mi * ncell, n, vH, nl, H, mH, total, bounds + (int64_t)mi * total);
}

__global__ __launch_bounds__(kThreads) void k_group_seeds(const int32_t* __restrict__ bounds, int32_t total, const int2* __restrict__ cells, int64_t ncell,
                                                          int32_t n, const Member* __restrict__ mt, int32_t nl, int32_t L, int32_t H, int32_t mH,
                                                          Ctrl* __restrict__ ctrl) {
    const int32_t mi = blockIdx.y;
    seeds_body(bounds + (int64_t)mi * total, cells + (int64_t)mi * ncell, n, mt[mi].lv, nl, L, H, mH, ctrl + mi);
}

__global__ __launch_bounds__(kThreads) void k_group_keep(const int32_t* __restrict__ bounds, int32_t total, int32_t H, int2* __restrict__ out, int32_t cap,
                                                         Ctrl* __restrict__ ctrl) {
    const int32_t mi = blockIdx.y;
    keep_body(bounds + (int64_t)mi * total, total, H, out + (int64_t)mi * cap, cap, ctrl + mi);
}

__global__ __launch_bounds__(kThreads) void k_group_level(int32_t h, const int2* __restrict__ in, int2* __restrict__ out, int32_t cap,
                                                          const int2* __restrict__ cells, int64_t ncell, int32_t n, const Member* __restrict__ mt,
                                                          int32_t nl, int32_t L, Ctrl* __restrict__ ctrl) {
    const int32_t mi = blockIdx.y;
    const LevelView lo = mt[mi].lv.v[h - 1];
    level_body(h, in + (int64_t)mi * cap, out + (int64_t)mi * cap, cap, cells + (int64_t)mi * ncell, n, lo, nl, L, ctrl + mi);
}

__global__ __launch_bounds__(kThreads) void k_group_best(const int2* __restrict__ in, int32_t cap, Ctrl* __restrict__ ctrl) {
    const int32_t mi = blockIdx.y;
    best_body(in + (int64_t)mi * cap, cap, ctrl + mi);
}

}  // namespace scanfast

// ---------------------------------------------------------------- the group object
struct visfs_scan_group {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    int32_t blocks = 1;                       // the single call's fixed grid, shared among the members
    std::vector<visfs_scan_stack*> mem;
    std::string err;
    // a match on the device: as the single call's buffers, every one an arena over the members; the hook's arenas (bnd[1], fr[2])
    // change hands with the working ones after a call that ran to its end
    char* h_up = nullptr; char* d_up = nullptr; size_t up_cap = 0;
    int2* d_cells = nullptr; size_t cells_cap = 0;
    Ctrl* d_ctrl = nullptr; Ctrl* h_ctrl = nullptr;   // [m], and behind them the refinement records [m]
    // match_refine: the traces [m][kMaxTrials][kTraceItems] of the call in work ([0]) and of the hook ([1]); the twin's traces; the
    // trials per member of the last call that ran to its end
    double* d_rtrace[2] = { nullptr, nullptr };
    std::vector<std::vector<double>> h_rtrace;
    std::vector<int32_t> rtrials;
    Bounds bnd[2];
    Frontier fr[3];
    // the last call that ran to its end, per member (have = false: its status was not OK); the strides of the hook's arenas
    std::vector<Last> last;
    int64_t last_top = 0, last_cap = 0;
    int32_t launches = 0, copies = 0, syncs = 0;
};

namespace {

thread_local std::string t_create_err;

int gfail(visfs_scan_group* g, int rc, const std::string& why) { g->err = why; return rc; }

#define SG_HIP(g, expr)                                                                                               \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return gfail((g), VISFS_BA_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

template <class T> int grow(visfs_scan_group* g, T** p, size_t* cap, size_t need) {
    if (*cap >= need) return VISFS_BA_OK;
    if (*p) SG_HIP(g, hipFree(*p));
    *p = nullptr; *cap = 0;
    SG_HIP(g, hipMalloc(reinterpret_cast<void**>(p), need * sizeof(T)));
    *cap = need;
    return VISFS_BA_OK;
}

void group_free(visfs_scan_group* g) {
    if (g->device) {
        (void)hipSetDevice(g->dev);
        if (g->stream) (void)hipStreamSynchronize(g->stream);
        if (g->h_up) (void)hipHostFree(g->h_up);
        if (g->d_up) (void)hipFree(g->d_up);
        if (g->d_cells) (void)hipFree(g->d_cells);
        if (g->d_ctrl) (void)hipFree(g->d_ctrl);
        if (g->h_ctrl) (void)hipHostFree(g->h_ctrl);
        for (double* p : g->d_rtrace) if (p) (void)hipFree(p);
        for (Bounds& b : g->bnd) if (b.p) (void)hipFree(b.p);
        for (Frontier& f : g->fr) if (f.p) (void)hipFree(f.p);
    }
    delete g;
}

std::string member_text(int32_t i, const std::string& why) { return "member " + std::to_string(i) + ": " + why; }

size_t ctrl_bytes(int32_t m) { return (size_t)m * sizeof(Ctrl); }
size_t record_bytes(int32_t m) { return (size_t)m * sizeof(visfs_scan_refine_result); }
visfs_scan_refine_result* records_of(Ctrl* c, int32_t m) { return reinterpret_cast<visfs_scan_refine_result*>(reinterpret_cast<char*>(c) + ctrl_bytes(m)); }

// member i's refinement job of a match_refine call: the start is formed on the device from the member's Ctrl
scanrefine::Job match_job(const visfs_scan_stack* st, const Search& s, double min_score, const Ctrl* ctrl, const double* rot) {
    const double zero[3] = { 0.0, 0.0, 0.0 };
    scanrefine::Job J = scanrefine::stack_job(st, zero, zero);
    J.from_match = 1; J.na = s.P.na; J.nl = s.P.nl; J.S = s.P.S;
    J.gx = s.P.gx; J.gy = s.P.gy; J.gyaw = s.P.gyaw; J.step = s.P.step; J.min_score = min_score;
    J.ctrl = ctrl; J.rot = rot;
    return J;
}

// Every member's search on the device: fills the Ctrl records of h_ctrl and leaves the frontier of level 0 in fr[*cur].  With `rp`
// every matched member's refinement follows in the same sequence: its records come behind the Ctrl records.
int device_run(visfs_scan_group* g, const std::vector<Search>& ss, int* cur_out, const scanrefine::Prm* rp = nullptr, double min_score = 0.0) {
    const int32_t m = (int32_t)g->mem.size();
    const Search& s0 = ss[0];
    const int32_t n = s0.P.n, S = s0.P.S, nl = s0.P.nl, L = s0.P.Lw, H = s0.H, mH = s0.mH, total = s0.top(), cap = s0.cap;
    const int64_t ncell = (int64_t)S * n;
    SG_HIP(g, hipSetDevice(g->dev));
    const size_t npts = 2 * (size_t)n, nrot = 2 * (size_t)S * m;
    const size_t match_bytes = (npts + nrot) * sizeof(double) + (size_t)m * sizeof(Member);
    const size_t bytes = match_bytes + (rp ? (size_t)m * sizeof(scanrefine::Job) : 0);
    if (g->up_cap < bytes) {
        if (g->h_up) SG_HIP(g, hipHostFree(g->h_up));
        if (g->d_up) SG_HIP(g, hipFree(g->d_up));
        g->h_up = g->d_up = nullptr; g->up_cap = 0;
        const size_t want = bytes + bytes / 2;
        SG_HIP(g, hipHostMalloc(reinterpret_cast<void**>(&g->h_up), want, hipHostMallocDefault));
        SG_HIP(g, hipMalloc(reinterpret_cast<void**>(&g->d_up), want));
        g->up_cap = want;
    }
    if (!g->d_ctrl) {
        SG_HIP(g, hipMalloc(reinterpret_cast<void**>(&g->d_ctrl), ctrl_bytes(m) + record_bytes(m)));
        SG_HIP(g, hipHostMalloc(reinterpret_cast<void**>(&g->h_ctrl), ctrl_bytes(m) + record_bytes(m), hipHostMallocDefault));
    }
    if (rp)
        for (double*& p : g->d_rtrace)
            if (!p) SG_HIP(g, hipMalloc(reinterpret_cast<void**>(&p), (size_t)m * scanrefine::kMaxTrials * scanrefine::kTraceItems * sizeof(double)));
    int rc;
    if ((rc = grow(g, &g->d_cells, &g->cells_cap, (size_t)m * (size_t)ncell)) != VISFS_BA_OK) return rc;
    if ((rc = grow(g, &g->bnd[0].p, &g->bnd[0].cap, (size_t)m * (size_t)total)) != VISFS_BA_OK) return rc;
    for (int f = 0; f < 2; ++f)
        if ((rc = grow(g, &g->fr[f].p, &g->fr[f].cap, (size_t)m * (size_t)cap)) != VISFS_BA_OK) return rc;
    double* hup = reinterpret_cast<double*>(g->h_up);
    std::memcpy(hup, s0.P.pts.data(), npts * sizeof(double));
    Member* hmt = reinterpret_cast<Member*>(hup + npts + nrot);                // doubles in front of it: aligned to 8
    for (int32_t i = 0; i < m; ++i) {
        const Plan& P = ss[i].P;
        std::memcpy(hup + npts + 2 * (size_t)S * i, P.rot.data(), 2 * (size_t)S * sizeof(double));
        Member M;
        M.gx = P.gx; M.gy = P.gy; M.res = P.L.res; M.max_x = P.L.max_x; M.max_y = P.L.max_y; M.lv = g->mem[i]->lv;
        std::memcpy(hmt + i, &M, sizeof M);
    }
    if (rp) {                                                              // the jobs point into the device's copies
        const double* drot0 = reinterpret_cast<const double*>(g->d_up) + npts;
        for (int32_t i = 0; i < m; ++i) {
            const scanrefine::Job J = match_job(g->mem[i], ss[i], min_score, g->d_ctrl + i, drot0 + 2 * (size_t)S * i);
            std::memcpy(g->h_up + match_bytes + (size_t)i * sizeof J, &J, sizeof J);
        }
    }
    SG_HIP(g, hipMemcpyAsync(g->d_up, g->h_up, bytes, hipMemcpyHostToDevice, g->stream));
    ++g->copies;
    const double* d = reinterpret_cast<const double*>(g->d_up);
    const double* drot = d + npts;
    const Member* dmt = reinterpret_cast<const Member*>(drot + nrot);
    const dim3 fixed((unsigned)std::max(1, g->blocks / m), (unsigned)m), wg(kThreads);
    hipLaunchKernelGGL(k_group_cells, dim3(blocks_for(ncell), (unsigned)m), wg, 0, g->stream, d, drot, dmt, n, S, ncell, g->d_cells, g->d_ctrl);
    SG_HIP(g, hipGetLastError()); ++g->launches;
    hipLaunchKernelGGL(k_group_bounds, fixed, wg, 0, g->stream, g->d_cells, ncell, n, dmt, nl, H, mH, total, g->bnd[0].p);
    SG_HIP(g, hipGetLastError()); ++g->launches;
    hipLaunchKernelGGL(k_group_seeds, dim3((unsigned)S, (unsigned)m), wg, 0, g->stream, g->bnd[0].p, total, g->d_cells, ncell, n, dmt, nl, L, H, mH, g->d_ctrl);
    SG_HIP(g, hipGetLastError()); ++g->launches;
    int cur = 0;                                                           // the frontiers of the level in work: fr[cur]
    hipLaunchKernelGGL(k_group_keep, fixed, wg, 0, g->stream, g->bnd[0].p, total, H, g->fr[cur].p, cap, g->d_ctrl);
    SG_HIP(g, hipGetLastError()); ++g->launches;
    for (int32_t h = H; h >= 1; --h) {
        hipLaunchKernelGGL(k_group_level, fixed, wg, 0, g->stream, h, g->fr[cur].p, g->fr[1 - cur].p, cap, g->d_cells, ncell, n, dmt, nl, L, g->d_ctrl);
        SG_HIP(g, hipGetLastError()); ++g->launches;
        cur = 1 - cur;
    }
    hipLaunchKernelGGL(k_group_best, dim3(1, (unsigned)m), wg, 0, g->stream, g->fr[cur].p, cap, g->d_ctrl);
    SG_HIP(g, hipGetLastError()); ++g->launches;
    if (rp) {
        SG_HIP(g, (hipError_t)scanrefine::launch_refine(g->stream, m, reinterpret_cast<const scanrefine::Job*>(g->d_up + match_bytes), *rp, d,
                                                        records_of(g->d_ctrl, m), g->d_rtrace[0]));
        ++g->launches;
    }
    SG_HIP(g, hipMemcpyAsync(g->h_ctrl, g->d_ctrl, ctrl_bytes(m) + (rp ? record_bytes(m) : 0), hipMemcpyDeviceToHost, g->stream));
    ++g->copies;
    SG_HIP(g, hipStreamSynchronize(g->stream));
    ++g->syncs;
    *cur_out = cur;
    return VISFS_BA_OK;
}

// rp and refined: both or neither (visfs_scan_group_match_refine)
int group_match(visfs_scan_group* g, const visfs_scan_stack_params& p, const double* guesses, int32_t n, const double* xyz,
                visfs_scan_stack_result* results, int32_t* status, int32_t* best_member, const visfs_scan_refine_params* rp = nullptr,
                visfs_scan_refine_result* refined = nullptr) {
    const int32_t m = (int32_t)g->mem.size();
    const char* why = "";
    int rc;
    for (int32_t i = 0; i < m; ++i)
        if ((rc = check_call(p, guesses + 3 * i, n, xyz, &why)) != VISFS_BA_OK) return gfail(g, rc, member_text(i, why));
    if (rp)
        for (int32_t i = 0; i < m; ++i)
            if ((rc = scanrefine::check_call(*rp, guesses + 3 * i, guesses + 3 * i, n, xyz, &why)) != VISFS_BA_OK) return gfail(g, rc, member_text(i, why));
    if ((int64_t)m * p.frontier_capacity > (int64_t)VISFS_SCAN_GROUP_MAX_FRONTIER)
        return gfail(g, VISFS_BA_ERR_UNSUPPORTED, "members times frontier_capacity exceed 2^26");
    if (n == 0) {                                                          // nothing to match: every guess back
        g->launches = g->copies = g->syncs = 0;
        for (int32_t i = 0; i < m; ++i) { no_points(guesses + 3 * i, results + i); status[i] = VISFS_BA_OK; }
        if (rp) {
            for (int32_t i = 0; i < m; ++i) scanrefine::not_refined(VISFS_BA_OK, guesses[3 * i], guesses[3 * i + 1], guesses[3 * i + 2], refined + i);
            g->rtrials.assign((size_t)m, 0);
        }
        *best_member = -1;
        g->err.clear();
        return VISFS_BA_OK;
    }
    std::vector<Search> ss((size_t)m);
    for (int32_t i = 0; i < m; ++i) {
        if ((rc = make_search(g->mem[i], p, guesses + 3 * i, n, xyz, ss[i], &why)) != VISFS_BA_OK) return gfail(g, rc, member_text(i, why));
        // equal resolution and depth: one S, nl, H and m_H for all, which the launches rely on
        if (ss[i].P.S != ss[0].P.S || ss[i].P.nl != ss[0].P.nl || ss[i].H != ss[0].H || ss[i].mH != ss[0].mH)
            return gfail(g, VISFS_BA_ERR_DEVICE, member_text(i, "its search differs in shape from member 0's"));
    }
    g->launches = g->copies = g->syncs = 0;
    std::vector<Last> now((size_t)m);
    std::string first_overflow;
    int cur = 0;
    scanrefine::Prm RP;
    if (rp) RP = scanrefine::make_prm(*rp, n);
    if (g->device) {
        if ((rc = device_run(g, ss, &cur, rp ? &RP : nullptr, p.min_score)) != VISFS_BA_OK) return rc;
        for (int32_t i = 0; i < m; ++i) {
            const Ctrl& c = g->h_ctrl[i];
            const Search& s = ss[i];
            if (c.overflow) {
                if (first_overflow.empty()) first_overflow = member_text(i, overflow_text(c.overflow - 1, s.cap));
                continue;
            }
            if (c.best_index < 0 || (int64_t)c.best_index >= s.P.candidates()) return gfail(g, VISFS_BA_ERR_DEVICE, member_text(i, "the search returned no candidate"));
            Last& l = now[i];
            l.have = true; l.S = s.P.S; l.L = s.P.Lw; l.n = n; l.H = s.H; l.mH = s.mH; l.survivors = c.kept[0]; l.c = c;
        }
        // the hook's arenas change hands: what this call wrote stays until the next call that runs to its end
        std::swap(g->bnd[0], g->bnd[1]);
        std::swap(g->fr[cur], g->fr[2]);
    } else {
        for (int32_t i = 0; i < m; ++i) {
            std::string text;
            rc = host_search(g->mem[i]->lv, ss[i], now[i], text);
            if (rc == VISFS_BA_ERR_UNSUPPORTED) {
                now[i] = Last();
                if (first_overflow.empty()) first_overflow = member_text(i, text);
            } else if (rc != VISFS_BA_OK) return gfail(g, rc, member_text(i, text));
        }
    }
    int32_t best = -1, best_sum = -1;
    for (int32_t i = 0; i < m; ++i) {
        if (!now[i].have) { status[i] = VISFS_BA_ERR_UNSUPPORTED; continue; }
        status[i] = VISFS_BA_OK;
        finish(ss[i], p, now[i].c.best_index, now[i].c.best_sum, results + i);
        if (results[i].match.matched && results[i].match.sum > best_sum) { best = i; best_sum = results[i].match.sum; }
    }
    *best_member = best;
    if (rp) {
        // a member that overflowed or stayed below min_score is not refined; the others from their winner towards their guess
        std::vector<std::vector<double>> traces;
        std::vector<int32_t> trials((size_t)m, 0);
        if (!g->device) traces.resize((size_t)m);
        for (int32_t i = 0; i < m; ++i) {
            const double* gi = guesses + 3 * i;
            if (status[i] != VISFS_BA_OK) { scanrefine::not_refined(status[i], gi[0], gi[1], gi[2], refined + i); continue; }
            const visfs_scan_match_result& w = results[i].match;
            if (!w.matched) { scanrefine::not_refined(VISFS_BA_OK, w.x, w.y, w.yaw, refined + i); continue; }
            if (g->device) {
                refined[i] = records_of(g->h_ctrl, m)[i];
                if (!refined[i].refined) return gfail(g, VISFS_BA_ERR_DEVICE, member_text(i, "the refinement skipped a matched member"));
            } else {
                const double start[3] = { w.x, w.y, w.yaw };
                traces[i].assign((size_t)scanrefine::kMaxTrials * scanrefine::kTraceItems, 0.0);
                scanrefine::host_refine(scanrefine::stack_job(g->mem[i], start, gi), RP, ss[i].P.pts.data(), refined + i, traces[i].data());
            }
            trials[i] = refined[i].trials;
        }
        if (g->device) std::swap(g->d_rtrace[0], g->d_rtrace[1]);
        g->h_rtrace.swap(traces);
        g->rtrials.swap(trials);
    }
    g->last = std::move(now);
    g->last_top = ss[0].top(); g->last_cap = ss[0].cap;
    g->err = first_overflow;
    return VISFS_BA_OK;
}

template <class F> int guarded(F&& f) noexcept {
    try { return f(); }
    catch (...) { return (int)VISFS_BA_ERR_DEVICE; }
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_scan_group_abi_version(void) { return VISFS_SCAN_GROUP_ABI_VERSION; }

int visfs_scan_group_create(int32_t m, visfs_scan_stack* const* members, visfs_scan_group** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded([&]() -> int {
        auto bad = [&](int rc, const std::string& why) { t_create_err = why; return rc; };
        if (m < 1 || m > VISFS_SCAN_GROUP_MAX) return bad(VISFS_BA_ERR_UNSUPPORTED, "a group holds 1 to 64 members");
        if (!members) return bad(VISFS_BA_ERR_BAD_ARGUMENT, "no members");
        for (int32_t i = 0; i < m; ++i) {
            const visfs_scan_stack* a = members[i];
            const visfs_scan_stack* f = members[0];
            if (!a) return bad(VISFS_BA_ERR_BAD_ARGUMENT, member_text(i, "null stack"));
            if (a->device != f->device) return bad(VISFS_BA_ERR_BAD_ARGUMENT, member_text(i, "device and host-twin stacks in one group"));
            if (a->device && (a->dev != f->dev || a->stream != f->stream)) return bad(VISFS_BA_ERR_BAD_ARGUMENT, member_text(i, "a stack of another handle"));
            if (std::memcmp(&a->L.res, &f->L.res, sizeof(double)) != 0) return bad(VISFS_BA_ERR_BAD_ARGUMENT, member_text(i, "its resolution differs from member 0's"));
            if (a->depth != f->depth) return bad(VISFS_BA_ERR_BAD_ARGUMENT, member_text(i, "its depth differs from member 0's"));
        }
        visfs_scan_group* g = new visfs_scan_group();
        g->mem.assign(members, members + m);
        g->last.resize((size_t)m);
        const visfs_scan_stack* f = members[0];
        g->device = f->device; g->dev = f->dev; g->stream = f->stream; g->blocks = f->blocks;
        *out = g;
        return (int)VISFS_BA_OK;
    });
}

void visfs_scan_group_destroy(visfs_scan_group* g) { if (g) group_free(g); }

const char* visfs_scan_group_last_error(const visfs_scan_group* g) { return g ? g->err.c_str() : t_create_err.c_str(); }

int visfs_scan_group_match(visfs_scan_group* g, const visfs_scan_stack_params* p, const double* guesses, int32_t n, const double* xyz,
                           visfs_scan_stack_result* results, int32_t* status, int32_t* best_member) {
    if (!g || !p || !guesses || !results || !status || !best_member || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded([&]() -> int { return group_match(g, *p, guesses, n, xyz, results, status, best_member); });
}

int visfs_scan_group_match_download(visfs_scan_group* g, int32_t member, int32_t header[8], int32_t scored[16], int32_t kept[16],
                                    int64_t bounds_cap, int32_t* bounds, int64_t survivors_cap, int32_t* survivors) {
    if (!g || !header || bounds_cap < 0 || survivors_cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded([&]() -> int {
        if (member < 0 || member >= (int32_t)g->mem.size()) return gfail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the group has no such member");
        const Last& l = g->last[(size_t)member];
        std::memset(header, 0, 8 * sizeof(int32_t));
        if (!l.have) return (int)VISFS_BA_OK;
        const int32_t per = l.mH * l.mH;
        const int64_t nb = (int64_t)l.S * per;
        header[0] = l.S; header[1] = l.L; header[2] = l.n; header[3] = l.H; header[4] = per; header[5] = l.survivors; header[6] = l.c.B;
        if (scored) std::memcpy(scored, l.c.scored, sizeof l.c.scored);
        if (kept) std::memcpy(kept, l.c.kept, sizeof l.c.kept);
        if ((bounds && bounds_cap < nb) || (survivors && survivors_cap < l.survivors)) return gfail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the hook's arrays are too small");
        if (!g->device) {
            if (bounds) std::memcpy(bounds, l.bounds.data(), (size_t)nb * sizeof(int32_t));
            if (survivors) std::memcpy(survivors, l.surv.data(), (size_t)l.survivors * sizeof(int2));
            return (int)VISFS_BA_OK;
        }
        SG_HIP(g, hipSetDevice(g->dev));
        if (bounds) SG_HIP(g, hipMemcpyAsync(bounds, g->bnd[1].p + (int64_t)member * g->last_top, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
        if (survivors) SG_HIP(g, hipMemcpyAsync(survivors, g->fr[2].p + (int64_t)member * g->last_cap, (size_t)l.survivors * sizeof(int2), hipMemcpyDeviceToHost, g->stream));
        SG_HIP(g, hipStreamSynchronize(g->stream));
        if (survivors) {                                                   // the device appends unordered
            int2* sv = reinterpret_cast<int2*>(survivors);
            std::sort(sv, sv + l.survivors, [](const int2& a, const int2& b) { return a.x < b.x; });
        }
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_group_match_refine(visfs_scan_group* g, const visfs_scan_stack_params* mp, const visfs_scan_refine_params* rp, const double* guesses,
                                  int32_t n, const double* xyz, visfs_scan_stack_result* results, int32_t* status, int32_t* best_member,
                                  visfs_scan_refine_result* refined) {
    if (!g || !mp || !rp || !guesses || !results || !status || !best_member || !refined || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded([&]() -> int { return group_match(g, *mp, guesses, n, xyz, results, status, best_member, rp, refined); });
}

int visfs_scan_group_refine_download(visfs_scan_group* g, int32_t member, int32_t cap, double* trace, int32_t* trials) {
    if (!g || !trials || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded([&]() -> int {
        if (member < 0 || member >= (int32_t)g->mem.size()) return gfail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the group has no such member");
        const int32_t nt = (size_t)member < g->rtrials.size() ? g->rtrials[(size_t)member] : 0;
        *trials = nt;
        if (!trace || nt == 0) return (int)VISFS_BA_OK;
        if (cap < nt) return gfail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the hook's array is too small");
        const size_t bytes = (size_t)nt * scanrefine::kTraceItems * sizeof(double);
        if (!g->device) { std::memcpy(trace, g->h_rtrace[(size_t)member].data(), bytes); return (int)VISFS_BA_OK; }
        SG_HIP(g, hipSetDevice(g->dev));
        SG_HIP(g, hipMemcpyAsync(trace, g->d_rtrace[1] + (size_t)member * scanrefine::kMaxTrials * scanrefine::kTraceItems, bytes, hipMemcpyDeviceToHost, g->stream));
        SG_HIP(g, hipStreamSynchronize(g->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_group_last_counts(const visfs_scan_group* g, int32_t* kernel_launches, int32_t* copies_and_memsets, int32_t* synchronisations) {
    if (!g) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (kernel_launches) *kernel_launches = g->launches;
    if (copies_and_memsets) *copies_and_memsets = g->copies;
    if (synchronisations) *synchronisations = g->syncs;
    return VISFS_BA_OK;
}

}  // extern "C"
