// One scan matched against many frozen grid stacks in one call (include/visfs_scan_group.h).
//
// This file holds the one device call path of the stack matcher: the match kernels and their launch sequence device_run, which
// the single call (visfs_scan_stack_match, ba_scan_fast.hip) runs with m = 1 on the stack's call block and the group call with its m
// members on the group's.  The member is blockIdx.y: every kernel runs one search's body (ba_scan_stack.hpp) on member blockIdx.y's
// slices of the block's arenas, its levels and limits read from the member table.  One call is one upload from a pinned buffer
// (points, a rotation table per member [m][S][2], the member table), H + 5 launches for any m, one download (Ctrl[m]) and one stream
// wait; nothing is read back between levels, the frontier counts live in the Ctrl records on the device:
//   k_group_cells   grid (S n / 256, m): the discretised cells[m][S][n] (scan::discretise), and every member's Ctrl zeroed;
//   k_group_bounds  grid (x, m): one wavefront per level-H node, lanes along the points, striding: bounds[m][S m_H^2];
//   k_group_seeds   grid (S, m): one workgroup per scan: its best level-H node, then H greedy steps, its four wavefronts scoring the
//                   four children of a step; the leaf's sum joins member i's incumbent Ctrl[i].B through the int32 atomic maximum;
//   k_group_keep    grid (x, m): the level-H nodes with U >= B_i appended to member i's frontier segment;
//   k_group_level   grid (x, m), for h = H .. 1: a fixed grid of wavefronts strides over member i's frontier of level h (its length
//                   read on the device), scores the up-to-four in-window children of a node from one pass over the scan's cells, and
//                   appends those with U >= B_i to its frontier of level h - 1 through an integer atomic counter in Ctrl[i]; frontier
//                   segments [m][cap] of two working arenas; entries beyond the capacity are dropped and the member's overflow flag
//                   is raised;
//   k_group_best    grid (1, m): one workgroup per member selects its winner among its level-0 survivors: Q descending, index
//                   ascending.
// x is the stack's fixed grid divided by m, at least 1; no result depends on it (integer sums, integer atomics, the total order of
// `better`).  The members share nothing but the scan, so member i's bytes are those of a single call on that stack.  The two callers
// differ in what they make of the records: the single call fails on an overflow and hands the hook's arenas over only after a good
// call; the group reports an overflow in that member's status and hands over after every call that ran to its end.  A group of
// host-twin stacks runs the one-core twin (host_search) per member.
//
// visfs_scan_group_match_refine (include/visfs_scan_refine.h, section 9o) is the same sequence with the members' refinement jobs
// appended to the upload, k_scan_refine (ba_scan_refine.hip) launched after k_group_best with the member as blockIdx.x, reading each
// member's winner from its Ctrl, and the refinement records behind the Ctrl records in the one download.
#include "ba_scan_refine.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_scan_group.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>

#pragma clang fp contract(off)

using namespace scanfast;
using namespace host;
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
    int32_t blocks = 1;                       // member 0's fixed grid, shared among the members
    std::vector<visfs_scan_stack*> mem;
    std::string err;
    // a match on the device: a block for the m members; the hook's arenas change hands after every call that ran to its end
    CallBlock blk;
    // match_refine: the traces [m][kMaxTrials][kTraceItems] of the call in work ([0]) and of the hook ([1]); the twin's traces; the
    // trials per member of the last call that ran to its end
    DeviceBuf<double> d_rtrace[2];
    std::vector<std::vector<double>> h_rtrace;
    std::vector<int32_t> rtrials;
    // the last call that ran to its end, per member (have = false: its status was not OK)
    std::vector<Last> last;

    ~visfs_scan_group() {                     // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

thread_local std::string t_create_err;


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

}  // namespace

// ---------------------------------------------------------------- the launch sequence (ba_scan_stack.hpp)
int scanfast::device_run(CallBlock& b, int dev, hipStream_t stream, int32_t blocks, int32_t m, visfs_scan_stack* const* mem, const Search* ss, int* cur_out,
                         std::string& why, const scanrefine::Prm* rp, double min_score, double* rtrace) {
    const Search& s0 = ss[0];
    const int32_t n = s0.P.n, S = s0.P.S, nl = s0.P.nl, L = s0.P.Lw, H = s0.H, mH = s0.mH, total = s0.top(), cap = s0.cap;
    const int64_t ncell = (int64_t)S * n;
    b.counts = {};
    HIP_TRY(&why, hipSetDevice(dev));
    const size_t npts = 2 * (size_t)n, nrot = 2 * (size_t)S * m;
    const size_t match_bytes = (npts + nrot) * sizeof(double) + (size_t)m * sizeof(Member);
    const size_t bytes = match_bytes + (rp ? (size_t)m * sizeof(scanrefine::Job) : 0);
    RC_TRY(b.up.reserve(&why, bytes, bytes + bytes / 2));
    if (!b.ctrl_d() || !b.h_ctrl) {
        RC_TRY(b.d_ctrl.alloc(&why, ctrl_bytes(m) + record_bytes(m)));
        RC_TRY(b.h_ctrl.alloc(&why, ctrl_bytes(m) + record_bytes(m)));
    }
    RC_TRY(b.d_cells.grow(&why, (size_t)m * (size_t)ncell));
    RC_TRY(b.bnd[0].grow(&why, (size_t)m * (size_t)total));
    for (int f = 0; f < 2; ++f) RC_TRY(b.fr[f].grow(&why, (size_t)m * (size_t)cap));
    double* hup = reinterpret_cast<double*>(b.up.h.get());
    std::memcpy(hup, s0.P.pts.data(), npts * sizeof(double));
    Member* hmt = reinterpret_cast<Member*>(hup + npts + nrot);                // doubles in front of it: aligned to 8
    for (int32_t i = 0; i < m; ++i) {
        const Plan& P = ss[i].P;
        std::memcpy(hup + npts + 2 * (size_t)S * i, P.rot.data(), 2 * (size_t)S * sizeof(double));
        Member M;
        M.gx = P.gx; M.gy = P.gy; M.res = P.L.res; M.max_x = P.L.max_x; M.max_y = P.L.max_y; M.lv = mem[i]->lv;
        std::memcpy(hmt + i, &M, sizeof M);
    }
    if (rp) {                                                              // the jobs point into the device's copies
        const double* drot0 = reinterpret_cast<const double*>(b.up.d.get()) + npts;
        for (int32_t i = 0; i < m; ++i) {
            const scanrefine::Job J = match_job(mem[i], ss[i], min_score, b.ctrl_d() + i, drot0 + 2 * (size_t)S * i);
            std::memcpy(b.up.h.get() + match_bytes + (size_t)i * sizeof J, &J, sizeof J);
        }
    }
    HIP_TRY(&why, hipMemcpyAsync(b.up.d.get(), b.up.h.get(), bytes, hipMemcpyHostToDevice, stream));
    ++b.counts.copies;
    const double* d = reinterpret_cast<const double*>(b.up.d.get());
    const double* drot = d + npts;
    const Member* dmt = reinterpret_cast<const Member*>(drot + nrot);
    const dim3 fixed((unsigned)std::max(1, blocks / m), (unsigned)m), wg(kThreads);
    hipLaunchKernelGGL(k_group_cells, dim3(blocks_for(ncell, kThreads), (unsigned)m), wg, 0, stream, d, drot, dmt, n, S, ncell, b.d_cells.get(), b.ctrl_d());
    HIP_TRY(&why, hipGetLastError()); ++b.counts.launches;
    hipLaunchKernelGGL(k_group_bounds, fixed, wg, 0, stream, b.d_cells.get(), ncell, n, dmt, nl, H, mH, total, b.bnd[0].get());
    HIP_TRY(&why, hipGetLastError()); ++b.counts.launches;
    hipLaunchKernelGGL(k_group_seeds, dim3((unsigned)S, (unsigned)m), wg, 0, stream, b.bnd[0].get(), total, b.d_cells.get(), ncell, n, dmt, nl, L, H, mH, b.ctrl_d());
    HIP_TRY(&why, hipGetLastError()); ++b.counts.launches;
    int cur = 0;                                                           // the frontiers of the level in work: fr[cur]
    hipLaunchKernelGGL(k_group_keep, fixed, wg, 0, stream, b.bnd[0].get(), total, H, b.fr[cur].get(), cap, b.ctrl_d());
    HIP_TRY(&why, hipGetLastError()); ++b.counts.launches;
    for (int32_t h = H; h >= 1; --h) {
        hipLaunchKernelGGL(k_group_level, fixed, wg, 0, stream, h, b.fr[cur].get(), b.fr[1 - cur].get(), cap, b.d_cells.get(), ncell, n, dmt, nl, L, b.ctrl_d());
        HIP_TRY(&why, hipGetLastError()); ++b.counts.launches;
        cur = 1 - cur;
    }
    hipLaunchKernelGGL(k_group_best, dim3(1, (unsigned)m), wg, 0, stream, b.fr[cur].get(), cap, b.ctrl_d());
    HIP_TRY(&why, hipGetLastError()); ++b.counts.launches;
    if (rp) {
        HIP_TRY(&why, (hipError_t)scanrefine::launch_refine(stream, m, reinterpret_cast<const scanrefine::Job*>(b.up.d.get() + match_bytes), *rp, d,
                                                            records_of(b.ctrl_d(), m), rtrace));
        ++b.counts.launches;
    }
    HIP_TRY(&why, hipMemcpyAsync(b.h_ctrl.get(), b.d_ctrl.get(), ctrl_bytes(m) + (rp ? record_bytes(m) : 0), hipMemcpyDeviceToHost, stream));
    ++b.counts.copies;
    HIP_TRY(&why, hipStreamSynchronize(stream));
    ++b.counts.waits;
    *cur_out = cur;
    return VISFS_BA_OK;
}

namespace {

// rp and refined: both or neither (visfs_scan_group_match_refine)
int group_match(visfs_scan_group* g, const visfs_scan_stack_params& p, const double* guesses, int32_t n, const double* xyz,
                visfs_scan_stack_result* results, int32_t* status, int32_t* best_member, const visfs_scan_refine_params* rp = nullptr,
                visfs_scan_refine_result* refined = nullptr) {
    const int32_t m = (int32_t)g->mem.size();
    const char* why = "";
    int rc;
    for (int32_t i = 0; i < m; ++i)
        if ((rc = check_call(p, guesses + 3 * i, n, xyz, &why)) != VISFS_BA_OK) return fail(g, rc, member_text(i, why));
    if (rp)
        for (int32_t i = 0; i < m; ++i)
            if ((rc = scanrefine::check_call(*rp, guesses + 3 * i, guesses + 3 * i, n, xyz, &why)) != VISFS_BA_OK) return fail(g, rc, member_text(i, why));
    if ((int64_t)m * p.frontier_capacity > (int64_t)VISFS_SCAN_GROUP_MAX_FRONTIER)
        return fail(g, VISFS_BA_ERR_UNSUPPORTED, "members times frontier_capacity exceed 2^26");
    if (n == 0) {                                                          // nothing to match: every guess back
        g->blk.counts = {};
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
        if ((rc = make_search(g->mem[i], p, guesses + 3 * i, n, xyz, ss[i], &why)) != VISFS_BA_OK) return fail(g, rc, member_text(i, why));
        // equal resolution and depth: one S, nl, H and m_H for all, which the launches rely on
        if (ss[i].P.S != ss[0].P.S || ss[i].P.nl != ss[0].P.nl || ss[i].H != ss[0].H || ss[i].mH != ss[0].mH)
            return fail(g, VISFS_BA_ERR_DEVICE, member_text(i, "its search differs in shape from member 0's"));
    }
    g->blk.counts = {};
    std::vector<Last> now((size_t)m);
    std::string first_overflow;
    int cur = 0;
    scanrefine::Prm RP;
    if (rp) RP = scanrefine::make_prm(*rp, n);
    if (g->device) {
        if (rp) {
            HIP_TRY(&g->err, hipSetDevice(g->dev));
            for (DeviceBuf<double>& t : g->d_rtrace)
                if (!t) RC_TRY(t.alloc(&g->err, (size_t)m * scanrefine::kMaxTrials * scanrefine::kTraceItems));
        }
        if ((rc = device_run(g->blk, g->dev, g->stream, g->blocks, m, g->mem.data(), ss.data(), &cur, g->err, rp ? &RP : nullptr, p.min_score,
                             g->d_rtrace[0].get())) != VISFS_BA_OK)
            return rc;
        for (int32_t i = 0; i < m; ++i) {
            const Ctrl& c = g->blk.ctrl_h()[i];
            const Search& s = ss[i];
            if (c.overflow) {
                if (first_overflow.empty()) first_overflow = member_text(i, overflow_text(c.overflow - 1, s.cap));
                continue;
            }
            if (c.best_index < 0 || (int64_t)c.best_index >= s.P.candidates()) return fail(g, VISFS_BA_ERR_DEVICE, member_text(i, "the search returned no candidate"));
            now[i] = device_last(s, c);
        }
        g->blk.hand_over(cur, ss[0]);                                      // after any call that ran to its end
    } else {
        for (int32_t i = 0; i < m; ++i) {
            std::string text;
            rc = host_search(g->mem[i]->lv, ss[i], now[i], text);
            if (rc == VISFS_BA_ERR_UNSUPPORTED) {
                now[i] = Last();
                if (first_overflow.empty()) first_overflow = member_text(i, text);
            } else if (rc != VISFS_BA_OK) return fail(g, rc, member_text(i, text));
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
                refined[i] = records_of(g->blk.ctrl_h(), m)[i];
                if (!refined[i].refined) return fail(g, VISFS_BA_ERR_DEVICE, member_text(i, "the refinement skipped a matched member"));
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
    g->err = first_overflow;
    return VISFS_BA_OK;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_scan_group_abi_version(void) { return VISFS_SCAN_GROUP_ABI_VERSION; }

int visfs_scan_group_create(int32_t m, visfs_scan_stack* const* members, visfs_scan_group** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
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

void visfs_scan_group_destroy(visfs_scan_group* g) { delete g; }

const char* visfs_scan_group_last_error(const visfs_scan_group* g) { return g ? g->err.c_str() : t_create_err.c_str(); }

int visfs_scan_group_match(visfs_scan_group* g, const visfs_scan_stack_params* p, const double* guesses, int32_t n, const double* xyz,
                           visfs_scan_stack_result* results, int32_t* status, int32_t* best_member) {
    if (!g || !p || !guesses || !results || !status || !best_member || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(g, [&]() -> int { return group_match(g, *p, guesses, n, xyz, results, status, best_member); });
}

int visfs_scan_group_match_download(visfs_scan_group* g, int32_t member, int32_t header[8], int32_t scored[16], int32_t kept[16],
                                    int64_t bounds_cap, int32_t* bounds, int64_t survivors_cap, int32_t* survivors) {
    if (!g || !header || bounds_cap < 0 || survivors_cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(g, [&]() -> int {
        if (member < 0 || member >= (int32_t)g->mem.size()) return fail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the group has no such member");
        return match_download(g->device, g->dev, g->stream, g->blk, member, g->last[(size_t)member], g->err, header, scored, kept, bounds_cap, bounds,
                              survivors_cap, survivors);
    });
}

int visfs_scan_group_match_refine(visfs_scan_group* g, const visfs_scan_stack_params* mp, const visfs_scan_refine_params* rp, const double* guesses,
                                  int32_t n, const double* xyz, visfs_scan_stack_result* results, int32_t* status, int32_t* best_member,
                                  visfs_scan_refine_result* refined) {
    if (!g || !mp || !rp || !guesses || !results || !status || !best_member || !refined || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(g, [&]() -> int { return group_match(g, *mp, guesses, n, xyz, results, status, best_member, rp, refined); });
}

int visfs_scan_group_refine_download(visfs_scan_group* g, int32_t member, int32_t cap, double* trace, int32_t* trials) {
    if (!g || !trials || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(g, [&]() -> int {
        if (member < 0 || member >= (int32_t)g->mem.size()) return fail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the group has no such member");
        const int32_t nt = (size_t)member < g->rtrials.size() ? g->rtrials[(size_t)member] : 0;
        *trials = nt;
        if (!trace || nt == 0) return (int)VISFS_BA_OK;
        if (cap < nt) return fail(g, VISFS_BA_ERR_BAD_ARGUMENT, "the hook's array is too small");
        const size_t bytes = (size_t)nt * scanrefine::kTraceItems * sizeof(double);
        if (!g->device) { std::memcpy(trace, g->h_rtrace[(size_t)member].data(), bytes); return (int)VISFS_BA_OK; }
        HIP_TRY(&g->err, hipSetDevice(g->dev));
        HIP_TRY(&g->err, hipMemcpyAsync(trace, g->d_rtrace[1].get() + (size_t)member * scanrefine::kMaxTrials * scanrefine::kTraceItems, bytes, hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(&g->err, hipStreamSynchronize(g->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_group_last_counts(const visfs_scan_group* g, int32_t* kernel_launches, int32_t* copies_and_memsets, int32_t* synchronisations) {
    return g ? g->blk.counts.read(kernel_launches, copies_and_memsets, synchronisations) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

}  // extern "C"
