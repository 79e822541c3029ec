// The stack object of the branch-and-bound scan matcher (ba_scan_fast.hip) and the one device call path that
// its single call and the group call over several stacks (ba_scan_group.hip, section 9n) both take: the search of one call, the
// one-core twin's schedule, the record, the call block (the device buffers of a call over m members), the launch sequence device_run
// and the bodies of its kernels.  The single call is the sequence at m = 1 on the stack's own block.  device_run and its kernels are
// defined in ba_scan_group.hip, the other host functions in ba_scan_fast.hip.
#pragma once
#include "ba_host.hpp"
#include "ba_scan_fast.hpp"

#include <climits>
#include <string>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

namespace scanfast {

using Frontier = host::DeviceBuf<int2>;
using Bounds = host::DeviceBuf<int32_t>;

// the last successful match, as the hook reports it
struct Last {
    bool have = false;
    int32_t S = 0, L = 0, n = 0, H = 0, mH = 0, survivors = 0;
    Ctrl c{};
    std::vector<int32_t> bounds;              // host twin
    std::vector<int2> surv;                   // host twin
};

// the search of one call
struct Search {
    scan::Plan P;
    int32_t H = 0, mH = 0, cap = 0;
    int32_t top() const { return P.S * mH * mH; }
};

// The device buffers of a call over m members, m fixed for the block's life (1: a stack's own, for its single calls): the upload
// with its pinned source, and every other one an arena of m equal slices: the cells, the records with their pinned copy (behind them
// room for m refinement records), bounds and frontiers of the call in work (bnd[0], fr[0], fr[1]) and those the hook reads (bnd[1],
// fr[2]), which change hands in hand_over.  Made by the first call.
struct CallBlock {
    host::Staged<char> up;
    host::DeviceBuf<int2> d_cells;
    host::DeviceBuf<char> d_ctrl; host::PinnedBuf<char> h_ctrl;      // Ctrl[m], then m refinement records
    Ctrl* ctrl_d() const { return reinterpret_cast<Ctrl*>(d_ctrl.get()); }
    Ctrl* ctrl_h() const { return reinterpret_cast<Ctrl*>(h_ctrl.get()); }
    Bounds bnd[2];
    Frontier fr[3];
    int64_t top = 0, cap = 0;                 // the strides of the hook's arenas: those of the last call handed over
    host::Counts counts;                      // of the last device_run
    // the hook's arenas become what a call wrote, its level-0 frontier in fr[cur]; they stay until the next hand-over
    void hand_over(int cur, const Search& s) {
        std::swap(bnd[0], bnd[1]);
        std::swap(fr[cur], fr[2]);
        top = s.top(); cap = s.cap;
    }
};

}  // namespace scanfast

// the buffers of visfs_scan_stack_refine on a stack (ba_scan_refine.hip), made by its first call
namespace scanrefine {
struct State;
struct Prm;
void state_free(State* s);
}

struct visfs_scan_stack {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    int32_t blocks = 1;                       // the fixed grid of the striding kernels: sized from the compute units
    submap::Limits L;
    int32_t depth = 0;
    int64_t bytes = 0;
    std::string err;
    size_t off[scanfast::kMaxDepth] = {};     // in uint16 items
    std::vector<uint16_t> h_mem;
    host::DeviceBuf<uint16_t> d_mem;
    scanfast::Levels lv;
    // a match on the device: a block for one member, whatever groups the stack is a member of; handed over by successful calls
    // only, so a failed call leaves the hook's arenas and `last`
    scanfast::CallBlock blk;
    scanfast::Last last;
    scanrefine::State* refine = nullptr;

    ~visfs_scan_stack() {                     // before the members free what they own
        if (device) {
            (void)hipSetDevice(dev);
            if (stream) (void)hipStreamSynchronize(stream);
        }
        scanrefine::state_free(refine);
    }
};

namespace scanfast {

// The argument checks of one call in the order visfs_scan_stack_match makes them (the pointers and n >= 0 already checked):
// VISFS_BA_OK, or the code with `why`.
int check_call(const visfs_scan_stack_params& p, const double g[3], int32_t n, const double* xyz, const char** why);
// The search of the scan about the guess on the stack's limits and depth, held to the limits of a call.
int make_search(const visfs_scan_stack* st, const visfs_scan_stack_params& p, const double g[3], int32_t n, const double* xyz, Search& s,
                const char** why);
std::string overflow_text(int32_t level, int32_t cap);
// the record of the winner (index, Q)
void finish(const Search& s, const visfs_scan_stack_params& p, int32_t index, int32_t Q, visfs_scan_stack_result* out);
// the record of a call without points: the guess back
void no_points(const double g[3], visfs_scan_stack_result* out);
// The one-core twin's schedule over the levels `lv`: fills `now` (counts, bounds, sorted survivors, winner) and returns VISFS_BA_OK;
// on a frontier overflow VISFS_BA_ERR_UNSUPPORTED, on an empty result VISFS_BA_ERR_DEVICE, with `why`.
int host_search(const Levels& lv, const Search& s, Last& now, std::string& why);

// The searches ss[0..m) of one scan, equal in S, nl, H, m_H and capacity, on the stacks mem[0..m) in one sequence on `stream`: one
// upload, H + 5 launches, one download and one wait, `blocks` being the fixed grid of the striding kernels shared among the members.
// Fills b.h_ctrl[0..m) and leaves member i's level-0 frontier in slice i of b.fr[*cur]; the hand-over is the caller's.  With `rp`
// every matched member's refinement follows in the same sequence, its traces into `rtrace` [m][kMaxTrials][kTraceItems] and its
// records behind the Ctrl records.  VISFS_BA_OK, or VISFS_BA_ERR_DEVICE with `why`.
int device_run(CallBlock& b, int dev, hipStream_t stream, int32_t blocks, int32_t m, visfs_scan_stack* const* mem, const Search* ss, int* cur,
               std::string& why, const scanrefine::Prm* rp = nullptr, double min_score = 0.0, double* rtrace = nullptr);
// the record of a member whose search on the device came to its end with the winner in `c`
Last device_last(const Search& s, const Ctrl& c);
// The hook of both calls on `l`, the record of member `member` of the last call handed over in `b` (a host twin's arrays stand in
// `l` itself).  VISFS_BA_OK, or the code with `why`.
int match_download(bool device, int dev, hipStream_t stream, const CallBlock& b, int64_t member, const Last& l, std::string& why, int32_t header[8],
                   int32_t scored[16], int32_t kept[16], int64_t bounds_cap, int32_t* bounds, int64_t survivors_cap, int32_t* survivors);

#ifdef __HIPCC__
__device__ inline int32_t wave_sum(int32_t v) {
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum over the scan's n cells of P_h(cell + (xo, yo)): every lane of the wavefront calls, every lane gets the sum
__device__ inline int32_t wave_node_sum(const int2* __restrict__ c, int32_t n, const LevelView& v, int32_t xo, int32_t yo, int lane) {
    int32_t q = 0;
    for (int32_t i = lane; i < n; i += kWave) { const int2 p = c[i]; q += level_read(v, p.x + xo, p.y + yo); }
    return wave_sum(q);
}

// The bodies of the match kernels.  Each works on one search: the kernels (k_group_*, ba_scan_group.hip) pass member blockIdx.y's
// slices.  Only blockIdx.x and gridDim.x are read here.
__device__ inline void cells_body(const double* __restrict__ pts, const double* __restrict__ rot, int32_t n, int64_t total, double gx, double gy,
                                  double res, double max_x, double max_y, int2* __restrict__ cells, Ctrl* __restrict__ ctrl) {
    if (blockIdx.x == 0 && threadIdx.x < sizeof(Ctrl) / sizeof(int32_t)) reinterpret_cast<int32_t*>(ctrl)[threadIdx.x] = 0;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t k = (int32_t)(i / n), j = (int32_t)(i - (int64_t)k * n);
    int32_t ix, iy;
    scan::discretise(rot[2 * k], rot[2 * k + 1], pts[2 * j], pts[2 * j + 1], gx, gy, res, max_x, max_y, ix, iy);
    cells[i] = make_int2(ix, iy);
}

__device__ inline void bounds_body(const int2* __restrict__ cells, int32_t n, const LevelView& vH, int32_t nl, int32_t H, int32_t mH, int32_t total,
                                   int32_t* __restrict__ bounds) {
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t nw = gridDim.x * kWaves;
    for (int32_t id = blockIdx.x * kWaves + (threadIdx.x >> 6); id < total; id += nw) {
        int32_t k, i, j;
        node_decode(mH, id, k, i, j);
        const int32_t U = wave_node_sum(cells + (int64_t)k * n, n, vH, -nl + (i << H), -nl + (j << H), lane);
        if (lane == 0) bounds[id] = U;
    }
}

__device__ inline void seeds_body(const int32_t* __restrict__ bounds, const int2* __restrict__ cells, int32_t n, const Levels& lv, int32_t nl, int32_t L,
                                  int32_t H, int32_t mH, Ctrl* __restrict__ ctrl) {
    __shared__ int32_t s_u[kThreads];
    __shared__ int32_t s_i[kThreads];
    __shared__ int32_t s_c[kWaves];
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
    const int32_t k = blockIdx.x, per = mH * mH;
    int32_t u = -1, id = INT_MAX;
    for (int32_t a = t; a < per; a += kThreads) {
        const int32_t ua = bounds[k * per + a];
        if (better(ua, a, u, id)) { u = ua; id = a; }
    }
    s_u[t] = u; s_i[t] = id;
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h && better(s_u[t + h], s_i[t + h], s_u[t], s_i[t])) { s_u[t] = s_u[t + h]; s_i[t] = s_i[t + h]; }
    }
    __syncthreads();
    int32_t i = s_i[0] / mH, j = s_i[0] % mH, cur = s_u[0];
    const int2* c = cells + (int64_t)k * n;
    for (int32_t h = H; h >= 1; --h) {                                     // every choice: the larger bound, then the lower index
        const int32_t m = nodes_per_axis(L, h - 1);
        const int32_t ci = 2 * i + (w >> 1), cj = 2 * j + (w & 1);
        int32_t U = -1;
        if (ci < m && cj < m) U = wave_node_sum(c, n, lv.v[h - 1], -nl + (ci << (h - 1)), -nl + (cj << (h - 1)), lane);
        if (lane == 0) s_c[w] = U;
        __syncthreads();
        int bw = 0;
        for (int a = 1; a < kWaves; ++a) if (s_c[a] > s_c[bw]) bw = a;
        cur = s_c[bw];
        i = 2 * i + (bw >> 1); j = 2 * j + (bw & 1);
        __syncthreads();
    }
    if (t == 0) atomicMax(&ctrl->B, cur);
}

__device__ inline void keep_body(const int32_t* __restrict__ bounds, int32_t total, int32_t H, int2* __restrict__ out, int32_t cap,
                                 Ctrl* __restrict__ ctrl) {
    const int32_t B = ctrl->B;
    const int32_t nt = gridDim.x * kThreads;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->scored[H] = total;
    for (int32_t id = blockIdx.x * kThreads + threadIdx.x; id < total; id += nt) {
        const int32_t U = bounds[id];
        if (U < B) continue;
        const int32_t slot = atomicAdd(&ctrl->kept[H], 1);
        if (slot < cap) out[slot] = make_int2(id, U);
        else atomicMax(&ctrl->overflow, H + 1);
    }
}

__device__ inline void level_body(int32_t h, const int2* __restrict__ in, int2* __restrict__ out, int32_t cap, const int2* __restrict__ cells, int32_t n,
                                  const LevelView& lo, int32_t nl, int32_t L, Ctrl* __restrict__ ctrl) {
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t nw = gridDim.x * kWaves;
    const int32_t cnt = min(ctrl->kept[h], cap), B = ctrl->B;
    const int32_t mh = nodes_per_axis(L, h), ml = nodes_per_axis(L, h - 1), half = 1 << (h - 1);
    int32_t nscored = 0;
    for (int32_t e = blockIdx.x * kWaves + (threadIdx.x >> 6); e < cnt; e += nw) {
        int32_t k, i, j;
        node_decode(mh, in[e].x, k, i, j);
        const int32_t ci = 2 * i, cj = 2 * j;
        const int32_t xo = -nl + ci * half, yo = -nl + cj * half;
        const bool vx = ci + 1 < ml, vy = cj + 1 < ml;                     // the children clipped by the window
        const int2* c = cells + (int64_t)k * n;
        int32_t q00 = 0, q01 = 0, q10 = 0, q11 = 0;
        for (int32_t a = lane; a < n; a += kWave) {
            const int2 p = c[a];
            const int32_t x = p.x + xo, y = p.y + yo;
            q00 += level_read(lo, x, y);
            if (vy) q01 += level_read(lo, x, y + half);
            if (vx) q10 += level_read(lo, x + half, y);
            if (vx && vy) q11 += level_read(lo, x + half, y + half);
        }
        q00 = wave_sum(q00); q01 = wave_sum(q01); q10 = wave_sum(q10); q11 = wave_sum(q11);
        if (lane == 0) {
            const int32_t U[4] = { q00, q01, q10, q11 };
            const bool ok[4] = { true, vy, vx, vx && vy };
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (!ok[a]) continue;
                ++nscored;
                if (U[a] < B) continue;
                const int32_t slot = atomicAdd(&ctrl->kept[h - 1], 1);
                if (slot < cap) out[slot] = make_int2(node_id(ml, k, ci + (a >> 1), cj + (a & 1)), U[a]);
                else atomicMax(&ctrl->overflow, h);                        // 1 + the level that overflowed
            }
        }
    }
    if (lane == 0 && nscored) atomicAdd(&ctrl->scored[h - 1], nscored);
}

__device__ inline void best_body(const int2* __restrict__ in, int32_t cap, Ctrl* __restrict__ ctrl) {
    __shared__ int32_t s_u[kThreads];
    __shared__ int32_t s_i[kThreads];
    const int t = threadIdx.x;
    const int32_t cnt = min(ctrl->kept[0], cap);
    int32_t u = -1, id = INT_MAX;
    for (int32_t a = t; a < cnt; a += kThreads) {
        const int2 e = in[a];
        if (better(e.y, e.x, u, id)) { u = e.y; id = e.x; }
    }
    s_u[t] = u; s_i[t] = id;
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h && better(s_u[t + h], s_i[t + h], s_u[t], s_i[t])) { s_u[t] = s_u[t + h]; s_i[t] = s_i[t + h]; }
    }
    __syncthreads();
    if (t == 0) { ctrl->best_index = s_i[0]; ctrl->best_sum = s_u[0]; }
}
#endif

}  // namespace scanfast
