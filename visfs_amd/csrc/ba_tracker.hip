// The resident front end (include/visfs_tracker.h): Tracker::pretreatment and Tracker::imageProcess of the
// reference (corelib/src/Tracker.cpp:98-419) in one call, with the word table of the tracker kept next to the image pyramids.
//
// Two ways over the decisions of ba_tracker.hpp and the work items of ba_flow.hpp / ba_corners.hpp:
//   * host restatement (trackers on objects of visfs_flow_create_host): every step in sequence on one core;
//   * device: the table (id, left pixel, 3-D point, track count) and every intermediate list stay in HBM.  A call is a tracker
//     group of one: one upload of the call's tables (outlier ids and guess in them), the frame's pyramids,
//     these launches on the stream of the owning handle, one copy of the output block and one synchronisation.  Every kernel reads
//     its arguments from the table at member blockIdx.z and carries the suffix _g.  No launch waits for a value read back:
//     counts travel through a control block in device memory, the grids are sized by what the host knows (the ids it returned
//     last, max_features) and surplus workgroups leave at once.
//       k_trk_pretreat_g  one workgroup: each row's id against the outlier list in LDS, order-preserving split into from-table and
//                       blocked list (ballot + prefix over the wavefronts)                                          (:143-165)
//       [bootstrap]     the corner kernels on the previous left image without a mask, k_trk_append_g, k_trk_stereo_g in its
//                       forward-only, ungated, status-blind form for the 3-D points                                 (:179-230)
//       k_trk_track_g   one wavefront per from-row: guess projection in fp64, lk_gated, the bounds test          (:237-274, :286)
//       [cull]          Tracker/CullByFundationMatrix with flow_back off: k_trk_cull_rows_g, one workgroup:
//                       the from-rows with four finite coordinates compacted in row order, the two Hartley transforms with the
//                       serial sums of fund::hartley, the winner key zeroed; then k_fund_ransac_g and k_fund_mask_g of ba_fund.hip
//                       (fund::group_cull), which leave the status after the AND for the reduce to keep its rows on    (:275-277, :83-96)
//       k_trk_reduce_g  one workgroup: compaction of the kept rows in row order: covisible output, kept count, LOST, the top-up's
//                       corner budget                                                                               (:280-320)
//       [pose guess]    estimateMotion3DTo2D on the covisible rows (include/visfs_tracker_pnp.h): k_trk_pnp_rows_g,
//                       one workgroup: the covisible rows with a finite 3-D point compacted in row order, their number, the winner
//                       key zeroed, the result of a call without a search; then k_pnp_ransac_g and k_pnp_refine_g of ba_pnp.hip
//                       (pnp::group_pnp), which leave model and inlier list in the output block       (MultiviewGeometry.cpp:94-216)
//       k_trk_discs_g   one workgroup: rank sort of the (count, row) keys, the serial draw decision of getMask 1024 discs at a time
//                       (each against the raster so far in parallel; then wavefront after wavefront settles its 64 discs among
//                       themselves through cover masks and the ones behind test against what it drew), the raster's Disc list
//                       and its length                                                                              (:116-141)
//       the corner kernels of ba_corners.hip on the current left image, disc count and budget read from device memory    (:327)
//       k_trk_append_g  ids for the new corners, appended behind the kept rows                                      (:330-336)
//       k_trk_stereo_g  one wavefront per row: lk_gated left -> right, bounds test, triangulate                     (:343-397)
//       k_trk_finish_g  one workgroup: final compaction into the table, counts + 1, the output block's head        (:98-114, :414-417)
//   * tracker groups (include/visfs_tracker_group.h): the same sequence (run_call) with n members in the
//     table, so n trackers of one handle take one launch sequence and one synchronisation.  plan_member and commit_member are the
//     per-member decisions in front of a call and the bookkeeping behind it, for both entry points.
#include "ba_tracker.hpp"
#include "ba_flow_object.hpp"
#include "ba_group.hpp"
#include "ba_fund.hpp"
#include "ba_pnp.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_tracker.h"
#include "../../include/visfs_tracker_pnp.h"
#include "../../include/visfs_tracker_group.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

using namespace flow;
using namespace trk;
using namespace host;

struct visfs_tracker;
struct visfs_tracker_group;

namespace flow {
struct TrackerState { std::vector<visfs_tracker*> list; };
}

namespace trk {

constexpr int TK_T = 1024;                     // the one-workgroup kernels
constexpr int TK_WAVES = TK_T / 64;

struct Ctl {                                   // device words of a tracker
    int32_t n_tab;                             // rows of the table (lives across calls)
    int32_t n_from, n_blocked, n_kept, lost, n_list, n_new, n_rows;
    int32_t corner_args[2];                    // the top-up: { raster discs, max_features - kept }
    int32_t boot_args[2];                      // the bootstrap: { 0, max_features }
    uint64_t next_id;                          // globalFeatureId_ (lives across calls)
    int32_t cull_m;                            // from-rows that entered the fundamental-matrix cull
    int32_t pnp_m;                             // covisible rows that entered the pose guess
};

struct Head {                                  // first words of the output block
    int32_t flags, n_covis, n_new, n_words, n_blocked, pad;
    uint64_t next_id;
};

struct InHead {                                // first words of the input block; the outlier ids follow
    int32_t n_outliers, pad;
};

struct Out {                                   // the output block, one layout for the device, the pinned copy and the host twin
    Head* head;
    uint64_t* cov_id; float* cov_from; float* cov_xyz; float* cov_to;
    uint64_t* new_id; float* new_xy;
    uint64_t* w_id; float* w_l; float* w_r; float* w_xyz; int32_t* w_cnt;
    uint64_t* blk_id;
    // the pose guess (all NULL on a tracker that never enabled it): rows that entered, the refine stage's block, its inlier list
    // (numbers of rows that entered), the covisible row of every row that entered
    int32_t* p_m; pnp::Result* p_res; int32_t* p_inl; int32_t* p_match;
};

struct Bufs {
    Ctl* ctl;
    const InHead* in; const uint64_t* outliers;
    uint64_t* tab_id; float* tab_xy; float* tab_xyz; int32_t* tab_cnt;            // the table
    uint64_t* from_id; float* from_xy; float* from_xyz; int32_t* from_cnt;        // the from-rows of a call
    float* blk_xy;
    float* guess; float* to; uint8_t* lk_st; uint8_t* inb;                        // per from-row
    const uint8_t* keep_st;                                                       // the status the reduce keeps a row on: lk_st, or the cull's
    fund::CullRec cull;                                                           // all NULL without the cull
    pnp::Row* pnp_rows; unsigned long long* pnp_key;                              // the pose guess: NULL without it
    uint64_t* row_id; float* row_xy; int32_t* row_cnt;                            // kept + new rows
    float* row_rxy; float* row_xyz; uint8_t* row_st; uint8_t* row_ok;
    visfs_corners_disc* list; uint32_t* packed; uint8_t* drawn; Disc* raster;     // getMask's discs in draw order; the raster's
    const int32_t* hw;                                                            // half-widths: min_distance, then min_distance / 2
    Out o;
};

struct Carver {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

// with_pnp: the pose guess's part behind the block of a tracker without it, whose layout stays what it is
size_t carve_out(char* base, size_t M, bool with_pnp, Out& o) {
    Carver c{ base };
    o.head = c.take<Head>(1);
    o.cov_id = c.take<uint64_t>(M); o.cov_from = c.take<float>(2 * M); o.cov_xyz = c.take<float>(3 * M); o.cov_to = c.take<float>(2 * M);
    o.new_id = c.take<uint64_t>(M); o.new_xy = c.take<float>(2 * M);
    o.w_id = c.take<uint64_t>(M); o.w_l = c.take<float>(2 * M); o.w_r = c.take<float>(2 * M); o.w_xyz = c.take<float>(3 * M);
    o.w_cnt = c.take<int32_t>(M);
    o.blk_id = c.take<uint64_t>(M);
    o.p_m = nullptr; o.p_res = nullptr; o.p_inl = nullptr; o.p_match = nullptr;
    if (with_pnp) {
        o.p_m = c.take<int32_t>(1); o.p_res = c.take<pnp::Result>(1); o.p_inl = c.take<int32_t>(M); o.p_match = c.take<int32_t>(M);
    }
    return (c.off + 255) & ~size_t(255);
}

// cull_iters: the hypotheses of the fundamental-matrix cull, 0 without it
size_t carve_work(char* base, size_t M, size_t hw_len, size_t cull_iters, Bufs& b, int32_t** hw) {
    Carver c{ base };
    b.ctl = c.take<Ctl>(1);
    b.tab_id = c.take<uint64_t>(M); b.tab_xy = c.take<float>(2 * M); b.tab_xyz = c.take<float>(3 * M); b.tab_cnt = c.take<int32_t>(M);
    b.from_id = c.take<uint64_t>(M); b.from_xy = c.take<float>(2 * M); b.from_xyz = c.take<float>(3 * M); b.from_cnt = c.take<int32_t>(M);
    b.blk_xy = c.take<float>(2 * M);
    b.guess = c.take<float>(2 * M); b.to = c.take<float>(2 * M); b.lk_st = c.take<uint8_t>(M); b.inb = c.take<uint8_t>(M);
    b.row_id = c.take<uint64_t>(M); b.row_xy = c.take<float>(2 * M); b.row_cnt = c.take<int32_t>(M);
    b.row_rxy = c.take<float>(2 * M); b.row_xyz = c.take<float>(3 * M); b.row_st = c.take<uint8_t>(M); b.row_ok = c.take<uint8_t>(M);
    b.list = c.take<visfs_corners_disc>(2 * M); b.packed = c.take<uint32_t>(2 * M); b.drawn = c.take<uint8_t>(2 * M);
    b.raster = c.take<Disc>(2 * M);
    *hw = c.take<int32_t>(hw_len);
    b.hw = *hw;
    b.keep_st = b.lk_st;
    b.pnp_rows = nullptr; b.pnp_key = nullptr;
    b.cull = fund::CullRec{};
    if (cull_iters > 0) {
        fund::CullRec& q = b.cull;
        q.m = base ? &b.ctl->cull_m : nullptr;
        q.head = c.take<fund::Header>(1); q.res = c.take<fund::Result>(1);
        q.rows = c.take<fund::Row>(M); q.keep = c.take<int32_t>(M); q.st = c.take<uint8_t>(M);
        q.samples = c.take<int32_t>(7 * cull_iters); q.nc = c.take<int32_t>(4 * cull_iters); q.models = c.take<double>(27 * cull_iters);
        q.mask = c.take<uint8_t>(M); q.status = c.take<uint8_t>(M);
        b.keep_st = q.status;
    }
    return (c.off + 255) & ~size_t(255);
}

struct Shape { int32_t M, w, h, r_track, r_blocked, min_inliers; };

// A member of a call: the arguments of the kernels, read by them from the call's table in device memory at
// blockIdx.z.  B.in and B.outliers point into the upload block the call goes through.
struct TrkRec {
    Bufs B;
    Image prev[2], cur[2];                     // left, right of the slot before and of the slot this call pushed into
    Camera cam;
    Guess g;
    const int32_t* corner_n; const float* corner_xy;     // where the member's corner extraction leaves its count and its corners
    int32_t has_guess;
    int32_t skip;                              // NO_PREVIOUS: the pair is pushed and nothing else runs
    int32_t boot;
    int32_t pad;
};

// ---------------------------------------------------------------- kernels
// where a flagged thread's item goes in an order-preserving compaction of the workgroup's items, and how many there are
__device__ inline int wg_offset(bool flag, int32_t* wcount, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wcount[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < TK_WAVES; ++k) {
        const int c = wcount[k];
        if (k < wave) before += c;
        total += c;
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// Every kernel works for member blockIdx.z of the call's table in device memory (a single call is a table of one).  A member without
// a previous pair leaves every one of them at once; a member that does not bootstrap leaves the bootstrap's.
__global__ __launch_bounds__(TK_T) void k_trk_pretreat_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const Bufs& B = r.B;
    __shared__ uint64_t s_out[kMaxOutliers];
    __shared__ int32_t wcount[TK_WAVES];
    const int tid = threadIdx.x;
    const int n = min(B.ctl->n_tab, S.M);
    const int n_o = min(max(B.in->n_outliers, 0), kMaxOutliers);
    for (int k = tid; k < n_o; k += TK_T) s_out[k] = B.outliers[k];
    __syncthreads();
    int n_keep = 0, n_blk = 0;
    for (int c0 = 0; c0 < n; c0 += TK_T) {
        const int i = c0 + tid;
        const bool valid = i < n;
        const uint64_t id = valid ? B.tab_id[i] : 0ull;
        bool hit = false;
        if (valid)
            for (int k = 0; k < n_o; ++k) hit = hit || s_out[k] == id;
        int tk, tb;
        const int ok = wg_offset(valid && !hit, wcount, tk);
        const int ob = wg_offset(hit, wcount, tb);
        if (valid && !hit) {
            const int o = n_keep + ok;
            B.from_id[o] = id;
            B.from_xy[2 * o] = B.tab_xy[2 * i]; B.from_xy[2 * o + 1] = B.tab_xy[2 * i + 1];
            B.from_xyz[3 * o] = B.tab_xyz[3 * i]; B.from_xyz[3 * o + 1] = B.tab_xyz[3 * i + 1]; B.from_xyz[3 * o + 2] = B.tab_xyz[3 * i + 2];
            B.from_cnt[o] = B.tab_cnt[i];
        }
        if (hit) {
            const int o = n_blk + ob;
            B.o.blk_id[o] = id;
            B.blk_xy[2 * o] = B.tab_xy[2 * i]; B.blk_xy[2 * o + 1] = B.tab_xy[2 * i + 1];
        }
        n_keep += tk;
        n_blk += tb;
    }
    if (tid == 0) {
        Ctl* c = B.ctl;
        c->n_from = n_keep; c->n_blocked = n_blk;
        c->n_kept = 0; c->lost = 0; c->n_list = 0; c->n_new = 0; c->n_rows = 0;
        c->corner_args[0] = 0; c->corner_args[1] = 0;
        c->boot_args[0] = 0; c->boot_args[1] = S.M;
        c->cull_m = 0;
    }
}

// The corners of a selection get ids next_id, next_id + 1, ... strongest first.  BOOT: they are the from-rows of this call, without a
// track count (Tracker.cpp:181-189).  Otherwise they follow the kept rows and are this frame's newly extracted words (:330-336).
template <bool BOOT>
__global__ __launch_bounds__(TK_T) void k_trk_append_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip || (BOOT && !r.boot)) return;
    const Bufs& B = r.B;
    const int32_t* n_out = r.corner_n;
    const float* xy = r.corner_xy;
    Ctl* c = B.ctl;
    const int tid = threadIdx.x;
    const int base = BOOT ? 0 : c->n_kept;
    int n = (!BOOT && c->lost) ? 0 : *n_out;
    n = max(min(n, S.M - base), 0);
    const uint64_t id0 = c->next_id;
    for (int a = tid; a < n; a += TK_T) {
        const uint64_t id = id0 + (uint64_t)a;
        const float x = xy[2 * a], y = xy[2 * a + 1];
        if (BOOT) {
            B.from_id[a] = id; B.from_xy[2 * a] = x; B.from_xy[2 * a + 1] = y; B.from_cnt[a] = 0;
        } else {
            const int r = base + a;
            B.row_id[r] = id; B.row_xy[2 * r] = x; B.row_xy[2 * r + 1] = y; B.row_cnt[r] = 0;
            B.o.new_id[a] = id; B.o.new_xy[2 * a] = x; B.o.new_xy[2 * a + 1] = y;
        }
    }
    __syncthreads();
    if (tid == 0) {
        c->next_id = id0 + (uint64_t)n;
        if (BOOT) c->n_from = n;
        else { c->n_new = n; c->n_rows = base + n; }
    }
}

struct WaveCells {                             // as in ba_flow.hip: cell s * 64 + lane in slot s, int64 butterfly
    static constexpr int kSlots = kLaneSlots;
    // int32 holds a lane's 7 products (derivation in ba_flow.hip): |gx|, |gy| <= 4081 and |diff| <= 8160 give at most
    // 7 * 8160 * 4081 = 2.33e8, against 2^31
    using acc_t = int32_t;
    int lane;
    __device__ int cell(int s) const { return s * 64 + lane; }
    __device__ int64_t total(acc_t v) const {
        long long x = v;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        return x;
    }
};

template <bool BACK>
__global__ __launch_bounds__(64) void k_trk_track_g(const TrkRec* __restrict__ recs, Shape S, LkParams prm, Layout lay, float gate) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const Bufs& B = r.B;
    const Image &I = r.prev[0], &J = r.cur[0];
    const Guess& g = r.g;
    const int has_guess = r.has_guess;
    const int p = blockIdx.x;
    if (p >= min(B.ctl->n_from, S.M)) return;
    WaveCells pol{ (int)threadIdx.x };
    const float ptx = B.from_xy[2 * p], pty = B.from_xy[2 * p + 1];
    float inx = ptx, iny = pty;
    if (has_guess) {
        const float P[3] = { B.from_xyz[3 * p], B.from_xyz[3 * p + 1], B.from_xyz[3 * p + 2] };
        project_guess(g, P, inx, iny);
    }
    float tox, toy, err;
    uint8_t st;
    lk_gated(pol, prm, lay, I, J, ptx, pty, has_guess != 0, inx, iny, BACK, gate, tox, toy, st, err);
    if (threadIdx.x != 0) return;
    B.guess[2 * p] = inx; B.guess[2 * p + 1] = iny;
    B.to[2 * p] = tox; B.to[2 * p + 1] = toy;
    B.lk_st[p] = st;
    B.inb[p] = (in_bounds(tox, S.w) && in_bounds(toy, S.h)) ? 1 : 0;
}

// The first two steps of the fundamental-matrix cull, which the staged visfs_fund_cull does on the host: the from-rows whose four
// coordinates are finite, whatever their status, compacted in row order, and the two Hartley transforms.  The terms of the sums are
// made by all lanes into LDS; the additions are the serial chains of fund::hartley (four for the means, then two for the
// distances, each on the first lane of a wavefront of its own), so the bytes are those of the host conditioning.  Rows that do not
// enter get mask 0 and status 0 here; with fewer than seven rows the status passes through and nothing else of the cull runs.
static_assert(kMaxFeatures <= fund::kMaxPoints && fund::kMaxPoints == 4 * TK_T, "a thread of the rows kernel owns up to four rows");
__global__ __launch_bounds__(TK_T) void k_trk_cull_rows_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const Bufs& B = r.B;
    const fund::CullRec& C = B.cull;
    __shared__ fund::Row s_rows[fund::kMaxPoints];     // the rows that entered; then the distance terms, double [2][kMaxPoints]
    __shared__ int32_t wcount[TK_WAVES];
    __shared__ double s_sum[6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(B.ctl->n_from, S.M);
    if (n <= 0) {
        if (tid == 0) *C.m = 0;
        return;
    }
    int m = 0;
    for (int c0 = 0; c0 < n; c0 += TK_T) {
        const int i = c0 + tid;
        const bool valid = i < n;
        fund::Row q{ 0.0f, 0.0f, 0.0f, 0.0f };
        if (valid) q = fund::Row{ B.from_xy[2 * i], B.from_xy[2 * i + 1], B.to[2 * i], B.to[2 * i + 1] };
        const bool enters = valid && isfinite(q.x1) && isfinite(q.y1) && isfinite(q.x2) && isfinite(q.y2);
        int total;
        const int o = m + wg_offset(enters, wcount, total);
        if (enters) {
            s_rows[o] = q;
            C.rows[o] = q; C.keep[o] = i; C.st[o] = B.lk_st[i] ? 1 : 0;
        }
        m += total;
    }
    const bool passes = m < fund::kMinRows;
    for (int i = tid; i < n; i += TK_T) { C.mask[i] = 0; C.status[i] = (passes && B.lk_st[i]) ? 1 : 0; }
    if (tid == 0) *C.m = m;
    if (passes) return;
    __syncthreads();
    if (lane == 0 && wave < 4) s_sum[wave] = fund::serial_sum(&s_rows[0].x1 + wave, m, 4);      // x1, y1, x2, y2
    __syncthreads();
    const double dm = (double)m;
    const double cx1 = s_sum[0] / dm, cy1 = s_sum[1] / dm, cx2 = s_sum[2] / dm, cy2 = s_sum[3] / dm;
    double d1[4], d2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + k * TK_T;
        d1[k] = d2[k] = 0.0;
        if (i < m) {
            const fund::Row q = s_rows[i];
            d1[k] = fund::centre_distance((double)q.x1, (double)q.y1, cx1, cy1);
            d2[k] = fund::centre_distance((double)q.x2, (double)q.y2, cx2, cy2);
        }
    }
    __syncthreads();
    double* s_term = reinterpret_cast<double*>(s_rows);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + k * TK_T;
        if (i < m) { s_term[i] = d1[k]; s_term[fund::kMaxPoints + i] = d2[k]; }
    }
    __syncthreads();
    if (lane == 0 && wave < 2) s_sum[4 + wave] = fund::serial_sum(s_term + wave * fund::kMaxPoints, m, 1);
    __syncthreads();
    if (tid == 0) {
        fund::Header hd;
        hd.key = 0; hd.pad = 0;                                                   // no winner yet
        hd.T1 = fund::hartley_of(cx1, cy1, s_sum[4], dm); hd.T2 = fund::hartley_of(cx2, cy2, s_sum[5], dm);
        *C.head = hd;
    }
}

__global__ __launch_bounds__(TK_T) void k_trk_reduce_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const Bufs& B = r.B;
    __shared__ int32_t wcount[TK_WAVES];
    const int tid = threadIdx.x;
    const int n = min(B.ctl->n_from, S.M);
    int kept = 0;
    for (int c0 = 0; c0 < n; c0 += TK_T) {
        const int i = c0 + tid;
        const bool keep = i < n && kept_row(B.keep_st[i], B.to[2 * i], B.to[2 * i + 1], S.w, S.h);
        int total;
        const int o = kept + wg_offset(keep, wcount, total);
        if (keep) {
            const uint64_t id = B.from_id[i];
            const float tx = B.to[2 * i], ty = B.to[2 * i + 1];
            B.o.cov_id[o] = id;
            B.o.cov_from[2 * o] = B.from_xy[2 * i]; B.o.cov_from[2 * o + 1] = B.from_xy[2 * i + 1];
            B.o.cov_xyz[3 * o] = B.from_xyz[3 * i]; B.o.cov_xyz[3 * o + 1] = B.from_xyz[3 * i + 1]; B.o.cov_xyz[3 * o + 2] = B.from_xyz[3 * i + 2];
            B.o.cov_to[2 * o] = tx; B.o.cov_to[2 * o + 1] = ty;
            B.row_id[o] = id; B.row_xy[2 * o] = tx; B.row_xy[2 * o + 1] = ty; B.row_cnt[o] = B.from_cnt[i];
        }
        kept += total;
    }
    if (tid == 0) {
        Ctl* c = B.ctl;
        const bool lost = kept < S.min_inliers;                                   // Tracker.cpp:303
        c->n_kept = kept; c->n_rows = lost ? 0 : kept; c->lost = lost ? 1 : 0;
        c->corner_args[1] = lost ? 0 : S.M - kept;                                // backUpCornersCnt (:324)
    }
}

// Step 1 of the pose guess, which the staged visfs_pnp_solve does on the host: the covisible rows with three finite from_xyz
// coordinates compacted in row order into the row list and the match index.  It leaves m, the zeroed winner key and the result of a
// call whose search does not run (too few rows); the refine stage writes over that one when it runs.  A LOST call has no rows.
__global__ __launch_bounds__(TK_T) void k_trk_pnp_rows_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const Bufs& B = r.B;
    __shared__ int32_t wcount[TK_WAVES];
    const int tid = threadIdx.x;
    Ctl* c = B.ctl;
    const int n = c->lost ? 0 : min(c->n_kept, S.M);
    int m = 0;
    for (int c0 = 0; c0 < n; c0 += TK_T) {
        const int i = c0 + tid;
        const bool valid = i < n;
        pnp::Row q{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        if (valid) q = pnp::Row{ B.o.cov_xyz[3 * i], B.o.cov_xyz[3 * i + 1], B.o.cov_xyz[3 * i + 2], B.o.cov_to[2 * i], B.o.cov_to[2 * i + 1] };
        const bool enters = valid && isfinite(q.X) && isfinite(q.Y) && isfinite(q.Z);
        int total;
        const int o = m + wg_offset(enters, wcount, total);
        if (enters) { B.pnp_rows[o] = q; B.o.p_match[o] = i; }
        m += total;
    }
    if (tid == 0) {
        c->pnp_m = m; *B.o.p_m = m;
        *B.pnp_key = 0ull;                                                        // no winner yet
        pnp::Result res{};
        res.winner = -1;
        *B.o.p_res = res;
    }
}

constexpr int kHwLds = 2048;                   // half-width entries kept in LDS (both radii together); larger tables are read in place

// does the packed disc p cover the pixel (x, y)?  HW is the half-width storage (LDS or global), the two tables one behind the other
template <class HW>
__device__ inline bool packed_covers(uint32_t p, const Shape& S, HW hw, int x, int y) {
    const int kind = (int)(p >> 30);
    return disc_covers_flat((int)(p & 0x7fffu), (int)((p >> 15) & 0x7fffu), kind ? S.r_blocked : S.r_track, hw + (kind ? S.r_track + 1 : 0), x, y);
}

// The draw decision in list order (Tracker.cpp:131-138).  Thread t of a chunk owns disc c0 + t.  Every disc is first tested against
// the raster of the chunks before; then the wavefronts take their turns: wavefront k settles its 64 discs among themselves and
// appends the drawn ones, and the wavefronts behind it test theirs against what it appended.  No loop over discs leaves early, so
// its reads do not wait for each other.
template <class HW>
__device__ inline int draw_decision(const Bufs& B, const Shape& S, HW hw, int n_list, uint32_t* s_buf, int32_t* s_nr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nr = 0, round = 0;
    for (int c0 = 0; c0 < n_list; c0 += TK_T) {
        const int i = c0 + tid;
        const bool valid = i < n_list;
        const uint32_t q = valid ? B.packed[i] : 0u;
        const Disc dq = unpack_disc(q, S.r_track, S.r_blocked);
        const bool inside = centre_inside(dq.cx, dq.cy, S.w, S.h);
        bool alive = valid;
        if (valid && inside) {
            bool covered = false;
#pragma unroll 8
            for (int a = 0; a < nr; ++a) covered |= packed_covers(s_buf[a], S, hw, dq.cx, dq.cy);
            alive = !covered;
        }
        const int waves = (min(TK_T, n_list - c0) + 63) / 64;
        for (int k = 0; k < waves; ++k, ++round) {
            if (wave == k) {
                // which earlier discs of this wavefront would cover my centre, should they be drawn
                const unsigned long long live = __ballot(alive);
                unsigned long long cover = 0;
#pragma unroll 8
                for (int j = 0; j < 63; ++j) {
                    const uint32_t qj = __shfl(q, j, 64);
                    if (packed_covers(qj, S, hw, dq.cx, dq.cy)) cover |= 1ull << j;
                }
                cover &= live & ((1ull << lane) - 1ull);
                if (!(alive && inside)) cover = 0;
                // a disc nothing could cover is drawn; the others are settled in order, each once all before it are
                unsigned long long drawn = __ballot(alive && cover == 0);
                unsigned long long open = __ballot(alive && cover != 0);
                while (open) {
                    const int f = __ffsll(open) - 1;
                    const unsigned long long cf = __shfl(cover, f, 64);
                    if ((cf & drawn) == 0) drawn |= 1ull << f;
                    open &= open - 1;
                }
                const bool mine = ((drawn >> lane) & 1ull) != 0;
                const bool raster = mine && touches_image(dq, S.w, S.h);
                const unsigned long long rb = __ballot(raster);
                if (valid) B.drawn[i] = mine ? 1 : 0;
                if (raster) {
                    const int o = nr + __popcll(rb & ((1ull << lane) - 1ull));
                    s_buf[o] = q;
                    B.raster[o] = dq;
                }
                if (lane == 0) s_nr[round & 1] = nr + __popcll(rb);
            }
            __syncthreads();
            const int nr_new = s_nr[round & 1];
            if (wave > k && alive && inside) {
                bool covered = false;
#pragma unroll 8
                for (int a = nr; a < nr_new; ++a) covered |= packed_covers(s_buf[a], S, hw, dq.cx, dq.cy);
                alive = !covered;
            }
            nr = nr_new;
        }
        __syncthreads();
    }
    return nr;
}

__device__ __forceinline__ void trk_discs_body(const Bufs& B, const Shape& S) {
    __shared__ uint32_t s_buf[2 * kMaxFeatures];       // the counts for the rank sort, then the raster's discs packed
    __shared__ int32_t s_hw[kHwLds];
    __shared__ int32_t wcount[TK_WAVES];
    __shared__ int32_t s_nr[2];
    Ctl* c = B.ctl;
    const int tid = threadIdx.x;
    if (c->lost || c->corner_args[1] <= 0) return;     // no mask is made (Tracker.cpp:303, :325); n_list and the raster count are 0
    const int n_kept = min(c->n_kept, S.M), n_blk = min(c->n_blocked, S.M);
    const int hw_len = S.r_track + S.r_blocked + 2;
    const bool hw_in_lds = hw_len <= kHwLds;
    if (hw_in_lds)
        for (int i = tid; i < hw_len; i += TK_T) s_hw[i] = B.hw[i];
    // ---- the tracked words that have a count, by count descending, equal counts in id order
    int32_t* s_cnt = reinterpret_cast<int32_t*>(s_buf);
    for (int i = tid; i < n_kept; i += TK_T) s_cnt[i] = B.row_cnt[i];
    __syncthreads();
    int n_counted = 0;
    for (int c0 = 0; c0 < n_kept; c0 += TK_T) {
        const int i = c0 + tid;
        const int32_t mine = i < n_kept ? s_cnt[i] : 0;
        int total;
        (void)wg_offset(mine > 0, wcount, total);
        n_counted += total;
        if (mine > 0) {
            int rank = 0;
#pragma unroll 8
            for (int j = 0; j < n_kept; ++j) {
                const int32_t other = s_cnt[j];
                rank += (other > 0 && drawn_before(other, j, mine, i)) ? 1 : 0;
            }
            const float x = B.row_xy[2 * i], y = B.row_xy[2 * i + 1];
            B.list[rank] = visfs_corners_disc{ x, y, S.r_track };
            B.packed[rank] = pack_disc(round_centre(x), round_centre(y), 0);
        }
    }
    for (int b = tid; b < n_blk; b += TK_T) {                                     // then the blocked words (:135)
        const float x = B.blk_xy[2 * b], y = B.blk_xy[2 * b + 1];
        const int o = n_counted + b;
        B.list[o] = visfs_corners_disc{ x, y, S.r_blocked };
        B.packed[o] = pack_disc(round_centre(x), round_centre(y), 1);
    }
    const int n_list = n_counted + n_blk;
    __threadfence_block();
    __syncthreads();
    const int nr = hw_in_lds ? draw_decision(B, S, (const int32_t*)s_hw, n_list, s_buf, s_nr) : draw_decision(B, S, B.hw, n_list, s_buf, s_nr);
    if (tid == 0) { c->n_list = n_list; c->corner_args[0] = nr; }
}

__global__ __launch_bounds__(TK_T) void k_trk_discs_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    trk_discs_body(r.B, S);
}

// BOOT: the 3-D points of bootstrapped words: one forward pass previous left -> previous right, no reverse pass, no gate, the status
// not looked at (Tracker.cpp:207-219).  Otherwise: the stereo pass of the frame with its gate, the bounds test of :376 and the
// finite test of :390.
template <bool BACK, bool BOOT>
__global__ __launch_bounds__(64) void k_trk_stereo_g(const TrkRec* __restrict__ recs, Shape S, LkParams prm, Layout lay, float gate) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip || (BOOT && !r.boot)) return;
    const Bufs& B = r.B;
    const Image* im = BOOT ? r.prev : r.cur;
    const Image &I = im[0], &J = im[1];
    const Camera& cam = r.cam;
    const int p = blockIdx.x;
    const Ctl* c = B.ctl;
    const int n = BOOT ? c->n_from : (c->lost ? 0 : c->n_rows);
    if (p >= min(n, S.M)) return;
    WaveCells pol{ (int)threadIdx.x };
    const float* pts = BOOT ? B.from_xy : B.row_xy;
    const float ptx = pts[2 * p], pty = pts[2 * p + 1];
    float tox, toy, err;
    uint8_t st;
    lk_gated(pol, prm, lay, I, J, ptx, pty, false, 0.0f, 0.0f, BACK, gate, tox, toy, st, err);
    if (threadIdx.x != 0) return;
    float xyz[3] = { __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("") };
    if (BOOT) {
        triangulate(cam, ptx, pty, tox, xyz);
        B.from_xyz[3 * p] = xyz[0]; B.from_xyz[3 * p + 1] = xyz[1]; B.from_xyz[3 * p + 2] = xyz[2];
    } else {
        if (st) triangulate(cam, ptx, pty, tox, xyz);
        B.row_rxy[2 * p] = tox; B.row_rxy[2 * p + 1] = toy;
        B.row_xyz[3 * p] = xyz[0]; B.row_xyz[3 * p + 1] = xyz[1]; B.row_xyz[3 * p + 2] = xyz[2];
        B.row_st[p] = st;
        B.row_ok[p] = stereo_row(st, tox, toy, xyz, S.w, S.h) ? 1 : 0;
    }
}

__global__ __launch_bounds__(TK_T) void k_trk_finish_g(const TrkRec* __restrict__ recs, Shape S) {
    const TrkRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const Bufs& B = r.B;
    const int boot = r.boot;
    __shared__ int32_t wcount[TK_WAVES];
    Ctl* c = B.ctl;
    const int tid = threadIdx.x;
    const bool lost = c->lost != 0;
    const int n = lost ? 0 : min(c->n_rows, S.M);
    int words = 0;
    for (int c0 = 0; c0 < n; c0 += TK_T) {
        const int i = c0 + tid;
        const bool keep = i < n && B.row_ok[i] != 0;
        int total;
        const int o = words + wg_offset(keep, wcount, total);
        if (keep) {
            const uint64_t id = B.row_id[i];
            const int32_t cnt = B.row_cnt[i] + 1;                                 // updateTrackCounter (:98-114)
            B.tab_id[o] = id; B.o.w_id[o] = id;
            B.tab_cnt[o] = cnt; B.o.w_cnt[o] = cnt;
            for (int k = 0; k < 2; ++k) {
                B.tab_xy[2 * o + k] = B.row_xy[2 * i + k]; B.o.w_l[2 * o + k] = B.row_xy[2 * i + k];
                B.o.w_r[2 * o + k] = B.row_rxy[2 * i + k];
            }
            for (int k = 0; k < 3; ++k) { B.tab_xyz[3 * o + k] = B.row_xyz[3 * i + k]; B.o.w_xyz[3 * o + k] = B.row_xyz[3 * i + k]; }
        }
        words += total;
    }
    if (tid == 0) {
        c->n_tab = words;
        Head hd;
        hd.flags = lost ? kLost : (boot ? kBootstrapped : 0);
        hd.n_covis = lost ? 0 : c->n_kept;
        hd.n_new = lost ? 0 : c->n_new;
        hd.n_words = words;
        hd.n_blocked = lost ? 0 : c->n_blocked;
        hd.pad = 0;
        hd.next_id = c->next_id;
        *B.o.head = hd;
    }
}

}  // namespace trk

// ---------------------------------------------------------------- the objects
// The tables of a call for n members stand in one block, pinned and on the device, and go up in one copy:
// [PyrRec n][ClaheRec n][CornerRec n: bootstrap][CornerRec n: top-up][TrkRec n][CullRec n][PnpRec n][InHead n][outlier ids of the
// members, one behind the other]
struct CallBlock {
    PinnedBuf<char> pinned; DeviceBuf<char> dev;
    size_t off_pyr = 0, off_clahe = 0, off_boot = 0, off_top = 0, off_trk = 0, off_cull = 0, off_pnp = 0, off_in = 0, off_ids = 0, bytes = 0;

    template <class S> int allocate(S sink, size_t n) {       // the caller has selected the device
        size_t off = 0;
        const auto take = [&](size_t b) { const size_t at = off; off = (off + b + 255) & ~size_t(255); return at; };
        off_pyr = take(n * sizeof(PyrRec));
        off_clahe = take(n * sizeof(ClaheRec));
        off_boot = take(n * sizeof(CornerRec));
        off_top = take(n * sizeof(CornerRec));
        off_trk = take(n * sizeof(TrkRec));
        off_cull = take(n * sizeof(fund::CullRec));
        off_pnp = take(n * sizeof(pnp::PnpRec));
        off_in = take(n * sizeof(InHead));
        off_ids = take(n * sizeof(uint64_t) * kMaxOutliers);
        bytes = off;
        RC_TRY(dev.alloc(sink, bytes));
        RC_TRY(pinned.alloc(sink, bytes));
        std::memset(pinned.get(), 0, bytes);
        return VISFS_BA_OK;
    }
};

struct visfs_tracker {
    visfs_flow* f = nullptr;                   // nullptr once the flow object is gone
    visfs_tracker_params prm{};
    visfs_flow_camera cam{};
    Shape S{};
    bool cull_on = false;                      // cull set and the flow object's flow_back off (Tracker.cpp:275)
    fund::CullShape cull{};
    std::string err;
    int seen_frames = 0;                       // f->frames after this tracker's last push
    bool have_call = false;                    // the download hook has something to report
    bool boot_last = false;
    std::vector<uint64_t> ids;                 // the table's ids as the last call returned them
    std::vector<int32_t> hw;                   // half-widths of min_distance, then of min_distance / 2

    // host restatement: the same blocks in host memory
    std::vector<char> h_work, h_outblk, h_inblk;
    // device
    struct Owned {                             // gone with the flow object (free_device), which the tracker may outlive
        DeviceBuf<char> d_work, d_out;
        PinnedBuf<char> p_out;
        DeviceBuf<char> d_pnp;                 // the pose guess: rows, winner key, hypotheses, passes
        CallBlock blk;                         // the tables of a single call: a group of one
    } own;
    size_t out_bytes = 0;

    Bufs B{};                                  // where the kernels (or the host steps) work
    Out R{};                                   // where the caller reads: the pinned copy, or the host twin's block itself

    visfs_tracker_group* group = nullptr;      // the tracker group this is a member of

    // the pose guess (include/visfs_tracker_pnp.h)
    bool pnp_on = false;
    bool called = false;                       // a process call has completed: visfs_tracker_pnp_last has something to report
    visfs_pnp_params pnp_prm{};
    visfs_pnp_camera pnp_cam{};
    pnp::PnpShape pnp_shape{};
    pnp::PnpRec pnp_rec{};                     // device: where the stages work
    size_t out_base_bytes = 0;                 // the output block of a tracker without the pose guess; what a call brings down with it off
    visfs_pnp* pnp_host = nullptr;             // host twin: the staged host solver its steps run on
    visfs_tracker_pnp_result pnp_res{};
    int32_t pnp_last_m = 0, pnp_last_hyp = 0, pnp_last_passes = 0;
    pnp::Result pnp_model{};
    std::vector<int32_t> pnp_matches, pnp_inliers, pnp_list;
    std::vector<float> pnp_to_xyz;
    std::vector<pnp::Row> pnp_rows;
    std::unordered_map<uint64_t, int32_t> pnp_index;
};

// n trackers processed by one call (include/visfs_tracker_group.h)
struct visfs_tracker_group {
    std::vector<visfs_tracker*> m;             // nullptr: the member has been destroyed
    bool device = false;
    std::string err;
    GroupCounts cnt;
    int dev = 0;
    hipStream_t stream = nullptr;
    CallBlock blk;                             // the tables of a call of all members

    ~visfs_tracker_group() {                   // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

Camera make_camera(const visfs_flow_params& p, const visfs_flow_camera& c) {
    Camera k;
    k.fx = c.fx; k.fy = c.fy; k.cx = c.cx; k.cy = c.cy; k.cx_right = c.cx_right; k.baseline = c.baseline;
    k.min_depth = p.min_depth; k.max_depth = p.max_depth;
    for (int i = 0; i < 12; ++i) k.T[i] = c.Tir[i];
    return k;
}

void free_device(visfs_tracker* t) {
    visfs_flow* f = t->f;
    if (!f || !f->device) return;
    (void)hipSetDevice(f->dev);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    t->own = visfs_tracker::Owned();
}

int allocate(visfs_tracker* t) {
    visfs_flow* f = t->f;
    const size_t M = (size_t)t->S.M;
    Bufs& B = t->B;
    int32_t* hw = nullptr;
    const size_t H = t->cull_on ? (size_t)t->cull.iterations : 0;
    const size_t work_bytes = carve_work(nullptr, M, t->hw.size(), H, B, &hw);
    t->out_bytes = t->out_base_bytes = carve_out(nullptr, M, false, B.o);
    if (!f->device) {
        t->h_work.assign(work_bytes, 0); t->h_outblk.assign(t->out_bytes, 0);
        t->h_inblk.assign(sizeof(InHead) + sizeof(uint64_t) * kMaxOutliers, 0);
        carve_work(t->h_work.data(), M, t->hw.size(), H, B, &hw);
        carve_out(t->h_outblk.data(), M, false, B.o);
        std::memcpy(hw, t->hw.data(), t->hw.size() * sizeof(int32_t));
        B.in = reinterpret_cast<const InHead*>(t->h_inblk.data());
        B.outliers = reinterpret_cast<const uint64_t*>(t->h_inblk.data() + sizeof(InHead));
        t->R = B.o;
        return VISFS_BA_OK;
    }
    HIP_TRY(t, hipSetDevice(f->dev));
    RC_TRY(t->own.d_work.alloc(t, work_bytes));
    RC_TRY(t->own.d_out.alloc(t, t->out_bytes));
    RC_TRY(t->own.p_out.alloc(t, t->out_bytes));
    RC_TRY(t->own.blk.allocate(t, 1));
    carve_work(t->own.d_work.get(), M, t->hw.size(), H, B, &hw);
    carve_out(t->own.d_out.get(), M, false, B.o);
    carve_out(t->own.p_out.get(), M, false, t->R);              // (B.in and B.outliers of a call point into the block the call goes through)
    std::memset(t->own.p_out.get(), 0, t->out_bytes);
    HIP_TRY(t, hipMemsetAsync(t->own.d_work.get(), 0, work_bytes, f->stream));
    HIP_TRY(t, hipMemsetAsync(t->own.d_out.get(), 0, t->out_bytes, f->stream));
    HIP_TRY(t, hipMemcpyAsync(hw, t->hw.data(), t->hw.size() * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(t, hipStreamSynchronize(f->stream));                        // t->hw may move; nothing else waits here
    return VISFS_BA_OK;
}

int check_params(const visfs_tracker_params* p, const visfs_flow_camera* cam, const char** why) {
    if (p->max_features < 1) { *why = "max_features must be at least 1"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p->max_features > kMaxFeatures) { *why = "max_features must not exceed 4096"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (!std::isfinite(p->quality_level) || !(p->quality_level > 0.0)) { *why = "quality_level must be finite and positive"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p->min_distance < 0) { *why = "min_distance must not be negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p->min_distance > kMaxRadius) { *why = "min_distance must not exceed 32768"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (p->min_inliers < 0) { *why = "min_inliers must not be negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(cam->Tir[i])) { *why = "Tir is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p->cull) {
        if (!std::isfinite(p->cull_params.pixel_error)) { *why = "cull_params.pixel_error is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        if (p->cull_params.iterations < 1) { *why = "cull_params.iterations must be at least 1"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        if (p->cull_params.iterations > fund::kMaxHypotheses) { *why = "cull_params.iterations above 4096"; return VISFS_BA_ERR_UNSUPPORTED; }
    }
    return VISFS_BA_OK;
}

// ---------------------------------------------------------------- host restatement: the kernels' steps on one core
void host_pretreat(visfs_tracker* t) {
    Bufs& B = t->B;
    Ctl* c = B.ctl;
    const std::unordered_set<uint64_t> out(B.outliers, B.outliers + B.in->n_outliers);
    int nk = 0, nb = 0;
    for (int i = 0; i < c->n_tab; ++i) {
        const uint64_t id = B.tab_id[i];
        if (out.count(id)) {
            B.o.blk_id[nb] = id; B.blk_xy[2 * nb] = B.tab_xy[2 * i]; B.blk_xy[2 * nb + 1] = B.tab_xy[2 * i + 1];
            ++nb;
        } else {
            B.from_id[nk] = id; B.from_cnt[nk] = B.tab_cnt[i];
            for (int k = 0; k < 2; ++k) B.from_xy[2 * nk + k] = B.tab_xy[2 * i + k];
            for (int k = 0; k < 3; ++k) B.from_xyz[3 * nk + k] = B.tab_xyz[3 * i + k];
            ++nk;
        }
    }
    c->n_from = nk; c->n_blocked = nb;
    c->n_kept = 0; c->lost = 0; c->n_list = 0; c->n_new = 0; c->n_rows = 0;
    c->corner_args[0] = c->corner_args[1] = 0;
    c->cull_m = 0;
    c->pnp_m = 0;
}

Image host_image(const visfs_flow* f, int slot, int image) { return Image{ f->hpx[slot][image].data(), f->hder[slot][image].data() }; }

int host_bootstrap(visfs_tracker* t) {
    visfs_flow* f = t->f;
    Bufs& B = t->B;
    Ctl* c = B.ctl;
    const int prev = 1 - f->cur;
    std::vector<float> xy(2 * (size_t)t->S.M);
    int32_t n = 0;
    const int rc = corners_host(f, f->hpx[prev][0].data(), t->S.M, t->prm.quality_level, (double)t->prm.min_distance, nullptr, 0, nullptr,
                                xy.data(), &n);
    if (rc != VISFS_BA_OK) return fail(t, rc, f->err);
    const Camera cam = make_camera(f->prm, t->cam);
    const Image I = host_image(f, prev, 0), J = host_image(f, prev, 1);
    const HostCells pol;
    for (int a = 0; a < n; ++a) {
        B.from_id[a] = c->next_id + (uint64_t)a; B.from_cnt[a] = 0;
        B.from_xy[2 * a] = xy[2 * a]; B.from_xy[2 * a + 1] = xy[2 * a + 1];
        float tx, ty, e;
        uint8_t st;
        lk_gated(pol, f->lk, f->lay, I, J, xy[2 * a], xy[2 * a + 1], false, 0.0f, 0.0f, false, 0.0f, tx, ty, st, e);
        triangulate(cam, xy[2 * a], xy[2 * a + 1], tx, B.from_xyz + 3 * a);
    }
    c->next_id += (uint64_t)n;
    c->n_from = n;
    return VISFS_BA_OK;
}

void host_track_reduce(visfs_tracker* t, const Guess* g) {
    visfs_flow* f = t->f;
    Bufs& B = t->B;
    Ctl* c = B.ctl;
    const Shape& S = t->S;
    const Image I = host_image(f, 1 - f->cur, 0), J = host_image(f, f->cur, 0);
    const HostCells pol;
    for (int p = 0; p < c->n_from; ++p) {
        const float ptx = B.from_xy[2 * p], pty = B.from_xy[2 * p + 1];
        float inx = ptx, iny = pty;
        if (g) project_guess(*g, B.from_xyz + 3 * p, inx, iny);
        float tx, ty, e;
        uint8_t st;
        lk_gated(pol, f->lk, f->lay, I, J, ptx, pty, g != nullptr, inx, iny, f->prm.flow_back != 0, f->prm.back_gate_track, tx, ty, st, e);
        B.guess[2 * p] = inx; B.guess[2 * p + 1] = iny;
        B.to[2 * p] = tx; B.to[2 * p + 1] = ty;
        B.lk_st[p] = st;
        B.inb[p] = (in_bounds(tx, S.w) && in_bounds(ty, S.h)) ? 1 : 0;
    }
    if (t->cull_on) fund::cull_host(B.cull, B.from_xy, B.to, B.lk_st, c->n_from, t->cull);     // Tracker.cpp:275-277
    int kept = 0;
    for (int p = 0; p < c->n_from; ++p) {
        const float tx = B.to[2 * p], ty = B.to[2 * p + 1];
        if (!kept_row(B.keep_st[p], tx, ty, S.w, S.h)) continue;
        const int o = kept++;
        B.o.cov_id[o] = B.from_id[p];
        for (int k = 0; k < 2; ++k) B.o.cov_from[2 * o + k] = B.from_xy[2 * p + k];
        for (int k = 0; k < 3; ++k) B.o.cov_xyz[3 * o + k] = B.from_xyz[3 * p + k];
        B.o.cov_to[2 * o] = tx; B.o.cov_to[2 * o + 1] = ty;
        B.row_id[o] = B.from_id[p]; B.row_xy[2 * o] = tx; B.row_xy[2 * o + 1] = ty; B.row_cnt[o] = B.from_cnt[p];
    }
    const bool lost = kept < S.min_inliers;
    c->n_kept = kept; c->n_rows = lost ? 0 : kept; c->lost = lost ? 1 : 0;
    c->corner_args[1] = lost ? 0 : S.M - kept;
}

void host_discs(visfs_tracker* t) {
    Bufs& B = t->B;
    Ctl* c = B.ctl;
    const Shape& S = t->S;
    if (c->lost || c->corner_args[1] <= 0) return;
    std::vector<int32_t> order;
    for (int i = 0; i < c->n_kept; ++i)
        if (B.row_cnt[i] > 0) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return drawn_before(B.row_cnt[a], a, B.row_cnt[b], b); });
    int n = 0;
    for (int32_t i : order) { B.list[n] = visfs_corners_disc{ B.row_xy[2 * i], B.row_xy[2 * i + 1], S.r_track }; B.packed[n++] = 0; }
    for (int b = 0; b < c->n_blocked; ++b) { B.list[n] = visfs_corners_disc{ B.blk_xy[2 * b], B.blk_xy[2 * b + 1], S.r_blocked }; B.packed[n++] = 1; }
    int nr = 0;
    for (int i = 0; i < n; ++i) {
        const int kind = (int)B.packed[i];
        const Disc d{ round_centre(B.list[i].x), round_centre(B.list[i].y), kind ? S.r_blocked : S.r_track, kind ? S.r_track + 1 : 0 };
        B.drawn[i] = 0;
        if (centre_inside(d.cx, d.cy, S.w, S.h) && masked(B.raster, nr, B.hw, d.cx, d.cy)) continue;
        B.drawn[i] = 1;
        if (touches_image(d, S.w, S.h)) B.raster[nr++] = d;
    }
    c->n_list = n; c->corner_args[0] = nr;
}

int host_topup_stereo_finish(visfs_tracker* t, bool boot) {
    visfs_flow* f = t->f;
    Bufs& B = t->B;
    Ctl* c = B.ctl;
    const Shape& S = t->S;
    if (!c->lost) {
        std::vector<float> xy(2 * (size_t)S.M);
        int32_t n = 0;
        const int rc = corners_host(f, f->hpx[f->cur][0].data(), c->corner_args[1], t->prm.quality_level, (double)t->prm.min_distance, B.raster,
                                    c->corner_args[0], B.hw, xy.data(), &n);
        if (rc != VISFS_BA_OK) return fail(t, rc, f->err);
        for (int a = 0; a < n; ++a) {
            const int r = c->n_kept + a;
            const uint64_t id = c->next_id + (uint64_t)a;
            B.row_id[r] = id; B.row_xy[2 * r] = xy[2 * a]; B.row_xy[2 * r + 1] = xy[2 * a + 1]; B.row_cnt[r] = 0;
            B.o.new_id[a] = id; B.o.new_xy[2 * a] = xy[2 * a]; B.o.new_xy[2 * a + 1] = xy[2 * a + 1];
        }
        c->next_id += (uint64_t)n;
        c->n_new = n; c->n_rows = c->n_kept + n;
        const Camera cam = make_camera(f->prm, t->cam);
        const Image I = host_image(f, f->cur, 0), J = host_image(f, f->cur, 1);
        const HostCells pol;
        for (int p = 0; p < c->n_rows; ++p) {
            const float ptx = B.row_xy[2 * p], pty = B.row_xy[2 * p + 1];
            float tx, ty, e;
            uint8_t st;
            lk_gated(pol, f->lk, f->lay, I, J, ptx, pty, false, 0.0f, 0.0f, f->prm.flow_back != 0, f->prm.back_gate_stereo, tx, ty, st, e);
            float* xyz = B.row_xyz + 3 * p;
            xyz[0] = xyz[1] = xyz[2] = __builtin_nanf("");
            if (st) triangulate(cam, ptx, pty, tx, xyz);
            B.row_rxy[2 * p] = tx; B.row_rxy[2 * p + 1] = ty;
            B.row_st[p] = st;
            B.row_ok[p] = stereo_row(st, tx, ty, xyz, S.w, S.h) ? 1 : 0;
        }
    }
    const bool lost = c->lost != 0;
    int words = 0;
    for (int i = 0; i < (lost ? 0 : c->n_rows); ++i) {
        if (!B.row_ok[i]) continue;
        const int o = words++;
        const int32_t cnt = B.row_cnt[i] + 1;
        B.tab_id[o] = B.o.w_id[o] = B.row_id[i];
        B.tab_cnt[o] = B.o.w_cnt[o] = cnt;
        for (int k = 0; k < 2; ++k) { B.tab_xy[2 * o + k] = B.o.w_l[2 * o + k] = B.row_xy[2 * i + k]; B.o.w_r[2 * o + k] = B.row_rxy[2 * i + k]; }
        for (int k = 0; k < 3; ++k) B.tab_xyz[3 * o + k] = B.o.w_xyz[3 * o + k] = B.row_xyz[3 * i + k];
    }
    c->n_tab = words;
    Head hd;
    hd.flags = lost ? kLost : (boot ? kBootstrapped : 0);
    hd.n_covis = lost ? 0 : c->n_kept; hd.n_new = lost ? 0 : c->n_new; hd.n_words = words; hd.n_blocked = lost ? 0 : c->n_blocked;
    hd.pad = 0; hd.next_id = c->next_id;
    *B.o.head = hd;
    return VISFS_BA_OK;
}

void clear_result(visfs_tracker* t, visfs_tracker_result* r, int32_t flags, uint64_t next_id) {
    std::memset(r, 0, sizeof(*r));
    r->flags = flags; r->next_id = next_id;
    const Out& o = t->R;
    r->covisible_id = o.cov_id; r->covisible_from_xy = o.cov_from; r->covisible_from_xyz = o.cov_xyz; r->covisible_to_xy = o.cov_to;
    r->new_id = o.new_id; r->new_xy = o.new_xy;
    r->word_id = o.w_id; r->word_left_xy = o.w_l; r->word_right_xy = o.w_r; r->word_xyz = o.w_xyz; r->word_count = o.w_cnt;
    r->blocked_id = o.blk_id;
}

void leave_group(visfs_tracker* t) {
    if (!t->group) return;
    for (visfs_tracker*& m : t->group->m)
        if (m == t) m = nullptr;
    t->group = nullptr;
}

// the argument checks of a call; nothing has been pushed or changed when one fails
int check_call(visfs_tracker* t, const uint8_t* left, const uint8_t* right, int32_t stride, const double* delta_guess, int32_t n_outliers,
               const uint64_t* outlier_ids, const visfs_tracker_result* result) {
    visfs_flow* f = t->f;
    if (!f) return fail(t, VISFS_BA_ERR_NOT_LOADED, "the flow object of this tracker is gone");
    if (!left || !right || !result) return fail(t, VISFS_BA_ERR_BAD_ARGUMENT, "a NULL argument");
    if (stride < f->w) return fail(t, VISFS_BA_ERR_BAD_ARGUMENT, "stride is smaller than the image width");
    if (n_outliers < 0 || n_outliers > kMaxOutliers) return fail(t, VISFS_BA_ERR_BAD_ARGUMENT, "n_outliers must lie in 0 .. 4096");
    if (n_outliers > 0 && !outlier_ids) return fail(t, VISFS_BA_ERR_BAD_ARGUMENT, "outlier_ids is NULL");
    if (delta_guess)
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(delta_guess[i])) return fail(t, VISFS_BA_ERR_BAD_ARGUMENT, "delta_guess is not finite");
    if (f->frames != t->seen_frames)
        return fail(t, VISFS_BA_ERR_NOT_LOADED, "the images of the flow object were pushed by another caller since this tracker's last call");
    return VISFS_BA_OK;
}

// what the table will hold after pretreatment is known from the ids handed out last (Tracker.cpp:143-165)
int32_t remaining_rows(const visfs_tracker* t, int32_t n_outliers, const uint64_t* outlier_ids) {
    const std::unordered_set<uint64_t> out(outlier_ids, outlier_ids + n_outliers);
    int32_t remaining = 0;
    for (uint64_t id : t->ids) remaining += out.count(id) ? 0 : 1;
    return remaining;
}

// the output block of a finished call into the caller's result and the tracker's id list
int take_result(visfs_tracker* t, bool boot, visfs_tracker_result* result) {
    const Head hd = *t->R.head;
    if (hd.n_covis < 0 || hd.n_covis > t->S.M || hd.n_new < 0 || hd.n_new > t->S.M || hd.n_words < 0 || hd.n_words > t->S.M ||
        hd.n_blocked < 0 || hd.n_blocked > t->S.M) {
        t->ids.clear();
        return fail(t, VISFS_BA_ERR_DEVICE, "the call returned an impossible count");
    }
    clear_result(t, result, hd.flags, hd.next_id);
    result->n_covisible = hd.n_covis; result->n_new = hd.n_new; result->n_words = hd.n_words; result->n_blocked = hd.n_blocked;
    t->ids.assign(t->R.w_id, t->R.w_id + hd.n_words);
    t->have_call = true;
    t->boot_last = boot;
    return VISFS_BA_OK;
}

// ---------------------------------------------------------------- the pose guess behind a call (include/visfs_tracker_pnp.h)
void pnp_clear(visfs_tracker* t, int ran) {
    visfs_tracker_pnp_result& r = t->pnp_res;
    r.ran = ran; r.n_matches = 0; r.n_inliers = 0; r.pad = 0;
    r.matches = t->pnp_matches.data(); r.inliers = t->pnp_inliers.data();
    for (int i = 0; i < 16; ++i) r.T[i] = 0.0;
    for (int i = 0; i < 36; ++i) r.cov[i] = (i % 7 == 0) ? 1.0 : 0.0;
    t->pnp_last_m = t->pnp_last_hyp = t->pnp_last_passes = 0;
    t->pnp_model = pnp::Result{};
    t->pnp_model.winner = -1;
}

// The result of the pose guess from the output block of a finished call (take_result has checked its counts).  to_xyz is matched by
// id from the call's words, as visfs_amd/host/MotionEstimator.h builds it from its maps; the transform and the covariance are the
// host's in both flavours (pnp::finalize).  A host-twin tracker runs the staged host solver on the rows.
int pnp_finish(visfs_tracker* t) {
    pnp_clear(t, 1);
    visfs_tracker_pnp_result& r = t->pnp_res;
    const Out& o = t->R;
    const Head hd = *o.head;
    const int32_t n = hd.n_covis;
    const float* to_xyz = nullptr;
    if (hd.n_words > 0) {                                              // MultiviewGeometry.cpp:160 tests _words3dTo.size()
        t->pnp_index.clear();
        for (int32_t k = 0; k < hd.n_words; ++k) t->pnp_index.emplace(o.w_id[k], k);
        for (int32_t i = 0; i < n; ++i) {
            const auto it = t->pnp_index.find(o.cov_id[i]);
            for (int k = 0; k < 3; ++k)
                t->pnp_to_xyz[3 * (size_t)i + k] = it == t->pnp_index.end() ? __builtin_nanf("") : o.w_xyz[3 * (size_t)it->second + k];
        }
        to_xyz = t->pnp_to_xyz.data();
    }
    if (!t->f->device) {
        const int rc = visfs_pnp_solve(t->pnp_host, &t->pnp_prm, &t->pnp_cam, n, o.cov_xyz, o.cov_to, to_xyz, r.T, r.cov, t->pnp_matches.data(),
                                       &r.n_matches, t->pnp_inliers.data(), &r.n_inliers);
        if (rc != VISFS_BA_OK) { pnp_clear(t, 0); return fail(t, rc, std::string("the pose guess: ") + visfs_pnp_last_error(t->pnp_host)); }
        return VISFS_BA_OK;
    }
    const int32_t m = *o.p_m;
    const pnp::Result res = *o.p_res;
    const int32_t min_inliers = t->pnp_shape.min_inliers;
    bool sane = m >= 0 && m <= n;
    for (int32_t k = 0; sane && k < m; ++k) sane = o.p_match[k] >= 0 && o.p_match[k] < n;
    const bool searched = sane && m >= min_inliers;
    if (searched) sane = res.n_inliers >= 0 && res.n_inliers <= m && res.n_passes >= 0 && res.n_passes <= pnp::kMaxRefine;
    for (int32_t k = 0; sane && searched && k < res.n_inliers; ++k) sane = o.p_inl[k] >= 0 && o.p_inl[k] < m;
    if (!sane) { pnp_clear(t, 0); return fail(t, VISFS_BA_ERR_DEVICE, "the pose guess returned an impossible count or row number"); }
    std::copy(o.p_match, o.p_match + m, t->pnp_matches.begin());
    r.n_matches = m;
    t->pnp_last_m = m;
    if (!searched) return VISFS_BA_OK;
    t->pnp_last_hyp = t->pnp_shape.iterations; t->pnp_last_passes = res.n_passes;
    t->pnp_model = res;
    if (res.n_inliers < min_inliers) return VISFS_BA_OK;
    for (int32_t k = 0; k < m; ++k) {
        const size_t i = (size_t)o.p_match[k];
        t->pnp_rows[(size_t)k] = pnp::Row{ o.cov_xyz[3 * i], o.cov_xyz[3 * i + 1], o.cov_xyz[3 * i + 2], o.cov_to[2 * i], o.cov_to[2 * i + 1] };
    }
    std::copy(o.p_inl, o.p_inl + res.n_inliers, t->pnp_list.begin());
    const pnp::Cam K{ t->pnp_cam.fx, t->pnp_cam.fy, t->pnp_cam.cx, t->pnp_cam.cy };
    pnp::finalize(res, t->pnp_rows.data(), t->pnp_cam.Tir, K, t->pnp_list.data(), (size_t)res.n_inliers, t->pnp_matches.data(), to_xyz, r.T, r.cov);
    r.n_inliers = res.n_inliers;
    for (int32_t k = 0; k < res.n_inliers; ++k) t->pnp_inliers[(size_t)k] = t->pnp_matches[(size_t)t->pnp_list[(size_t)k]];
    return VISFS_BA_OK;
}

struct MemberPlan {                            // what the host decides for a member before anything is pushed
    bool no_previous, boot, has_guess;
    int32_t from_bound;                        // rows the tracking launch must cover
    int slot;                                  // where the pair goes
    Guess g;
};

MemberPlan plan_member(const visfs_tracker* t, const double* delta_guess, int32_t n_outliers, const uint64_t* outlier_ids) {
    const visfs_flow* f = t->f;
    MemberPlan P;
    const int32_t remaining = remaining_rows(t, n_outliers, outlier_ids);
    P.boot = remaining == 0;                   // (a bootstrapped table is never empty where corners exist: Tracker.cpp:238)
    P.no_previous = f->frames == 0;            // Tracker.cpp:168
    P.from_bound = P.boot ? t->S.M : remaining;
    P.slot = f->frames == 0 ? f->cur : 1 - f->cur;
    P.has_guess = delta_guess != nullptr;
    P.g = Guess{};
    if (P.has_guess) {
        guess_camera_ref(delta_guess, t->cam.Tir, P.g);
        P.g.fx = (double)t->cam.fx; P.g.fy = (double)t->cam.fy; P.g.cx = (double)t->cam.cx; P.g.cy = (double)t->cam.cy;
    }
    return P;
}

// The books of a member after its call: the pair is in its slot (the host twin's push has moved the flow object on itself), the
// result goes to the caller.
int commit_member(visfs_tracker* t, const MemberPlan& P, visfs_tracker_result* result) {
    visfs_flow* f = t->f;
    if (f->device) {
        if (t->prm.clahe)
            group_clahe_pushed(f, clahe::make_geom(f->w, f->h, t->prm.clahe_params.tiles_x, t->prm.clahe_params.tiles_y,
                                                   t->prm.clahe_params.clip_limit));
        f->cur = P.slot;
        ++f->frames;
    }
    t->seen_frames = f->frames;
    t->called = true;
    pnp_clear(t, 0);
    if (P.no_previous) {
        clear_result(t, result, kNoPrevious, 0);
        t->have_call = false;
        return VISFS_BA_OK;
    }
    const int rc = take_result(t, P.boot, result);
    if (rc != VISFS_BA_OK || !t->pnp_on) return rc;
    return pnp_finish(t);
}

// ---------------------------------------------------------------- device: the launches of a call
struct CallFault { int member = -1; std::string why; };               // which member a failed call blames (-1: none), and why
void set_error(CallFault* fault, const std::string& text) { fault->member = -1; fault->why = text; }      // a sink of HIP_TRY

// A call of n members (equal shapes and parameters, one handle) through the block `blk` on `stream`; a single call is n = 1 through
// the tracker's own block.  Nothing here waits for a value read back: the one wait in front is for the pinned staging images and
// the pinned tables of the call before to have left, the one behind ends the call.
int run_call(visfs_tracker* const* m, int n, const visfs_tracker_frame* fr, const MemberPlan* plan, const CallBlock& blk, int device,
             hipStream_t stream, GroupCounts* cnt_out, CallFault* fault) {
    visfs_tracker* t0 = m[0];
    visfs_flow* f0 = t0->f;
    const Shape S = t0->S;
    const bool clahe_on = t0->prm.clahe != 0, back = f0->prm.flow_back != 0, cull_on = t0->cull_on, pnp_on = t0->pnp_on;
    const clahe::Geom geom = clahe_on ? clahe::make_geom(f0->w, f0->h, t0->prm.clahe_params.tiles_x, t0->prm.clahe_params.tiles_y,
                                                         t0->prm.clahe_params.clip_limit)
                                      : clahe::Geom{};
    GroupCounts& cnt = *cnt_out;
    const auto blame = [&](int rc, int member, const std::string& why) { fault->member = member; fault->why = why; return rc; };
    HIP_TRY(fault, hipSetDevice(device));
    HIP_TRY(fault, hipStreamSynchronize(stream));
    ++cnt.waits;
    PyrRec* pyr = reinterpret_cast<PyrRec*>(blk.pinned.get() + blk.off_pyr);
    ClaheRec* clr = reinterpret_cast<ClaheRec*>(blk.pinned.get() + blk.off_clahe);
    CornerRec* cboot = reinterpret_cast<CornerRec*>(blk.pinned.get() + blk.off_boot);
    CornerRec* ctop = reinterpret_cast<CornerRec*>(blk.pinned.get() + blk.off_top);
    TrkRec* trk = reinterpret_cast<TrkRec*>(blk.pinned.get() + blk.off_trk);
    fund::CullRec* cull = reinterpret_cast<fund::CullRec*>(blk.pinned.get() + blk.off_cull);
    pnp::PnpRec* pnr = reinterpret_cast<pnp::PnpRec*>(blk.pinned.get() + blk.off_pnp);
    InHead* inh = reinterpret_cast<InHead*>(blk.pinned.get() + blk.off_in);
    uint64_t* ids = reinterpret_cast<uint64_t*>(blk.pinned.get() + blk.off_ids);
    size_t n_ids = 0;
    bool any_active = false, any_boot = false;
    int32_t bound = 0;
    for (int i = 0; i < n; ++i) {
        visfs_tracker* t = m[i];
        visfs_flow* f = t->f;
        const MemberPlan& P = plan[i];
        const int cur = P.slot, prev = 1 - P.slot;
        int rc;
        if (clahe_on) {
            uint8_t* raw[2];
            group_clahe_fill(f, geom, cur, &clr[i], raw);
            rc = group_stage(f, raw, fr[i].left, fr[i].right, fr[i].stride, &cnt);
        } else {
            rc = group_stage(f, f->dpx[cur], fr[i].left, fr[i].right, fr[i].stride, &cnt);
        }
        if (rc != VISFS_BA_OK) return blame(rc, i, f->err);
        group_pyr_fill(f, cur, &pyr[i]);
        const bool skip = P.no_previous;
        TrkRec& r = trk[i];
        r.B = t->B;
        r.B.in = reinterpret_cast<const InHead*>(blk.dev.get() + blk.off_in) + i;
        r.B.outliers = reinterpret_cast<const uint64_t*>(blk.dev.get() + blk.off_ids) + n_ids;
        inh[i] = InHead{ fr[i].n_outliers, 0 };
        if (fr[i].n_outliers > 0) std::memcpy(ids + n_ids, fr[i].outlier_ids, sizeof(uint64_t) * (size_t)fr[i].n_outliers);
        n_ids += (size_t)fr[i].n_outliers;
        for (int k = 0; k < 2; ++k) {
            r.prev[k] = Image{ f->dpx[prev][k], f->dder[prev][k] };
            r.cur[k] = Image{ f->dpx[cur][k], f->dder[cur][k] };
        }
        r.cam = make_camera(f->prm, t->cam);
        r.g = P.g;
        r.has_guess = P.has_guess ? 1 : 0; r.skip = skip ? 1 : 0; r.boot = P.boot ? 1 : 0; r.pad = 0;
        cull[i] = t->B.cull;
        cull[i].skip = skip ? 1 : 0;
        pnr[i] = t->pnp_rec;
        pnr[i].skip = skip ? 1 : 0;
        // both extractions of a member work in the same state, one behind the other in stream order
        group_corners_fill(f, f->dpx[prev][0], nullptr, nullptr, t->B.ctl->boot_args, skip || !P.boot, &cboot[i], &r.corner_n, &r.corner_xy);
        group_corners_fill(f, f->dpx[cur][0], t->B.raster, t->B.hw, t->B.ctl->corner_args, skip, &ctop[i], &r.corner_n, &r.corner_xy);
        if (!skip) {
            any_active = true;
            any_boot = any_boot || P.boot;
            bound = std::max(bound, P.from_bound);
            t->have_call = false;
        }
    }
    HIP_TRY(fault, hipMemcpyAsync(blk.dev.get(), blk.pinned.get(), blk.off_ids + sizeof(uint64_t) * n_ids, hipMemcpyHostToDevice, stream));
    ++cnt.copies;
    const auto dev = [&](size_t off) { return blk.dev.get() + off; };
    int rc;
    if (clahe_on) {
        rc = group_clahe(f0, geom, n, reinterpret_cast<const ClaheRec*>(dev(blk.off_clahe)), &cnt);
        if (rc != VISFS_BA_OK) return blame(rc, -1, f0->err);
    }
    rc = group_pyramids(f0, n, reinterpret_cast<const PyrRec*>(dev(blk.off_pyr)), &cnt);
    if (rc != VISFS_BA_OK) return blame(rc, -1, f0->err);
    if (any_active) {
        const TrkRec* d_trk = reinterpret_cast<const TrkRec*>(dev(blk.off_trk));
        const unsigned z = (unsigned)n;
        const dim3 one(1, 1, z), rows((unsigned)S.M, 1, z), wg(TK_T), wave(64);
        const double quality = t0->prm.quality_level, min_distance = (double)t0->prm.min_distance;
#define RC_LAUNCH(kernel, grid, block, ...)                                                  \
    do {                                                                                     \
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                     \
        HIP_TRY(fault, hipGetLastError());                                                           \
        ++cnt.launches;                                                                       \
    } while (0)
        RC_LAUNCH(k_trk_pretreat_g, one, wg, d_trk, S);
        if (any_boot) {
            rc = group_corners(f0, quality, min_distance, n, reinterpret_cast<const CornerRec*>(dev(blk.off_boot)), &cnt);
            if (rc != VISFS_BA_OK) return blame(rc, -1, f0->err);
            RC_LAUNCH((k_trk_append_g<true>), one, wg, d_trk, S);
            RC_LAUNCH((k_trk_stereo_g<false, true>), rows, wave, d_trk, S, f0->lk, f0->lay, 0.0f);
        }
        if (bound > 0) {
            const dim3 grid((unsigned)bound, 1, z);
            if (back) RC_LAUNCH((k_trk_track_g<true>), grid, wave, d_trk, S, f0->lk, f0->lay, f0->prm.back_gate_track);
            else RC_LAUNCH((k_trk_track_g<false>), grid, wave, d_trk, S, f0->lk, f0->lay, f0->prm.back_gate_track);
        }
        if (cull_on) {                                                 // Tracker.cpp:275-277: between the forward pass and the reduce
            RC_LAUNCH(k_trk_cull_rows_g, one, wg, d_trk, S);
            rc = fund::group_cull(stream, n, reinterpret_cast<const fund::CullRec*>(dev(blk.off_cull)), S.M, t0->cull, &cnt);
            if (rc != VISFS_BA_OK) return blame(rc, -1, "a launch of the fundamental-matrix cull failed");
        }
        RC_LAUNCH(k_trk_reduce_g, one, wg, d_trk, S);
        if (pnp_on) {                                                  // the covisible rows exist; nothing behind this reads what it writes
            RC_LAUNCH(k_trk_pnp_rows_g, one, wg, d_trk, S);
            rc = pnp::group_pnp(stream, n, reinterpret_cast<const pnp::PnpRec*>(dev(blk.off_pnp)), t0->pnp_shape, &cnt);
            if (rc != VISFS_BA_OK) return blame(rc, -1, "a launch of the pose guess failed");
        }
        RC_LAUNCH(k_trk_discs_g, one, wg, d_trk, S);
        rc = group_corners(f0, quality, min_distance, n, reinterpret_cast<const CornerRec*>(dev(blk.off_top)), &cnt);
        if (rc != VISFS_BA_OK) return blame(rc, -1, f0->err);
        RC_LAUNCH((k_trk_append_g<false>), one, wg, d_trk, S);
        if (back) RC_LAUNCH((k_trk_stereo_g<true, false>), rows, wave, d_trk, S, f0->lk, f0->lay, f0->prm.back_gate_stereo);
        else RC_LAUNCH((k_trk_stereo_g<false, false>), rows, wave, d_trk, S, f0->lk, f0->lay, f0->prm.back_gate_stereo);
        RC_LAUNCH(k_trk_finish_g, one, wg, d_trk, S);
#undef RC_LAUNCH
        for (int i = 0; i < n; ++i) {
            if (plan[i].no_previous) continue;
            visfs_tracker* t = m[i];
            HIP_TRY(fault, hipMemcpyAsync(t->own.p_out.get(), t->own.d_out.get(), pnp_on ? t->out_bytes : t->out_base_bytes, hipMemcpyDeviceToHost, stream));
            ++cnt.copies;
        }
    }
    HIP_TRY(fault, hipStreamSynchronize(stream));
    ++cnt.waits;
    return VISFS_BA_OK;
}

void detach(visfs_tracker* t) {
    if (!t->f) return;
    free_device(t);
    if (t->f->trackers) {
        auto& l = t->f->trackers->list;
        l.erase(std::remove(l.begin(), l.end(), t), l.end());
    }
    t->f = nullptr;
}

}  // namespace

namespace flow {
void tracker_release(visfs_flow* f) {
    TrackerState* s = f->trackers;
    if (!s) return;
    const std::vector<visfs_tracker*> list = s->list;
    for (visfs_tracker* t : list) detach(t);
    delete s;
    f->trackers = nullptr;
}
}  // namespace flow

// ====================================================================== exported C ABI
extern "C" {

int visfs_tracker_abi_version(void) { return VISFS_TRACKER_ABI_VERSION; }

void visfs_tracker_default_params(visfs_tracker_params* p) {
    if (!p) return;
    p->max_features = 300; p->quality_level = 0.01; p->min_distance = 40; p->min_inliers = 10; p->clahe = 0;
    visfs_clahe_default_params(&p->clahe_params);
    p->cull = 0;
    visfs_fund_default_params(&p->cull_params);
}

int visfs_tracker_create(visfs_flow* f, const visfs_tracker_params* p, const visfs_flow_camera* cam, visfs_tracker** out) {
    if (!f || !p || !cam || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        const char* why = "";
        int rc = check_params(p, cam, &why);
        if (rc != VISFS_BA_OK) { f->err = why; return rc; }
        if (p->clahe) {
            int32_t dummy = 0;
            rc = visfs_clahe_hook_geometry(&p->clahe_params, f->w, f->h, &dummy, nullptr, nullptr, nullptr, nullptr);
            if (rc != VISFS_BA_OK) { f->err = "the CLAHE setting is not one the equalised push accepts"; return rc; }
        }
        if (f->w < 3 || f->h < 3) { f->err = "the image is smaller than 3 x 3"; return (int)VISFS_BA_ERR_BAD_ARGUMENT; }
        visfs_tracker* t = new visfs_tracker();
        t->f = f; t->prm = *p; t->cam = *cam;
        t->S = Shape{ p->max_features, f->w, f->h, p->min_distance, p->min_distance / 2, p->min_inliers };
        t->hw.resize((size_t)t->S.r_track + 1 + (size_t)t->S.r_blocked + 1);
        disc_halfwidth(t->S.r_track, t->hw.data());
        disc_halfwidth(t->S.r_blocked, t->hw.data() + t->S.r_track + 1);
        t->seen_frames = f->frames;
        t->cull_on = p->cull != 0 && f->prm.flow_back == 0;
        if (t->cull_on)
            t->cull = fund::CullShape{ p->cull_params.iterations, fund::cull_thr2(p->cull_params.pixel_error), p->cull_params.seed };
        rc = allocate(t);
        if (rc != VISFS_BA_OK) { f->err = t->err; free_device(t); delete t; return rc; }
        if (f->device) {                       // the states the call's records point into
            rc = group_corners_prepare(f);
            if (rc == VISFS_BA_OK && p->clahe) rc = group_clahe_prepare(f);
            if (rc != VISFS_BA_OK) { free_device(t); delete t; return rc; }
        }
        if (!f->trackers) f->trackers = new TrackerState();
        f->trackers->list.push_back(t);
        *out = t;
        return (int)VISFS_BA_OK;
    });
}

void visfs_tracker_destroy(visfs_tracker* t) {
    if (!t) return;
    leave_group(t);
    detach(t);
    if (t->pnp_host) visfs_pnp_destroy(t->pnp_host);
    delete t;
}

const char* visfs_tracker_last_error(const visfs_tracker* t) { return t ? t->err.c_str() : "null tracker"; }

int visfs_tracker_reset(visfs_tracker* t) {
    if (!t) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(t, [&]() -> int {
        if (!t->f) return fail(t, VISFS_BA_ERR_NOT_LOADED, "the flow object of this tracker is gone");
        t->ids.clear();
        if (!t->f->device) { t->B.ctl->n_tab = 0; return (int)VISFS_BA_OK; }
        HIP_TRY(t, hipSetDevice(t->f->dev));
        HIP_TRY(t, hipMemsetAsync(&t->B.ctl->n_tab, 0, sizeof(int32_t), t->f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_tracker_process(visfs_tracker* t, const uint8_t* left, const uint8_t* right, int32_t stride, const double* delta_guess,
                          int32_t n_outliers, const uint64_t* outlier_ids, visfs_tracker_result* result) {
    if (!t) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(t, [&]() -> int {
        visfs_flow* f = t->f;
        const int rc_args = check_call(t, left, right, stride, delta_guess, n_outliers, outlier_ids, result);
        if (rc_args != VISFS_BA_OK) return rc_args;
        const MemberPlan P = plan_member(t, delta_guess, n_outliers, outlier_ids);
        if (f->device) {                                               // a group of one through the tracker's own block
            const visfs_tracker_frame fr{ left, right, stride, delta_guess, n_outliers, outlier_ids };
            GroupCounts counts;
            CallFault fault;
            const int rc = run_call(&t, 1, &fr, &P, t->own.blk, f->dev, f->stream, &counts, &fault);
            if (rc != VISFS_BA_OK) { t->ids.clear(); return fail(t, rc, fault.why); }
            return commit_member(t, P, result);
        }
        const int rc_push = t->prm.clahe ? visfs_flow_push_frame_clahe(f, &t->prm.clahe_params, left, right, stride)
                                         : visfs_flow_push_frame(f, left, right, stride);
        if (rc_push != VISFS_BA_OK) return fail(t, rc_push, f->err);
        t->seen_frames = f->frames;
        if (!P.no_previous) {
            t->have_call = false;
            InHead ih{ n_outliers, 0 };
            std::memcpy(t->h_inblk.data(), &ih, sizeof(ih));
            if (n_outliers > 0) std::memcpy(t->h_inblk.data() + sizeof(InHead), outlier_ids, sizeof(uint64_t) * (size_t)n_outliers);
            host_pretreat(t);
            if (P.boot) {
                const int rc = host_bootstrap(t);
                if (rc != VISFS_BA_OK) return rc;
            }
            host_track_reduce(t, P.has_guess ? &P.g : nullptr);
            host_discs(t);
            const int rc = host_topup_stereo_finish(t, P.boot);
            if (rc != VISFS_BA_OK) return rc;
        }
        return commit_member(t, P, result);
    });
}

int visfs_tracker_download(const visfs_tracker* ct, int32_t* n_from, float* guess_xy, float* to_xy, uint8_t* lk_status, uint8_t* in_bounds,
                           int32_t* n_discs, visfs_corners_disc* discs, uint8_t* disc_drawn, int32_t* n_rows, uint8_t* stereo_status) {
    visfs_tracker* t = const_cast<visfs_tracker*>(ct);
    if (!t) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(t, [&]() -> int {
        if (!t->f) return fail(t, VISFS_BA_ERR_NOT_LOADED, "the flow object of this tracker is gone");
        if (!t->have_call) return fail(t, VISFS_BA_ERR_NOT_LOADED, "no call to report on");
        visfs_flow* f = t->f;
        const Bufs& B = t->B;
        Ctl c;
        if (f->device) {
            HIP_TRY(t, hipSetDevice(f->dev));
            HIP_TRY(t, hipMemcpyAsync(&c, B.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipStreamSynchronize(f->stream));
        } else {
            c = *B.ctl;
        }
        const size_t nf = (size_t)std::min(std::max(c.n_from, 0), t->S.M), nl = (size_t)std::min(std::max(c.n_list, 0), 2 * t->S.M),
                     nr = (size_t)std::min(std::max(c.lost ? 0 : c.n_rows, 0), t->S.M);
        if (n_from) *n_from = (int32_t)nf;
        if (n_discs) *n_discs = (int32_t)nl;
        if (n_rows) *n_rows = (int32_t)nr;
        const auto get = [&](void* dst, const void* src, size_t bytes) -> int {
            if (!dst || bytes == 0) return VISFS_BA_OK;
            if (!f->device) { std::memcpy(dst, src, bytes); return VISFS_BA_OK; }
            HIP_TRY(t, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, f->stream));
            return VISFS_BA_OK;
        };
        int rc = get(guess_xy, B.guess, 8 * nf);
        if (rc == VISFS_BA_OK) rc = get(to_xy, B.to, 8 * nf);
        if (rc == VISFS_BA_OK) rc = get(lk_status, B.lk_st, nf);
        if (rc == VISFS_BA_OK) rc = get(in_bounds, B.inb, nf);
        if (rc == VISFS_BA_OK) rc = get(discs, B.list, sizeof(visfs_corners_disc) * nl);
        if (rc == VISFS_BA_OK) rc = get(disc_drawn, B.drawn, nl);
        if (rc == VISFS_BA_OK) rc = get(stereo_status, B.row_st, nr);
        if (rc != VISFS_BA_OK) return rc;
        if (f->device) HIP_TRY(t, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_tracker_download_cull(const visfs_tracker* ct, int32_t* applied, int32_t* m, int32_t* n_hypotheses, int32_t* n_inliers, uint8_t* mask,
                                uint8_t* status, double* F, double* T1, double* T2, int32_t* winner_h, int32_t* winner_k) {
    visfs_tracker* t = const_cast<visfs_tracker*>(ct);
    if (!t) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(t, [&]() -> int {
        if (!t->f) return fail(t, VISFS_BA_ERR_NOT_LOADED, "the flow object of this tracker is gone");
        if (!t->have_call) return fail(t, VISFS_BA_ERR_NOT_LOADED, "no call to report on");
        if (applied) *applied = 0;
        if (m) *m = 0;
        if (n_hypotheses) *n_hypotheses = 0;
        if (n_inliers) *n_inliers = 0;
        if (winner_h) *winner_h = -1;
        if (winner_k) *winner_k = -1;
        for (int i = 0; i < 9; ++i) { if (F) F[i] = 0.0; if (T1) T1[i] = 0.0; if (T2) T2[i] = 0.0; }
        if (!t->cull_on) return (int)VISFS_BA_OK;
        visfs_flow* f = t->f;
        const fund::CullRec& C = t->B.cull;
        const size_t M = (size_t)t->S.M;
        Ctl c;
        fund::Header hd{};
        fund::Result res{};
        std::vector<uint8_t> h_mask(M), h_status(M);
        if (f->device) {
            HIP_TRY(t, hipSetDevice(f->dev));
            HIP_TRY(t, hipMemcpyAsync(&c, t->B.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(&hd, C.head, sizeof(hd), hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(&res, C.res, sizeof(res), hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(h_mask.data(), C.mask, M, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(h_status.data(), C.status, M, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipStreamSynchronize(f->stream));
        } else {
            c = *t->B.ctl; hd = *C.head; res = *C.res;
            std::memcpy(h_mask.data(), C.mask, M); std::memcpy(h_status.data(), C.status, M);
        }
        const size_t nf = (size_t)std::min(std::max(c.n_from, 0), t->S.M);
        const int32_t rows = std::min(std::max(c.cull_m, 0), t->S.M);
        if (m) *m = rows;
        if (status) std::memcpy(status, h_status.data(), nf);
        if (mask) std::memcpy(mask, h_mask.data(), nf);
        if (rows < fund::kMinRows) return (int)VISFS_BA_OK;            // not applied: the status passed through, the rest is zero
        if (applied) *applied = 1;
        if (n_hypotheses) *n_hypotheses = rows == fund::kMinRows ? 1 : t->cull.iterations;
        int32_t inl = 0;
        for (size_t i = 0; i < nf; ++i) inl += h_mask[i];
        if (n_inliers) *n_inliers = inl;
        if (winner_h) *winner_h = res.winner_h;
        if (winner_k) *winner_k = res.winner_k;
        if (F) for (int i = 0; i < 9; ++i) F[i] = res.F[i];
        if (T1) fund::hartley_matrix(hd.T1, T1);
        if (T2) fund::hartley_matrix(hd.T2, T2);
        return (int)VISFS_BA_OK;
    });
}

// ---------------------------------------------------------------- the pose guess (include/visfs_tracker_pnp.h)
int visfs_tracker_pnp_abi_version(void) { return VISFS_TRACKER_PNP_ABI_VERSION; }

int visfs_tracker_enable_pnp(visfs_tracker* t, const visfs_pnp_params* p) {
    if (!t) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(t, [&]() -> int {
        visfs_flow* f = t->f;
        if (!f) return fail(t, VISFS_BA_ERR_NOT_LOADED, "the flow object of this tracker is gone");
        if (t->group) return fail(t, VISFS_BA_ERR_BAD_ARGUMENT, "the tracker is in a group: set the pose guess first, then create the group");
        if (!p) { t->pnp_on = false; return (int)VISFS_BA_OK; }
        visfs_pnp_camera cam;
        cam.fx = (double)t->cam.fx; cam.fy = (double)t->cam.fy; cam.cx = (double)t->cam.cx; cam.cy = (double)t->cam.cy;
        for (int i = 0; i < 12; ++i) cam.Tir[i] = t->cam.Tir[i];
        const char* why = "";
        const int rc = pnp::check_params(*p, cam, &why);
        if (rc != VISFS_BA_OK) return fail(t, rc, why);
        const size_t M = (size_t)t->S.M, H = (size_t)p->iterations;
        t->pnp_matches.assign(M, 0); t->pnp_inliers.assign(M, 0); t->pnp_list.assign(M, 0);
        t->pnp_to_xyz.assign(3 * M, 0.0f); t->pnp_rows.assign(M, pnp::Row{});
        t->pnp_index.reserve(M);
        pnp_clear(t, 0);                                               // (the arrays of the result before have moved)
        if (!f->device) {
            if (!t->pnp_host) {
                const int rc_h = visfs_pnp_create_host(t->S.M, &t->pnp_host);
                if (rc_h != VISFS_BA_OK) return fail(t, rc_h, "the host solver of the pose guess could not be created");
            }
        } else {
            HIP_TRY(t, hipSetDevice(f->dev));
            HIP_TRY(t, hipStreamSynchronize(f->stream));                // nothing reads the blocks that go
            t->pnp_on = false;
            // the state of the two stages; then the output block again, with the pose guess's part behind what it holds today
            Carver c{ nullptr };
            const auto carve = [&](Carver& k, pnp::PnpRec& q, Bufs& b) {
                b.pnp_key = k.take<unsigned long long>(1); b.pnp_rows = k.take<pnp::Row>(M);
                q.models = k.take<double>(12 * H); q.pass_tq = k.take<double>(7 * pnp::kMaxRefine);
                q.samples = k.take<int32_t>(4 * H); q.vc = k.take<int32_t>(2 * H);
                q.pass_thr = k.take<float>(pnp::kMaxRefine); q.pass_cnt = k.take<int32_t>(pnp::kMaxRefine);
                q.pass_lists = k.take<int32_t>((size_t)pnp::kMaxRefine * M);
                return (k.off + 255) & ~size_t(255);
            };
            pnp::PnpRec q{};
            Bufs scratch{};
            const size_t state_bytes = carve(c, q, scratch);
            Out sized{};
            const size_t out_bytes = carve_out(nullptr, M, true, sized);
            DeviceBuf<char> d_pnp, d_out;
            PinnedBuf<char> p_out;
            std::string why;
            const int made = [&]() -> int {
                RC_TRY(d_pnp.alloc(&why, state_bytes));
                RC_TRY(d_out.alloc(&why, out_bytes));
                RC_TRY(p_out.alloc(&why, out_bytes));
                hipError_t e = hipMemsetAsync(d_pnp.get(), 0, state_bytes, f->stream);
                if (e == hipSuccess) e = hipMemsetAsync(d_out.get(), 0, out_bytes, f->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
                if (e != hipSuccess) { why = hipGetErrorString(e); return VISFS_BA_ERR_DEVICE; }
                return VISFS_BA_OK;
            }();
            if (made != VISFS_BA_OK) return fail(t, VISFS_BA_ERR_DEVICE, "the buffers of the pose guess: " + why);
            std::memset(p_out.get(), 0, out_bytes);
            t->own.d_pnp = std::move(d_pnp); t->own.d_out = std::move(d_out); t->own.p_out = std::move(p_out); t->out_bytes = out_bytes;
            Carver k{ t->own.d_pnp.get() };
            carve(k, q, t->B);
            carve_out(t->own.d_out.get(), M, true, t->B.o);
            carve_out(t->own.p_out.get(), M, true, t->R);
            q.m = &t->B.ctl->pnp_m; q.rows = t->B.pnp_rows; q.key = t->B.pnp_key;
            q.res = t->B.o.p_res; q.inliers = t->B.o.p_inl;
            q.K = pnp::Cam{ cam.fx, cam.fy, cam.cx, cam.cy };
            q.cap = t->S.M; q.skip = 0;
            t->pnp_rec = q;
            t->have_call = false;                                      // (the hooks' arrays of the call before are gone with the block)
        }
        t->pnp_prm = *p; t->pnp_cam = cam;
        t->pnp_shape = pnp::PnpShape{ p->iterations, p->min_inliers < 4 ? 4 : p->min_inliers, p->refine_iterations, p->reproj_error,
                                      p->refine_sigma, p->seed };
        t->pnp_on = true;
        return (int)VISFS_BA_OK;
    });
}

int visfs_tracker_pnp_last(const visfs_tracker* t, visfs_tracker_pnp_result* out) {
    if (!t || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!t->called) return VISFS_BA_ERR_NOT_LOADED;
    *out = t->pnp_res;
    return VISFS_BA_OK;
}

int visfs_tracker_download_pnp(const visfs_tracker* ct, int32_t* m, int32_t* n_hypotheses, int32_t* n_passes, int32_t* samples,
                               int32_t* valid, double* models, int32_t* counts, int32_t* winner, double* refit_tq, double* pass_tq,
                               float* pass_threshold, int32_t* pass_count, int32_t* pass_inliers) {
    visfs_tracker* t = const_cast<visfs_tracker*>(ct);
    if (!t) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(t, [&]() -> int {
        if (!t->f) return fail(t, VISFS_BA_ERR_NOT_LOADED, "the flow object of this tracker is gone");
        if (!t->have_call) return fail(t, VISFS_BA_ERR_NOT_LOADED, "no call to report on");
        if (m) *m = 0;
        if (n_hypotheses) *n_hypotheses = 0;
        if (n_passes) *n_passes = 0;
        if (winner) *winner = -1;
        if (refit_tq) for (int i = 0; i < 7; ++i) refit_tq[i] = 0.0;
        if (!t->pnp_on || !t->pnp_res.ran) return (int)VISFS_BA_OK;
        visfs_flow* f = t->f;
        if (!f->device) {
            int rc = visfs_pnp_last_sizes(t->pnp_host, m, n_hypotheses, n_passes);
            if (rc == VISFS_BA_OK)
                rc = visfs_pnp_download(t->pnp_host, samples, valid, models, counts, winner, refit_tq, pass_tq, pass_threshold, pass_count,
                                        pass_inliers);
            if (rc != VISFS_BA_OK) return fail(t, rc, visfs_pnp_last_error(t->pnp_host));
            return (int)VISFS_BA_OK;
        }
        const size_t H = (size_t)t->pnp_last_hyp, R = (size_t)t->pnp_last_passes, rows = (size_t)t->pnp_last_m, cap = (size_t)t->S.M;
        if (m) *m = t->pnp_last_m;
        if (n_hypotheses) *n_hypotheses = t->pnp_last_hyp;
        if (n_passes) *n_passes = t->pnp_last_passes;
        if (winner) *winner = t->pnp_model.winner;
        if (refit_tq) for (int i = 0; i < 7; ++i) refit_tq[i] = t->pnp_model.refit0[i];
        if (H == 0) return (int)VISFS_BA_OK;
        const pnp::PnpRec& q = t->pnp_rec;
        std::vector<int32_t> h_samples(4 * H), h_vc(2 * H), h_pcnt(pnp::kMaxRefine), h_plists(R * cap);
        std::vector<double> h_models(12 * H), h_ptq(7 * pnp::kMaxRefine);
        std::vector<float> h_pthr(pnp::kMaxRefine);
        HIP_TRY(t, hipSetDevice(f->dev));
        HIP_TRY(t, hipMemcpyAsync(h_samples.data(), q.samples, 16 * H, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(t, hipMemcpyAsync(h_vc.data(), q.vc, 8 * H, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(t, hipMemcpyAsync(h_models.data(), q.models, 96 * H, hipMemcpyDeviceToHost, f->stream));
        if (R > 0) {
            HIP_TRY(t, hipMemcpyAsync(h_ptq.data(), q.pass_tq, 56 * R, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(h_pthr.data(), q.pass_thr, 4 * R, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(h_pcnt.data(), q.pass_cnt, 4 * R, hipMemcpyDeviceToHost, f->stream));
            HIP_TRY(t, hipMemcpyAsync(h_plists.data(), q.pass_lists, 4 * R * cap, hipMemcpyDeviceToHost, f->stream));
        }
        HIP_TRY(t, hipStreamSynchronize(f->stream));
        for (size_t h = 0; h < H; ++h) {
            if (samples) for (int k = 0; k < 4; ++k) samples[4 * h + k] = h_samples[4 * h + k];
            if (valid) valid[h] = h_vc[2 * h];
            if (counts) counts[h] = h_vc[2 * h + 1];
            if (models) for (int k = 0; k < 12; ++k) models[12 * h + k] = h_models[12 * h + k];
        }
        for (size_t k = 0; k < R; ++k) {
            if (pass_tq) for (int i = 0; i < 7; ++i) pass_tq[7 * k + i] = h_ptq[7 * k + i];
            if (pass_threshold) pass_threshold[k] = h_pthr[k];
            if (pass_count) pass_count[k] = h_pcnt[k];
            const size_t cnt_k = (size_t)std::min(std::max(h_pcnt[k], 0), t->pnp_last_m);
            if (pass_inliers)
                for (size_t i = 0; i < rows; ++i) pass_inliers[k * rows + i] = i < cnt_k ? h_plists[k * cap + i] : -1;
        }
        return (int)VISFS_BA_OK;
    });
}

}  // extern "C"

// ====================================================================== tracker groups (include/visfs_tracker_group.h)
namespace {

thread_local std::string g_create_err;         // why the last visfs_tracker_group_create of this thread refused

int refuse(int rc, int member, const std::string& why) {
    g_create_err = member >= 0 ? "member " + std::to_string(member) + ": " + why : why;
    return rc;
}

int gfail(visfs_tracker_group* g, int rc, int member, const std::string& why) {
    g->err = member >= 0 ? "member " + std::to_string(member) + ": " + why : why;
    return rc;
}
bool same_flow_params(const visfs_flow_params& a, const visfs_flow_params& b) {
    return a.win_size == b.win_size && a.max_level == b.max_level && a.iterations == b.iterations && a.eps == b.eps &&
           a.flow_back == b.flow_back && a.min_eig_threshold == b.min_eig_threshold && a.back_gate_track == b.back_gate_track &&
           a.back_gate_stereo == b.back_gate_stereo && a.min_depth == b.min_depth && a.max_depth == b.max_depth;
}

bool same_tracker_params(const visfs_tracker_params& a, const visfs_tracker_params& b) {
    return a.max_features == b.max_features && a.quality_level == b.quality_level && a.min_distance == b.min_distance &&
           a.min_inliers == b.min_inliers && (a.clahe != 0) == (b.clahe != 0) && a.clahe_params.clip_limit == b.clahe_params.clip_limit &&
           a.clahe_params.tiles_x == b.clahe_params.tiles_x && a.clahe_params.tiles_y == b.clahe_params.tiles_y &&
           (a.cull != 0) == (b.cull != 0) && a.cull_params.pixel_error == b.cull_params.pixel_error &&
           a.cull_params.iterations == b.cull_params.iterations && a.cull_params.seed == b.cull_params.seed;
}

bool same_pnp(const visfs_tracker* a, const visfs_tracker* b) {
    if (a->pnp_on != b->pnp_on) return false;
    if (!a->pnp_on) return true;
    const visfs_pnp_params &p = a->pnp_prm, &q = b->pnp_prm;
    return p.min_inliers == q.min_inliers && p.iterations == q.iterations && p.reproj_error == q.reproj_error &&
           p.refine_iterations == q.refine_iterations && p.refine_sigma == q.refine_sigma && p.seed == q.seed;
}

}  // namespace

extern "C" {

int visfs_tracker_group_abi_version(void) { return VISFS_TRACKER_GROUP_ABI_VERSION; }

int visfs_tracker_group_create(int32_t n, visfs_tracker* const* members, visfs_tracker_group** out) {
    if (!out) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, -1, "out is NULL");
    *out = nullptr;
    try {
        if (n < 1 || n > VISFS_TRACKER_GROUP_MAX) return refuse(VISFS_BA_ERR_UNSUPPORTED, -1, "the number of members must lie in 1 .. 64");
        if (!members) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, -1, "members is NULL");
        for (int i = 0; i < n; ++i) {
            const visfs_tracker* t = members[i];
            if (!t) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "a NULL tracker");
            if (!t->f) return refuse(VISFS_BA_ERR_NOT_LOADED, i, "the flow object of this tracker is gone");
            if (t->group) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the tracker is in a group already");
            const visfs_flow *f = t->f, *f0 = members[0]->f;
            if (f->device != f0->device) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "device and host-twin trackers cannot share a group");
            if (f->device && f->ba != f0->ba) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the tracker belongs to another handle");
            for (int k = 0; k < i; ++k)
                if (members[k]->f == f) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the tracker shares its flow object with member " + std::to_string(k));
            if (f->w != f0->w || f->h != f0->h) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the image size differs from member 0's");
            if (!same_flow_params(f->prm, f0->prm)) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the flow parameters differ from member 0's");
            if (!same_tracker_params(t->prm, members[0]->prm)) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the tracker parameters differ from member 0's");
            if (!same_pnp(t, members[0])) return refuse(VISFS_BA_ERR_BAD_ARGUMENT, i, "the pose guess setting differs from member 0's");
        }
        visfs_tracker_group* g = new visfs_tracker_group();
        g->m.assign(members, members + n);
        visfs_flow* f0 = members[0]->f;
        g->device = f0->device;
        if (g->device) {
            g->dev = f0->dev; g->stream = f0->stream;
            int rc = VISFS_BA_OK;
            std::string why;
            const hipError_t e = hipSetDevice(g->dev);
            if (e != hipSuccess) why = hipGetErrorString(e);
            if (e != hipSuccess || g->blk.allocate(&why, (size_t)n) != VISFS_BA_OK) rc = gfail(g, VISFS_BA_ERR_DEVICE, -1, "the group's call block: " + why);
            for (int i = 0; i < n && rc == VISFS_BA_OK; ++i) {
                visfs_flow* f = members[i]->f;
                rc = group_corners_prepare(f);
                if (rc == VISFS_BA_OK && members[i]->prm.clahe) rc = group_clahe_prepare(f);
                if (rc != VISFS_BA_OK) gfail(g, rc, i, f->err);
            }
            if (rc != VISFS_BA_OK) {
                g_create_err = g->err;
                delete g;
                return rc;
            }
        }
        for (int i = 0; i < n; ++i) members[i]->group = g;
        g_create_err.clear();
        *out = g;
        return VISFS_BA_OK;
    } catch (...) {
        return refuse(VISFS_BA_ERR_DEVICE, -1, "out of host memory");
    }
}

void visfs_tracker_group_destroy(visfs_tracker_group* g) {
    if (!g) return;
    for (visfs_tracker* t : g->m)
        if (t) t->group = nullptr;
    delete g;
}

// g == NULL: why the last visfs_tracker_group_create of the calling thread refused
const char* visfs_tracker_group_last_error(const visfs_tracker_group* g) { return g ? g->err.c_str() : g_create_err.c_str(); }

int visfs_tracker_group_last_counts(const visfs_tracker_group* g, int32_t* kernel_launches, int32_t* copies_and_memsets,
                                    int32_t* synchronisations) {
    return g ? g->cnt.read(kernel_launches, copies_and_memsets, synchronisations) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

int visfs_tracker_group_process(visfs_tracker_group* g, const visfs_tracker_frame* frames, visfs_tracker_result* results) {
    if (!g) return VISFS_BA_ERR_BAD_ARGUMENT;
    try {
        g->cnt = GroupCounts{};
        if (!frames || !results) return gfail(g, VISFS_BA_ERR_BAD_ARGUMENT, -1, "a NULL argument");
        const int n = (int)g->m.size();
        // every check of every member before anything is pushed
        for (int i = 0; i < n; ++i) {
            visfs_tracker* t = g->m[i];
            if (!t) return gfail(g, VISFS_BA_ERR_NOT_LOADED, i, "the tracker has been destroyed");
            const visfs_tracker_frame& fr = frames[i];
            const int rc = check_call(t, fr.left, fr.right, fr.stride, fr.delta_guess, fr.n_outliers, fr.outlier_ids, &results[i]);
            if (rc != VISFS_BA_OK) return gfail(g, rc, i, t->err);
        }
        if (!g->device) {                      // the host twin: its members in sequence on one core
            for (int i = 0; i < n; ++i) {
                const visfs_tracker_frame& fr = frames[i];
                const int rc = visfs_tracker_process(g->m[i], fr.left, fr.right, fr.stride, fr.delta_guess, fr.n_outliers, fr.outlier_ids,
                                                     &results[i]);
                if (rc != VISFS_BA_OK) return gfail(g, rc, i, g->m[i]->err);
            }
            return VISFS_BA_OK;
        }
        std::vector<MemberPlan> plan((size_t)n);
        for (int i = 0; i < n; ++i) plan[(size_t)i] = plan_member(g->m[i], frames[i].delta_guess, frames[i].n_outliers, frames[i].outlier_ids);
        CallFault fault;
        const int rc = run_call(g->m.data(), n, frames, plan.data(), g->blk, g->dev, g->stream, &g->cnt, &fault);
        if (rc != VISFS_BA_OK) {
            for (visfs_tracker* t : g->m) t->ids.clear();
            return gfail(g, rc, fault.member, fault.why);
        }
        int rc_all = VISFS_BA_OK;
        for (int i = 0; i < n; ++i) {
            const int rc_i = commit_member(g->m[i], plan[(size_t)i], &results[i]);
            if (rc_i != VISFS_BA_OK && rc_all == VISFS_BA_OK) rc_all = gfail(g, rc_i, i, g->m[i]->err);
        }
        return rc_all;
    } catch (...) {
        return gfail(g, VISFS_BA_ERR_DEVICE, -1, "out of host memory");
    }
}

}  // extern "C"
