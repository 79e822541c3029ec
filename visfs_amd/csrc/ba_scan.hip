// Correlative scan matching on the laser sub-maps (include/visfs_scan_match.h).
//
// One call: the host forms the search (rotation table, weight table: every transcendental), uploads it with the points in one
// copy, and two launches on the sub-maps' stream follow, whatever S, L and n are:
//   k_scan_score  a workgroup owns scan k and a tile of <= 256 offsets; it stages the scan's cells chunk by chunk in LDS (the shared
//                 discretise function: no [S][n] array in global memory), every work item sums one candidate's int32 Q over its share
//                 of the chunk (neighbouring lanes take neighbouring xo: one point's loads of a wave fall into one or two lines of
//                 the grid), the shares are added through LDS (integers: no order), Q and the score are written, and the
//                 workgroup's best (score, index) goes into its slot;
//   k_scan_best   one workgroup reduces the slots under the same total order and writes the result record.
// The host twin (host sub-maps) runs the same functions of ba_scan.hpp sequentially.
#include "ba_scan.hpp"
#include "ba_host.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <string>

#pragma clang fp contract(off)

using namespace scan;
using namespace host;

namespace scan {

struct Slot { double score; int32_t index; int32_t pad; };
struct Record { double score; int32_t index; int32_t sum; };

struct ScoreArgs {
    const double* pts; const double* rot; const double* weight;
    GridView grid;
    double gx, gy, res, max_x, max_y;
    int32_t n, na, nl, Lw, Lsq;
    int32_t tc, slices, tiles;            // candidates of one tile, point slices (tc * slices <= kThreads), tiles per scan
    int32_t* sums; double* scores; Slot* slots;
};

// (score, index) of every work item reduced to the workgroup's best in item 0's entry; kThreads items, all of them call
__device__ inline void reduce_best(double* s_score, int32_t* s_index, int t) {
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h && better(s_score[t + h], s_index[t + h], s_score[t], s_index[t])) { s_score[t] = s_score[t + h]; s_index[t] = s_index[t + h]; }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_scan_score(ScoreArgs A) {
    __shared__ int2 s_cell[kChunk];
    __shared__ int32_t s_part[kThreads];
    __shared__ double s_score[kThreads];
    __shared__ int32_t s_index[kThreads];
    const int t = threadIdx.x;
    const int32_t k = blockIdx.y, tile = blockIdx.x;
    const int32_t c = t % A.tc, slice = t / A.tc;
    const int32_t cand = tile * A.tc + c;                                  // within the scan: yo-major, so that lanes run along xo
    const bool active = slice < A.slices && cand < A.Lsq;
    const int32_t yi = cand / A.Lw, xi = cand - yi * A.Lw;
    const int32_t xo = xi - A.nl, yo = yi - A.nl;
    const double cr = A.rot[2 * k], sr = A.rot[2 * k + 1];
    int32_t Q = 0;
    for (int32_t base = 0; base < A.n; base += kChunk) {
        const int32_t m = min(kChunk, A.n - base);
        for (int32_t i = t; i < m; i += kThreads) {
            int32_t ix, iy;
            discretise(cr, sr, A.pts[2 * (base + i)], A.pts[2 * (base + i) + 1], A.gx, A.gy, A.res, A.max_x, A.max_y, ix, iy);
            s_cell[i] = make_int2(ix, iy);
        }
        __syncthreads();
        if (active) {
#pragma unroll 4
            for (int32_t i = slice; i < m; i += A.slices) {
                const int2 p = s_cell[i];
                Q += cell_gain(A.grid, p.x + xo, p.y + yo);                // bounds-checked: the window may lie outside the grid
            }
        }
        __syncthreads();
    }
    s_part[t] = active ? Q : 0;
    __syncthreads();
    double score = -1.0;                                                   // below every candidate's (>= 0)
    int32_t index = INT_MAX;
    if (active && slice == 0) {
        int32_t q = 0;
        for (int32_t j = 0; j < A.slices; ++j) q += s_part[c + j * A.tc];
        index = (k * A.Lw + xi) * A.Lw + yi;                               // generation order: k, then xo, then yo
        score = candidate_score(q, A.n, A.weight[weight_index(A.na, A.nl, k, xo, yo)]);
        A.sums[index] = q;
        A.scores[index] = score;
    }
    s_score[t] = score; s_index[t] = index;
    reduce_best(s_score, s_index, t);
    if (t == 0) { Slot o; o.score = s_score[0]; o.index = s_index[0]; o.pad = 0; A.slots[k * A.tiles + tile] = o; }
}

__global__ __launch_bounds__(kThreads) void k_scan_best(const Slot* __restrict__ slots, int32_t nslots, const int32_t* __restrict__ sums,
                                                        Record* __restrict__ out) {
    __shared__ double s_score[kThreads];
    __shared__ int32_t s_index[kThreads];
    const int t = threadIdx.x;
    double score = -1.0;
    int32_t index = INT_MAX;
    for (int32_t i = t; i < nslots; i += kThreads) {
        const Slot s = slots[i];
        if (better(s.score, s.index, score, index)) { score = s.score; index = s.index; }
    }
    s_score[t] = score; s_index[t] = index;
    reduce_best(s_score, s_index, t);
    if (t == 0) { Record r; r.score = s_score[0]; r.index = s_index[0]; r.sum = s_index[0] == INT_MAX ? 0 : sums[s_index[0]]; *out = r; }
}

// the hook's cells [S][n][2] (not part of a match)
__global__ __launch_bounds__(kThreads) void k_scan_cells(const double* __restrict__ pts, const double* __restrict__ rot, int32_t n, int64_t total,
                                                         double gx, double gy, double res, double max_x, double max_y, int32_t* __restrict__ cells) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t k = (int32_t)(i / n), j = (int32_t)(i - (int64_t)k * n);
    int32_t ix, iy;
    discretise(rot[2 * k], rot[2 * k + 1], pts[2 * j], pts[2 * j + 1], gx, gy, res, max_x, max_y, ix, iy);
    cells[2 * i] = ix; cells[2 * i + 1] = iy;
}

}  // namespace scan

namespace {

// ---------------------------------------------------------------- the matcher's state on a sub-maps object
struct State {
    bool have = false;                        // the last successful call matched: `plan` and the candidates describe it
    bool device = false;
    Plan plan;
    // host twin
    std::vector<int32_t> sums;
    std::vector<double> scores;
    // device: one upload buffer (points, rotation table, weight table) with its pinned source, the candidates, the slots, the record
    Staged<char> up;
    DeviceBuf<int32_t> d_sums; DeviceBuf<double> d_scores;
    DeviceBuf<Slot> d_slots;
    DeviceBuf<Record> d_rec; PinnedBuf<Record> h_rec;
    DeviceBuf<int32_t> d_cells;
    const double* d_pts() const { return reinterpret_cast<const double*>(up.d.get()); }
    const double* d_rot() const { return d_pts() + 2 * (size_t)plan.n; }
};

void state_destroy(void* v) {
    delete static_cast<State*>(v);
}

State* state_of(visfs_submaps* s) {
    void** slot = visfs_internal_scan_slot(s, state_destroy);
    if (!*slot) *slot = new State();
    return static_cast<State*>(*slot);
}

// candidates of one tile and point slices of a workgroup: small windows share the workgroup's items among slices of the points
void tiling(int32_t Lsq, int32_t& tc, int32_t& slices, int32_t& tiles) {
    tc = std::min<int32_t>(Lsq, kThreads);
    slices = kThreads / tc;
    tiles = (Lsq + tc - 1) / tc;
}

int device_match(visfs_submaps* s, State* st, const submap::ScanAccess& acc, Plan& P, visfs_scan_match_result* out) {
    const size_t npts = 2 * (size_t)P.n, nrot = 2 * (size_t)P.S, nw = P.weight.size();
    const size_t bytes = (npts + nrot + nw) * sizeof(double);
    bool grew = false;
    const int made = st->up.reserve(s, bytes, bytes + bytes / 2, &grew);
    if (grew) st->have = false;                                            // what the last call left went with the old buffer
    if (made != VISFS_BA_OK) return made;
    if (!st->d_rec.get() || !st->h_rec.get()) {
        RC_TRY(st->d_rec.alloc(s, 1));
        RC_TRY(st->h_rec.alloc(s, 1));
    }
    int32_t tc, slices, tiles;
    tiling(P.Lw * P.Lw, tc, slices, tiles);
    const size_t ncand = (size_t)P.candidates(), nslots = (size_t)P.S * tiles;
    if (st->d_sums.cap() < ncand || st->d_scores.cap() < ncand) st->have = false;
    RC_TRY(st->d_sums.grow(s, ncand, ncand / 2));
    RC_TRY(st->d_scores.grow(s, ncand, ncand / 2));
    RC_TRY(st->d_slots.grow(s, nslots, nslots / 2));
    st->have = false;                                                      // the buffers are about to hold this call
    double* h = reinterpret_cast<double*>(st->up.h.get());
    std::memcpy(h, P.pts.data(), npts * sizeof(double));
    std::memcpy(h + npts, P.rot.data(), nrot * sizeof(double));
    std::memcpy(h + npts + nrot, P.weight.data(), nw * sizeof(double));
    HIP_TRY(s, hipMemcpyAsync(st->up.d.get(), st->up.h.get(), bytes, hipMemcpyHostToDevice, acc.stream));
    const double* d = reinterpret_cast<const double*>(st->up.d.get());
    ScoreArgs A{};
    A.pts = d; A.rot = d + npts; A.weight = d + npts + nrot;
    A.grid = acc.grid;
    A.gx = P.gx; A.gy = P.gy; A.res = P.L.res; A.max_x = P.L.max_x; A.max_y = P.L.max_y;
    A.n = P.n; A.na = P.na; A.nl = P.nl; A.Lw = P.Lw; A.Lsq = P.Lw * P.Lw;
    A.tc = tc; A.slices = slices; A.tiles = tiles;
    A.sums = st->d_sums.get(); A.scores = st->d_scores.get(); A.slots = st->d_slots.get();
    hipLaunchKernelGGL(k_scan_score, dim3(tiles, P.S), dim3(kThreads), 0, acc.stream, A);
    HIP_TRY(s, hipGetLastError());
    hipLaunchKernelGGL(k_scan_best, dim3(1), dim3(kThreads), 0, acc.stream, st->d_slots.get(), (int32_t)nslots, st->d_sums.get(), st->d_rec.get());
    HIP_TRY(s, hipGetLastError());
    HIP_TRY(s, hipMemcpyAsync(st->h_rec.get(), st->d_rec.get(), sizeof(Record), hipMemcpyDeviceToHost, acc.stream));
    HIP_TRY(s, hipStreamSynchronize(acc.stream));
    const Record r = *st->h_rec.get();
    if (r.index < 0 || (int64_t)r.index >= P.candidates()) return visfs_internal_scan_fail(s, VISFS_BA_ERR_DEVICE, "the reduction returned no candidate");
    fill_result(P, r.index, r.score, r.sum, *out);
    st->plan = std::move(P);
    st->have = true;
    return VISFS_BA_OK;
}

// the scan's cells of rotation k, in point order
void host_cells(const Plan& P, int32_t k, int32_t* cells_xy) {
    for (int32_t i = 0; i < P.n; ++i)
        discretise(P.rot[2 * k], P.rot[2 * k + 1], P.pts[2 * i], P.pts[2 * i + 1], P.gx, P.gy, P.L.res, P.L.max_x, P.L.max_y, cells_xy[2 * i], cells_xy[2 * i + 1]);
}

int host_match(State* st, const submap::ScanAccess& acc, Plan& P, visfs_scan_match_result* out) {
    std::vector<int32_t> sums((size_t)P.candidates());
    std::vector<double> scores((size_t)P.candidates());
    std::vector<int32_t> cells(2 * (size_t)P.n);
    double best = -1.0;
    int32_t best_i = INT_MAX;
    int32_t idx = 0;
    for (int32_t k = 0; k < P.S; ++k) {
        host_cells(P, k, cells.data());
        for (int32_t xo = -P.nl; xo <= P.nl; ++xo)
            for (int32_t yo = -P.nl; yo <= P.nl; ++yo, ++idx) {
                int32_t Q = 0;
                for (int32_t i = 0; i < P.n; ++i) Q += cell_gain(acc.grid, cells[2 * i] + xo, cells[2 * i + 1] + yo);
                const double sc = candidate_score(Q, P.n, P.weight[weight_index(P.na, P.nl, k, xo, yo)]);
                sums[idx] = Q; scores[idx] = sc;
                if (better(sc, idx, best, best_i)) { best = sc; best_i = idx; }
            }
    }
    fill_result(P, best_i, best, sums[best_i], *out);
    st->sums.swap(sums); st->scores.swap(scores);
    st->plan = std::move(P);
    st->have = true;
    return VISFS_BA_OK;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_scan_match_abi_version(void) { return VISFS_SCAN_MATCH_ABI_VERSION; }

void visfs_scan_match_default_params(visfs_scan_match_params* p) {
    if (!p) return;
    p->linear_search_window = 0.1;
    p->angular_search_window = 20.0 * 3.14159265358979323846 / 180.0;
    p->translation_delta_cost_weight = 0.1;
    p->rotation_delta_cost_weight = 0.1;
}

int visfs_scan_match(visfs_submaps* s, int32_t index, const visfs_scan_match_params* p, const double g[3], int32_t n, const double* xyz,
                     visfs_scan_match_result* out) {
    if (!s || !p || !g || !out || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        if (index < 0) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        if (n > VISFS_SCAN_MATCH_MAX_POINTS) return visfs_internal_scan_fail(s, VISFS_BA_ERR_UNSUPPORTED, "more than 16384 points");
        for (int i = 0; i < 3; ++i) if (!std::isfinite(g[i])) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "the guess is not finite");
        for (int64_t i = 0; i < 3 * (int64_t)n; ++i) if (!std::isfinite(xyz[i])) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "a point is not finite");
        if (!std::isfinite(p->linear_search_window) || !std::isfinite(p->angular_search_window) || p->linear_search_window < 0.0 || p->angular_search_window < 0.0)
            return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "the search windows must be finite and not negative");
        if (!std::isfinite(p->translation_delta_cost_weight) || !std::isfinite(p->rotation_delta_cost_weight))
            return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "the cost weights must be finite");
        submap::ScanAccess acc;
        int rc = visfs_internal_scan_access(s, index, &acc);
        if (rc != VISFS_BA_OK) return rc;
        if (acc.count > 0 && index >= acc.count) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        Plan P;
        if (acc.count > 0 && n > 0) {
            const char* why = "";
            if ((rc = make_plan(acc.L, *p, g, n, xyz, P, &why)) != VISFS_BA_OK) return visfs_internal_scan_fail(s, rc, why);
        }
        State* st = state_of(s);
        st->device = acc.device;
        if (acc.count == 0 || n == 0) {                                    // no sub-map yet, or nothing to match: the guess back
            std::memset(out, 0, sizeof *out);
            out->x = g[0]; out->y = g[1]; out->yaw = g[2];
            st->have = false;
            return (int)VISFS_BA_OK;
        }
        return acc.device ? device_match(s, st, acc, P, out) : host_match(st, acc, P, out);
    });
}

int visfs_scan_match_download(visfs_submaps* s, int64_t cap, int32_t* sums, double* scores, int32_t* cells_xy) {
    if (!s || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        State* st = state_of(s);
        if (!st->have) return (int)VISFS_BA_OK;
        const Plan& P = st->plan;
        const int64_t nc = P.candidates(), ncell = (int64_t)P.S * P.n;
        if (((sums || scores) && cap < nc) || (cells_xy && cap < ncell)) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "the hook's arrays are too small");
        if (!st->device) {
            if (sums) std::memcpy(sums, st->sums.data(), (size_t)nc * sizeof(int32_t));
            if (scores) std::memcpy(scores, st->scores.data(), (size_t)nc * sizeof(double));
            if (cells_xy) for (int32_t k = 0; k < P.S; ++k) host_cells(P, k, cells_xy + 2 * (size_t)k * P.n);
            return (int)VISFS_BA_OK;
        }
        submap::ScanAccess acc;
        int rc = visfs_internal_scan_access(s, -1, &acc);                  // the device and the stream
        if (rc != VISFS_BA_OK) return rc;
        if (sums) HIP_TRY(s, hipMemcpyAsync(sums, st->d_sums.get(), (size_t)nc * sizeof(int32_t), hipMemcpyDeviceToHost, acc.stream));
        if (scores) HIP_TRY(s, hipMemcpyAsync(scores, st->d_scores.get(), (size_t)nc * sizeof(double), hipMemcpyDeviceToHost, acc.stream));
        if (cells_xy) {
            RC_TRY(st->d_cells.grow(s, 2 * (size_t)ncell, (size_t)ncell));
            hipLaunchKernelGGL(k_scan_cells, dim3((unsigned)((ncell + kThreads - 1) / kThreads)), dim3(kThreads), 0, acc.stream, st->d_pts(), st->d_rot(),
                               P.n, ncell, P.gx, P.gy, P.L.res, P.L.max_x, P.L.max_y, st->d_cells.get());
            HIP_TRY(s, hipGetLastError());
            HIP_TRY(s, hipMemcpyAsync(cells_xy, st->d_cells.get(), 2 * (size_t)ncell * sizeof(int32_t), hipMemcpyDeviceToHost, acc.stream));
        }
        HIP_TRY(s, hipStreamSynchronize(acc.stream));
        return (int)VISFS_BA_OK;
    });
}

void visfs_scan_pretreat_default_params(visfs_scan_pretreat_params* p) {
    if (!p) return;
    p->num_subdivisions = 1; p->min_range = 0.1; p->max_range = 30.0; p->missing_ray_length = 5.0;
}

int visfs_scan_pretreat(const visfs_scan_pretreat_params* p, const double T[12], const double origin[3], int32_t n, const double* xyz,
                        double* returns_out, double* misses_out, visfs_range_data* rd_out, int32_t* n_out) {
    if (!p || !T || !origin || !n_out || n < 0 || p->num_subdivisions < 1) return VISFS_BA_ERR_BAD_ARGUMENT;
    *n_out = 0;
    if (n == 0) return VISFS_BA_OK;                                        // an empty cloud: nothing (Estimator.cpp:117-119)
    if (!xyz || !returns_out || !misses_out || !rd_out) return VISFS_BA_ERR_BAD_ARGUMENT;
    pretreat(*p, T, origin, n, xyz, returns_out, misses_out, rd_out, n_out);
    return VISFS_BA_OK;
}

}  // extern "C"
