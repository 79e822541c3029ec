// Monte-Carlo localisation on the likelihood field of a global map (include/visfs_mcl.h).
//
// The field, two launches:
//   k_mcl_rows      one work item per cell: the distance along the row to its nearest obstacle, clamped to R + 1 (ba_mcl.hpp: row_dist);
//   k_mcl_cols      one work item per cell: min over |dy| <= R of dy^2 + g^2, left once dy^2 reaches the best so far (col_min).
// An update, four launches whatever N and n are:
//   k_mcl_weight    `lanes` work items per particle (1 .. 64, a power of two, so a particle never straddles a wavefront): each moves
//                   the particle (the same bits in every lane), gathers its share of the beams from the field and the lanes' integer
//                   sums meet by xor shuffles; lane 0 stores the pose, its cos and sin, Q and the raw weight;
//   k_mcl_sums      a workgroup per 256 particles: the nine sums' adjacent-pair tree over its particles in LDS, and its largest weight;
//   k_mcl_finish    every workgroup finishes the tree over the at most 256 partial sums (the same bits in each), decides the
//                   resampling flag, normalises its 256 weights, forms their counts k and the exclusive scan of them within the
//                   workgroup; workgroup 0 writes the record;
//   k_mcl_resample  returns at once when the flag is clear; else every workgroup scans the at most 256 workgroup totals, and one work
//                   item per new particle finds its ancestor by two binary searches and copies it into the other buffer.
// No floating atomics, no workgroup waits for another: the kernels' order on the stream is the only dependence.  The one-core
// twin calls the same functions of ba_mcl.hpp in plain loops.
// A filter has an active count n, which is also the stride of its particle arrays; it is N unless the filter was made a KLD filter
// (include/visfs_mcl_kld.h), whose fourth launch is k_mcl_kld_resample of ba_mcl_kld.hip.  ba_mcl_state.hpp holds the objects.
#include "ba_mcl_state.hpp"
#include "ba_map_access.hpp"
#include "ba_host.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#pragma clang fp contract(off)

using namespace mcl;
using namespace host;
using submap::Limits;

namespace mcl {

__global__ __launch_bounds__(kThreads) void k_mcl_rows(const uint16_t* __restrict__ cells, int32_t nx, int64_t total, int32_t v_occ, int32_t R,
                                                       uint16_t* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t y = (int32_t)(i / nx), x = (int32_t)(i - (int64_t)y * nx);
    g[i] = row_dist(cells, nx, x, y, v_occ, R);
}

__global__ __launch_bounds__(kThreads) void k_mcl_cols(const uint16_t* __restrict__ g, int32_t nx, int32_t ny, int64_t total, int32_t R, int32_t T,
                                                       uint16_t* __restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t y = (int32_t)(i / nx), x = (int32_t)(i - (int64_t)y * nx);
    t[i] = col_min(g, nx, ny, x, y, R, T);
}

// st: x, y, yaw, w, each [N]
__global__ __launch_bounds__(kThreads) void k_mcl_init(const InitHdr* __restrict__ up, double* __restrict__ st, int64_t* __restrict__ Q,
                                                       int32_t* __restrict__ anc) {
    const InitHdr& I = *up;
    const int32_t j = (int32_t)(blockIdx.x * kThreads + threadIdx.x), N = I.N;
    if (j >= N) return;
    double x, y, yaw;
    init_particle(I, j, x, y, yaw);
    st[j] = x; st[(size_t)N + j] = y; st[2 * (size_t)N + j] = yaw; st[3 * (size_t)N + j] = I.inv_n;
    Q[j] = 0; anc[j] = j;
}

__device__ inline int64_t shfl_xor64(int64_t v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)((uint64_t)v & 0xFFFFFFFFull), m), hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), m);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

__global__ __launch_bounds__(kThreads) void k_mcl_weight(const Hdr* __restrict__ up, FieldView F, double* __restrict__ st, double* __restrict__ cs,
                                                         int64_t* __restrict__ Q) {
    const Hdr& H = *up;
    const double* __restrict__ beams = reinterpret_cast<const double*>(up + 1);
    const int32_t N = H.N, G = H.lanes;
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t jj = gid / G;
    if (jj >= N) return;                                                   // the whole group of lanes leaves together
    const int32_t j = (int32_t)jj, lane = (int32_t)(gid - jj * G);
    double x = st[j], y = st[(size_t)N + j], yaw = st[2 * (size_t)N + j];
    move_particle(H, j, x, y, yaw);
    double s, c;
    sincos_any(yaw, s, c);
    int64_t q = 0;
    for (int32_t b = lane; b < H.n; b += G) q += beam_q(F, x, y, c, s, beams[2 * b], beams[2 * b + 1]);
    for (int m = 1; m < G; m <<= 1) q += shfl_xor64(q, m);
    if (lane == 0) {
        st[j] = x; st[(size_t)N + j] = y; st[2 * (size_t)N + j] = yaw;
        st[3 * (size_t)N + j] = st[3 * (size_t)N + j] * weight_factor(q);
        cs[j] = c; cs[(size_t)N + j] = s;
        Q[j] = q;
    }
}

// The tree over sh[k][0 .. limit) for every k (limit a power of two, at most 256) and the largest weight of bw/bi over all 256.
__device__ inline void block_reduce(double (*sh)[kThreads], double* bw, int32_t* bi, int32_t limit) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
    for (int s = 1; s < kThreads; s <<= 1) {
        if ((tid & (2 * s - 1)) == 0) {
            if (s < limit)
                for (int k = 0; k < kSums; ++k) sh[k][tid] = sh[k][tid] + sh[k][tid + s];
            const double w2 = bw[tid + s];
            const int32_t i2 = bi[tid + s];
            if (w2 > bw[tid] || (w2 == bw[tid] && i2 < bi[tid])) { bw[tid] = w2; bi[tid] = i2; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void k_mcl_sums(const Hdr* __restrict__ up, const double* __restrict__ st, const double* __restrict__ cs,
                                                       double* __restrict__ part, double* __restrict__ pbw, int32_t* __restrict__ pbi) {
    __shared__ double sh[kSums][kThreads];
    __shared__ double bw[kThreads];
    __shared__ int32_t bi[kThreads];
    const Hdr& H = *up;
    const int32_t N = H.N, tid = (int32_t)threadIdx.x, j = (int32_t)(blockIdx.x * kThreads) + tid;
    double t[kSums];
    for (int k = 0; k < kSums; ++k) t[k] = 0.0;
    bw[tid] = -1.0; bi[tid] = 0x7FFFFFFF;
    if (j < N) {
        const double w = st[3 * (size_t)N + j];
        sum_terms(w, st[j], st[(size_t)N + j], cs[j], cs[(size_t)N + j], t);
        bw[tid] = w; bi[tid] = j;
    }
    for (int k = 0; k < kSums; ++k) sh[k][tid] = t[k];
    block_reduce(sh, bw, bi, H.P < kThreads ? H.P : kThreads);
    if (tid < kSums) part[(size_t)blockIdx.x * kSums + tid] = sh[tid][0];
    if (tid == 0) { pbw[blockIdx.x] = bw[0]; pbi[blockIdx.x] = bi[0]; }
}

// The inclusive scan of v over the workgroup.
__device__ inline uint64_t block_scan(uint64_t* sc, uint64_t v) {
    const int tid = (int)threadIdx.x;
    sc[tid] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const uint64_t a = tid >= off ? sc[tid - off] : 0;
        __syncthreads();
        sc[tid] += a;
        __syncthreads();
    }
    return sc[tid];
}

__global__ __launch_bounds__(kThreads) void k_mcl_finish(const Hdr* __restrict__ up, double* __restrict__ st, const double* __restrict__ part,
                                                         const double* __restrict__ pbw, const int32_t* __restrict__ pbi, int32_t blocks,
                                                         Rec* __restrict__ rec, uint64_t* __restrict__ C, uint64_t* __restrict__ bsum,
                                                         int32_t* __restrict__ anc) {
    __shared__ double sh[kSums][kThreads];
    __shared__ double bw[kThreads];
    __shared__ int32_t bi[kThreads];
    __shared__ uint64_t sc[kThreads];
    const Hdr& H = *up;
    const int32_t N = H.N, tid = (int32_t)threadIdx.x, j = (int32_t)(blockIdx.x * kThreads) + tid;
    for (int k = 0; k < kSums; ++k) sh[k][tid] = tid < blocks ? part[(size_t)tid * kSums + k] : 0.0;
    bw[tid] = tid < blocks ? pbw[tid] : -1.0;
    bi[tid] = tid < blocks ? pbi[tid] : 0x7FFFFFFF;
    block_reduce(sh, bw, bi, H.P > kThreads ? H.P / kThreads : 1);
    const double W = sh[0][0];
    const int32_t flag = gate_open(H.gate, W, sh[1][0], H.ratio_n) ? 1 : 0;
    if (blockIdx.x == 0 && tid == 0) {
        for (int k = 0; k < kSums; ++k) rec->sums[k] = sh[k][0];
        const int32_t b = bi[0];
        rec->best_w = bw[0]; rec->best = b;
        rec->best_pose[0] = st[b]; rec->best_pose[1] = st[(size_t)N + b]; rec->best_pose[2] = st[2 * (size_t)N + b];
        rec->K = 0; rec->r0 = 0; rec->resampled = flag;
    }
    uint64_t k = 0;
    if (j < N) {
        const double w = st[3 * (size_t)N + j] / W;
        st[3 * (size_t)N + j] = w;
        k = count_of(w);
        anc[j] = j;
    }
    const uint64_t inc = block_scan(sc, k);
    if (j < N) C[j] = inc - k;
    if (tid == kThreads - 1) bsum[blockIdx.x] = inc;
}

__global__ __launch_bounds__(kThreads) void k_mcl_resample(const Hdr* __restrict__ up, Rec* __restrict__ rec, const double* __restrict__ st,
                                                           double* __restrict__ out, const uint64_t* __restrict__ C,
                                                           const uint64_t* __restrict__ bsum, int32_t blocks, int32_t* __restrict__ anc) {
    __shared__ uint64_t sc[kThreads];
    if (rec->resampled == 0) return;                                       // the same in every work item of the launch
    const Hdr& H = *up;
    const int32_t N = H.N, tid = (int32_t)threadIdx.x, i = (int32_t)(blockIdx.x * kThreads) + tid;
    const uint64_t v = tid < blocks ? bsum[tid] : 0;
    const uint64_t inc = block_scan(sc, v);
    const uint64_t K = sc[kThreads - 1];
    __syncthreads();
    sc[tid] = inc - v;                                                     // the exclusive offsets of the workgroups
    __syncthreads();
    if (K == 0) return;                                                    // cannot happen with normalised weights; never divide by it
    const uint64_t r0 = key(H.seed, H.update, (uint64_t)N, 0) % K;
    if (blockIdx.x == 0 && tid == 0) { rec->K = K; rec->r0 = r0; }
    if (i >= N) return;
    const uint64_t u = ((uint64_t)i * K + r0) / (uint64_t)N;
    int32_t lo = 0, hi = blocks - 1;                                       // the last workgroup whose offset is at most u
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (sc[mid] <= u) lo = mid; else hi = mid - 1;
    }
    const uint64_t base = sc[lo];
    int32_t l = lo * kThreads, h = l + kThreads - 1;
    if (h > N - 1) h = N - 1;
    while (l < h) {                                                        // ... and its last particle whose prefix is at most u
        const int32_t mid = (l + h + 1) >> 1;
        if (base + C[mid] <= u) l = mid; else h = mid - 1;
    }
    out[i] = st[l]; out[(size_t)N + i] = st[(size_t)N + l]; out[2 * (size_t)N + i] = st[2 * (size_t)N + l];
    out[3 * (size_t)N + i] = H.inv_n;
    anc[i] = l;
}

}  // namespace mcl

namespace {

constexpr size_t kUpBytes = sizeof(Hdr) + (size_t)VISFS_MCL_MAX_BEAMS * 2 * sizeof(double);
static_assert(sizeof(Hdr) % 8 == 0 && sizeof(InitHdr) <= sizeof(Hdr), "the beams follow the header as doubles");

// The field of `cells` (memory of the given flavour, dense [ny][nx]); the parameters are already planned into f.
int field_build(visfs_mcl_field* f, const uint16_t* cells) {
    const int32_t nx = f->L.nx, ny = f->L.ny;
    const int64_t total = (int64_t)nx * ny;
    if (!f->device) {
        std::vector<uint16_t> g((size_t)total);
        f->h_t.resize((size_t)total);
        for (int32_t y = 0; y < ny; ++y)
            for (int32_t x = 0; x < nx; ++x) g[(size_t)y * nx + x] = row_dist(cells, nx, x, y, f->v_occ, f->R);
        for (int32_t y = 0; y < ny; ++y)
            for (int32_t x = 0; x < nx; ++x) f->h_t[(size_t)y * nx + x] = col_min(g.data(), nx, ny, x, y, f->R, f->T);
        return VISFS_BA_OK;
    }
    DeviceBuf<uint16_t> g;
    HIP_TRY(nullptr, hipSetDevice(f->dev));
    RC_TRY(f->d_t.alloc(nullptr, (size_t)total));
    RC_TRY(f->d_q.alloc(nullptr, f->h_q.size()));
    RC_TRY(g.alloc(nullptr, (size_t)total));
    f->counts = { VISFS_MCL_FIELD_LAUNCHES, 1, 1 };
    HIP_TRY(nullptr, hipMemcpyAsync(f->d_q.get(), f->h_q.data(), f->h_q.size() * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(k_mcl_rows, dim3(blocks_for(total, kThreads)), dim3(kThreads), 0, f->stream, cells, nx, total, f->v_occ, f->R, g.get());
    HIP_TRY(nullptr, hipGetLastError());
    hipLaunchKernelGGL(k_mcl_cols, dim3(blocks_for(total, kThreads)), dim3(kThreads), 0, f->stream, g.get(), nx, ny, total, f->R, f->T, f->d_t.get());
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipStreamSynchronize(f->stream));
    return VISFS_BA_OK;
}

// The field of host `cells` on the device: their copy lives until field_build has waited for the stream.
int field_build_uploaded(visfs_mcl_field* f, const uint16_t* cells) {
    const size_t total = (size_t)f->L.nx * f->L.ny;
    DeviceBuf<uint16_t> d_cells;
    HIP_TRY(nullptr, hipSetDevice(f->dev));
    RC_TRY(d_cells.alloc(nullptr, total));
    HIP_TRY(nullptr, hipMemcpyAsync(d_cells.get(), cells, total * 2, hipMemcpyHostToDevice, f->stream));
    return field_build(f, d_cells.get());
}

// Plans the parameters on limits L into a new field object; *out stays null on a refusal.
int field_new(const Limits& L, const visfs_mcl_field_params& p, visfs_mcl_field** out, const char** why) {
    std::vector<double> cost(32768);
    if (visfs_submap_hook_value_tables(cost.data(), nullptr) != VISFS_BA_OK) throw std::bad_alloc();
    visfs_mcl_field* f = new visfs_mcl_field();
    f->L = L;
    const int rc = field_plan(p, L.res, cost, f->v_occ, f->R, f->T, f->h_q, why);
    if (rc != VISFS_BA_OK) { delete f; return rc; }
    *out = f;
    return VISFS_BA_OK;
}

FieldView view_of(const visfs_mcl_field* f) {
    FieldView F;
    F.t = f->device ? f->d_t.get() : f->h_t.data();
    F.q = f->device ? f->d_q.get() : f->h_q.data();
    F.res = f->L.res; F.max_x = f->L.max_x; F.max_y = f->L.max_y; F.nx = f->L.nx; F.ny = f->L.ny; F.T = f->T;
    return F;
}

int mcl_alloc(visfs_mcl* f) {
    const size_t N = (size_t)f->N;
    HIP_TRY(f, hipSetDevice(f->dev));
    for (int b = 0; b < 2; ++b) RC_TRY(f->d_st[b].alloc(f, 4 * N));
    RC_TRY(f->d_cs.alloc(f, 2 * N));
    RC_TRY(f->d_Q.alloc(f, N));
    RC_TRY(f->d_anc.alloc(f, N));
    RC_TRY(f->d_C.alloc(f, N));
    RC_TRY(f->d_bsum.alloc(f, kMaxBlocks));
    RC_TRY(f->d_part.alloc(f, (size_t)kMaxBlocks * kSums));
    RC_TRY(f->d_pbw.alloc(f, kMaxBlocks));
    RC_TRY(f->d_pbi.alloc(f, kMaxBlocks));
    RC_TRY(f->d_up.alloc(f, kUpBytes));
    RC_TRY(f->d_rec.alloc(f, 1));
    RC_TRY(f->h_up.alloc(f, kUpBytes));
    RC_TRY(f->h_rec.alloc(f, 1));
    return VISFS_BA_OK;
}

int32_t lanes_for(const visfs_mcl* f, int32_t n) {
    if (f->lanes > 0) return f->lanes;
    int32_t G = 1;
    while (G < 64 && (int64_t)f->n * G < 32768 && G < n) G *= 2;
    return G;
}

int device_update(visfs_mcl* f, const Hdr& H, const std::vector<double>& beams, Rec& rec) {
    const int32_t N = H.N, blocks = (int32_t)blocks_for(N, kThreads);                 // the active count
    HIP_TRY(f, hipSetDevice(f->dev));
    std::memcpy(f->h_up.get(), &H, sizeof H);
    if (!beams.empty()) std::memcpy(f->h_up.get() + sizeof H, beams.data(), beams.size() * sizeof(double));
    HIP_TRY(f, hipMemcpyAsync(f->d_up.get(), f->h_up.get(), sizeof H + beams.size() * sizeof(double), hipMemcpyHostToDevice, f->stream));
    const Hdr* up = reinterpret_cast<const Hdr*>(f->d_up.get());
    double* st = f->d_st[f->cur].get();
    hipLaunchKernelGGL(k_mcl_weight, dim3(blocks_for((int64_t)N * H.lanes, kThreads)), dim3(kThreads), 0, f->stream, up, view_of(f->field), st, f->d_cs.get(), f->d_Q.get());
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_mcl_sums, dim3((unsigned)blocks), dim3(kThreads), 0, f->stream, up, st, f->d_cs.get(), f->d_part.get(), f->d_pbw.get(), f->d_pbi.get());
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_mcl_finish, dim3((unsigned)blocks), dim3(kThreads), 0, f->stream, up, st, f->d_part.get(), f->d_pbw.get(), f->d_pbi.get(), blocks,
                       f->kld ? kld_device_rec(f) : f->d_rec.get(), f->d_C.get(), f->d_bsum.get(), f->d_anc.get());
    HIP_TRY(f, hipGetLastError());
    if (f->kld) {                                                          // k_mcl_kld_resample takes the fourth launch's place
        const int rc = kld_device_resample(f, up, st, f->d_st[f->cur ^ 1].get(), blocks, rec);
        if (rc != VISFS_BA_OK) return rc;
        f->counts = { VISFS_MCL_UPDATE_LAUNCHES, 2, 1 };
        return VISFS_BA_OK;
    }
    hipLaunchKernelGGL(k_mcl_resample, dim3((unsigned)blocks), dim3(kThreads), 0, f->stream, up, f->d_rec.get(), st, f->d_st[f->cur ^ 1].get(), f->d_C.get(),
                       f->d_bsum.get(), blocks, f->d_anc.get());
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipMemcpyAsync(f->h_rec.get(), f->d_rec.get(), sizeof(Rec), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    rec = *f->h_rec.get();
    f->counts = { VISFS_MCL_UPDATE_LAUNCHES, 2, 1 };
    return VISFS_BA_OK;
}

void host_update(visfs_mcl* f, const Hdr& H, const std::vector<double>& beams, Rec& rec) {
    const size_t N = (size_t)H.N;                                          // the active count
    const FieldView F = view_of(f->field);
    std::vector<double>& st = f->h_st[f->cur];
    double *X = st.data(), *Y = X + N, *A = Y + N, *Wt = A + N;
    std::vector<double> sums[kSums];
    for (auto& v : sums) v.assign((size_t)H.P, 0.0);
    int32_t best = 0;
    for (size_t j = 0; j < N; ++j) {
        move_particle(H, (int32_t)j, X[j], Y[j], A[j]);
        double s, c;
        sincos_any(A[j], s, c);
        int64_t q = 0;
        for (int32_t b = 0; b < H.n; ++b) q += beam_q(F, X[j], Y[j], c, s, beams[2 * (size_t)b], beams[2 * (size_t)b + 1]);
        f->h_Q[j] = q;
        Wt[j] = Wt[j] * weight_factor(q);
        double t[kSums];
        sum_terms(Wt[j], X[j], Y[j], c, s, t);
        for (int k = 0; k < kSums; ++k) sums[k][j] = t[k];
        if (Wt[j] > Wt[(size_t)best]) best = (int32_t)j;
    }
    for (int k = 0; k < kSums; ++k) rec.sums[k] = tree_sum(sums[k]);
    rec.best = best; rec.best_w = Wt[(size_t)best];
    rec.best_pose[0] = X[(size_t)best]; rec.best_pose[1] = Y[(size_t)best]; rec.best_pose[2] = A[(size_t)best];
    rec.K = rec.r0 = 0;
    const double W = rec.sums[0];
    rec.resampled = gate_open(H.gate, W, rec.sums[1], H.ratio_n) ? 1 : 0;
    std::vector<uint64_t> C(N + 1, 0);
    for (size_t j = 0; j < N; ++j) {
        Wt[j] = Wt[j] / W;
        C[j + 1] = C[j] + count_of(Wt[j]);
        f->h_anc[j] = (int32_t)j;
    }
    const uint64_t K = C[N];
    if (!rec.resampled || K == 0) { rec.resampled = 0; return; }
    if (f->kld) { kld_host_resample(f, H, C, rec); return; }
    const uint64_t r0 = key(H.seed, H.update, (uint64_t)N, 0) % K;
    rec.K = K; rec.r0 = r0;
    std::vector<double>& out = f->h_st[f->cur ^ 1];
    for (size_t i = 0; i < N; ++i) {
        const uint64_t u = ((uint64_t)i * K + r0) / (uint64_t)N;
        const size_t a = (size_t)(std::upper_bound(C.begin(), C.begin() + (ptrdiff_t)N, u) - C.begin()) - 1;   // the last a with C_a <= u
        out[i] = X[a]; out[N + i] = Y[a]; out[2 * N + i] = A[a]; out[3 * N + i] = H.inv_n;
        f->h_anc[i] = (int32_t)a;
    }
}

bool limits_ok(const Limits& L) {
    return std::isfinite(L.res) && L.res > 0.0 && std::isfinite(L.max_x) && std::isfinite(L.max_y) && L.nx >= 1 && L.ny >= 1 &&
           (int64_t)L.nx * L.ny <= (int64_t)VISFS_MAP_MAX_CELLS;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_mcl_abi_version(void) { return VISFS_MCL_ABI_VERSION; }

void visfs_mcl_field_default_params(visfs_mcl_field_params* p) {
    if (!p) return;
    p->occupied_probability = 0.65; p->max_dist = 2.0; p->z_hit = 0.5; p->z_rand = 0.5; p->sigma_hit = 0.2; p->range_max = 12.0;
}

void visfs_mcl_default_params(visfs_mcl_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->alpha1 = p->alpha2 = p->alpha3 = p->alpha4 = 0.2;
    p->n_eff_ratio = 1.0; p->resample_interval = 2; p->max_beams = 0;
}

int visfs_mcl_field_create_from_map(visfs_map* m, const visfs_mcl_field_params* p, visfs_mcl_field** out) {
    if (!m || !p || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        gmap::MapAccess a;
        int rc = visfs_internal_map_access(m, &a);
        if (rc != VISFS_BA_OK) return rc;
        if (!a.have || !limits_ok(a.L)) return (int)VISFS_BA_ERR_BAD_ARGUMENT;         // no composed grid
        visfs_mcl_field* f = nullptr;
        const char* why = "";
        if ((rc = field_new(a.L, *p, &f, &why)) != VISFS_BA_OK) return rc;
        f->device = a.device; f->dev = a.dev; f->stream = a.stream;
        if ((rc = field_build(f, a.cells)) != VISFS_BA_OK) { delete f; return rc; }
        *out = f;
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_field_create_from_grid(visfs_ba_handle* h, const visfs_submap_info* limits, const uint16_t* cells, const visfs_mcl_field_params* p,
                                     visfs_mcl_field** out) {
    if (!limits || !cells || !p || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        const Limits L = submap::limits_of(*limits);
        if (!limits_ok(L)) return (int)VISFS_BA_ERR_BAD_ARGUMENT;
        visfs_mcl_field* f = nullptr;
        const char* why = "";
        int rc = field_new(L, *p, &f, &why);
        if (rc != VISFS_BA_OK) { if (h) visfs_internal_set_error(h, why); return rc; }
        if (!h) {
            if ((rc = field_build(f, cells)) != VISFS_BA_OK) { delete f; return rc; }
            *out = f;
            return (int)VISFS_BA_OK;
        }
        f->device = true; f->dev = visfs_internal_device(h); f->stream = visfs_internal_stream(h);
        rc = field_build_uploaded(f, cells);
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, "the likelihood field could not be built on the device"); delete f; return rc; }
        *out = f;
        return (int)VISFS_BA_OK;
    });
}

void visfs_mcl_field_destroy(visfs_mcl_field* f) { delete f; }

int visfs_mcl_field_describe(const visfs_mcl_field* f, visfs_mcl_field_info* info) {
    if (!f || !info) return VISFS_BA_ERR_BAD_ARGUMENT;
    std::memset(info, 0, sizeof *info);
    visfs_submap_info& l = info->limits;
    l.resolution = f->L.res; l.max_x = f->L.max_x; l.max_y = f->L.max_y; l.num_x_cells = f->L.nx; l.num_y_cells = f->L.ny;
    l.known_min_x = l.known_min_y = 1;
    info->R = f->R; info->T = f->T; info->v_occ = f->v_occ; info->device = f->device ? 1 : 0;
    return VISFS_BA_OK;
}

int visfs_mcl_field_download(visfs_mcl_field* f, uint16_t* t, int64_t* q, int32_t* v_occ, int32_t* T) {
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int {
        const size_t n = (size_t)f->L.nx * f->L.ny;
        if (t) {
            if (!f->device) std::memcpy(t, f->h_t.data(), n * 2);
            else {
                HIP_TRY(nullptr, hipSetDevice(f->dev));
                HIP_TRY(nullptr, hipMemcpyAsync(t, f->d_t.get(), n * 2, hipMemcpyDeviceToHost, f->stream));
                HIP_TRY(nullptr, hipStreamSynchronize(f->stream));
            }
        }
        if (q) {
            if (!f->device) std::memcpy(q, f->h_q.data(), f->h_q.size() * sizeof(int64_t));
            else {                                                                     // what the device holds, not the host's copy
                HIP_TRY(nullptr, hipSetDevice(f->dev));
                HIP_TRY(nullptr, hipMemcpyAsync(q, f->d_q.get(), f->h_q.size() * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
                HIP_TRY(nullptr, hipStreamSynchronize(f->stream));
            }
        }
        if (v_occ) *v_occ = f->v_occ;
        if (T) *T = f->T;
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_field_last_counts(const visfs_mcl_field* f, int32_t* launches, int32_t* copies, int32_t* waits) {
    return f ? f->counts.read(launches, copies, waits) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

int visfs_mcl_create(visfs_mcl_field* field, int32_t n_particles, uint64_t seed, visfs_mcl** out) {
    if (!field || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (n_particles < 1 || n_particles > VISFS_MCL_MAX_PARTICLES) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int {
        visfs_mcl* f = new visfs_mcl();
        f->field = field; f->device = field->device; f->dev = field->dev; f->stream = field->stream;
        f->N = f->n = n_particles; f->seed = seed;
        const size_t N = (size_t)n_particles;
        if (f->device) {
            const int rc = mcl_alloc(f);
            if (rc != VISFS_BA_OK) { delete f; return rc; }
        } else {
            for (auto& v : f->h_st) v.assign(4 * N, 0.0);
            f->h_Q.assign(N, 0); f->h_anc.assign(N, 0);
        }
        *out = f;
        const double zero[3] = { 0.0, 0.0, 0.0 };
        const int rc = visfs_mcl_init(f, zero, zero);                                  // a defined state from the start
        if (rc != VISFS_BA_OK) { *out = nullptr; delete f; return rc; }
        f->counts = {};
        return (int)VISFS_BA_OK;
    });
}

void visfs_mcl_destroy(visfs_mcl* f) { if (f) delete f; }

const char* visfs_mcl_last_error(const visfs_mcl* f) { return f ? f->err.c_str() : "null filter"; }

int visfs_mcl_init(visfs_mcl* f, const double mean[3], const double sigma[3]) {
    if (!f || !mean || !sigma) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        InitHdr I;
        std::memset(&I, 0, sizeof I);
        for (int i = 0; i < 3; ++i) {
            if (!std::isfinite(mean[i]) || !(std::isfinite(sigma[i]) && sigma[i] >= 0.0)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the mean must be finite, the sigmas finite and not negative");
            I.mean[i] = mean[i]; I.sigma[i] = sigma[i];
        }
        if (std::fabs(mean[2]) + 6.0 * sigma[2] > 3.0 * kPi) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the yaw would need more than one wrap");
        I.mean[2] = wrap(mean[2]);
        if (!(std::fabs(I.mean[2]) + 6.0 * sigma[2] <= 3.0 * kPi)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the yaw would need more than one wrap");
        I.inv_n = 1.0 / (double)f->N; I.seed = f->seed; I.N = f->N;
        const size_t N = (size_t)f->N;
        if (!f->device) {
            double* st = f->h_st[0].data();
            for (size_t j = 0; j < N; ++j) {
                init_particle(I, (int32_t)j, st[j], st[N + j], st[2 * N + j]);
                st[3 * N + j] = I.inv_n;
                f->h_Q[j] = 0; f->h_anc[j] = (int32_t)j;
            }
            f->counts = {};
        } else {
            HIP_TRY(f, hipSetDevice(f->dev));
            std::memcpy(f->h_up.get(), &I, sizeof I);
            HIP_TRY(f, hipMemcpyAsync(f->d_up.get(), f->h_up.get(), sizeof I, hipMemcpyHostToDevice, f->stream));
            hipLaunchKernelGGL(k_mcl_init, dim3(blocks_for(f->N, kThreads)), dim3(kThreads), 0, f->stream, reinterpret_cast<const InitHdr*>(f->d_up.get()), f->d_st[0].get(),
                               f->d_Q.get(), f->d_anc.get());
            HIP_TRY(f, hipGetLastError());
            HIP_TRY(f, hipStreamSynchronize(f->stream));
            f->counts = { VISFS_MCL_INIT_LAUNCHES, 1, 1 };
        }
        f->cur = 0; f->update = 0; f->n = f->N;
        if (f->kld) kld_particles_replaced(f);
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_update(visfs_mcl* f, const visfs_mcl_params* p, const double odom_delta[3], int32_t n, const double* points_xyz,
                     visfs_mcl_result* result) {
    if (!f || !p || !odom_delta || (n > 0 && !points_xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (n < 0 || n > VISFS_MCL_MAX_BEAMS) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the points must number 0 .. 16384");
        if (p->resample_interval < 1 || p->max_beams < 0 || !(std::isfinite(p->n_eff_ratio) && p->n_eff_ratio >= 0.0))
            return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "resample_interval >= 1, max_beams >= 0 and a finite n_eff_ratio >= 0 are needed");
        Hdr H;
        std::memset(&H, 0, sizeof H);
        const char* why = "";
        const int rc = motion_plan(*p, odom_delta, H.M, &why);
        if (rc != VISFS_BA_OK) return fail(f, rc, why);
        const int32_t step = p->max_beams > 0 ? (n + p->max_beams - 1) / p->max_beams : 1;
        std::vector<double> beams;
        for (int32_t i = 0; i < n; i += (step > 0 ? step : 1)) {
            const double px = points_xyz[3 * (size_t)i], py = points_xyz[3 * (size_t)i + 1];
            if (!(std::fabs(px) <= 1e6) || !(std::fabs(py) <= 1e6)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "a point is not finite");
            beams.push_back(px); beams.push_back(py);
        }
        H.n = (int32_t)(beams.size() / 2);
        const int32_t n_before = f->n;
        H.N = n_before; H.P = pow2_at_least(n_before);
        H.ratio_n = p->n_eff_ratio * (double)n_before; H.inv_n = 1.0 / (double)n_before;
        H.seed = f->seed; H.update = (uint64_t)(f->update + 1);
        H.gate = ((f->update + 1) % p->resample_interval) == 0 ? 1 : 0;
        H.lanes = lanes_for(f, H.n);
        Rec rec;
        std::memset(&rec, 0, sizeof rec);
        if (f->device) { const int rd = device_update(f, H, beams, rec); if (rd != VISFS_BA_OK) return rd; }
        else { host_update(f, H, beams, rec); f->counts = {}; }
        f->update += 1;
        if (rec.resampled) f->cur ^= 1;
        if (f->kld) kld_commit(f, rec, n_before);
        finalize(rec, H.n, f->update, f->last);
        f->have_last = true;
        if (result) *result = f->last;
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_last_result(const visfs_mcl* f, visfs_mcl_result* result) {
    if (!f || !result) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->have_last) { std::memset(result, 0, sizeof *result); result->status = VISFS_BA_ERR_BAD_ARGUMENT; return VISFS_BA_ERR_BAD_ARGUMENT; }
    *result = f->last;
    return VISFS_BA_OK;
}

int visfs_mcl_download(visfs_mcl* f, double* x, double* y, double* yaw, double* w, int64_t* Q, int32_t* ancestors) {
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        const size_t N = (size_t)f->n;                                                 // the active count, and the arrays' stride
        double* dst[4] = { x, y, yaw, w };
        if (!f->device) {
            for (int k = 0; k < 4; ++k) if (dst[k]) std::memcpy(dst[k], f->h_st[f->cur].data() + k * N, N * sizeof(double));
            if (Q) std::memcpy(Q, f->h_Q.data(), N * sizeof(int64_t));
            if (ancestors) std::memcpy(ancestors, f->h_anc.data(), N * sizeof(int32_t));
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(f, hipSetDevice(f->dev));
        for (int k = 0; k < 4; ++k)
            if (dst[k]) HIP_TRY(f, hipMemcpyAsync(dst[k], f->d_st[f->cur].get() + k * N, N * sizeof(double), hipMemcpyDeviceToHost, f->stream));
        if (Q) HIP_TRY(f, hipMemcpyAsync(Q, f->d_Q.get(), N * sizeof(int64_t), hipMemcpyDeviceToHost, f->stream));
        if (ancestors) HIP_TRY(f, hipMemcpyAsync(ancestors, f->d_anc.get(), N * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_upload(visfs_mcl* f, const double* x, const double* y, const double* yaw, const double* w) {
    if (!f || !x || !y || !yaw || !w) return VISFS_BA_ERR_BAD_ARGUMENT;
    return upload_n(f, f->N, x, y, yaw, w);
}

}  // extern "C"

int mcl::upload_n(visfs_mcl* f, int32_t n, const double* x, const double* y, const double* yaw, const double* w) {
    return guarded(f, [&]() -> int {
        const size_t N = (size_t)n;
        double sum = 0.0;
        for (size_t j = 0; j < N; ++j) {
            if (!(std::fabs(x[j]) <= 1e9) || !(std::fabs(y[j]) <= 1e9) || !(yaw[j] > -kPi && yaw[j] <= kPi) || !(std::isfinite(w[j]) && w[j] >= 0.0))
                return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "finite poses, yaw in (-pi, pi] and finite weights >= 0 are needed");
            sum += w[j];
        }
        if (!(std::isfinite(sum) && sum > 0.0)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the weights need a positive finite sum");
        const double* src[4] = { x, y, yaw, w };
        if (!f->device) {
            for (int k = 0; k < 4; ++k) std::memcpy(f->h_st[f->cur].data() + k * N, src[k], N * sizeof(double));
            f->n = n;
            if (f->kld) kld_particles_replaced(f);
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(f, hipSetDevice(f->dev));
        for (int k = 0; k < 4; ++k) HIP_TRY(f, hipMemcpyAsync(f->d_st[f->cur].get() + k * N, src[k], N * sizeof(double), hipMemcpyHostToDevice, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        f->n = n;
        if (f->kld) kld_particles_replaced(f);
        return (int)VISFS_BA_OK;
    });
}

extern "C" {

int visfs_mcl_hook_set_lanes(visfs_mcl* f, int32_t lanes) {
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (lanes != 0 && (lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0)) return VISFS_BA_ERR_BAD_ARGUMENT;
    f->lanes = lanes;
    return VISFS_BA_OK;
}

int visfs_mcl_last_counts(const visfs_mcl* f, int32_t* launches, int32_t* copies, int32_t* waits) {
    return f ? f->counts.read(launches, copies, waits) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

int visfs_mcl_hook_sincos(int32_t n, const double* a, double* s, double* c) {
    if (n < 0 || (n > 0 && (!a || !s || !c))) return VISFS_BA_ERR_BAD_ARGUMENT;
    for (int32_t i = 0; i < n; ++i) {
        if (!(std::fabs(a[i]) <= 16.0)) return VISFS_BA_ERR_BAD_ARGUMENT;
        sincos_any(a[i], s[i], c[i]);
    }
    return VISFS_BA_OK;
}

}  // extern "C"
