// ba_pnp.hip — the PnP-RANSAC pose guess (include/visfs_pnp.h): two kernels and the two flavours of the object.
//
//   k_pnp_ransac   one wavefront per hypothesis, four per workgroup.  The workgroup stages the rows in LDS once; every lane of a
//                  wavefront draws the same sample and runs the same P3P (uniform, as the scalar tail of k_flow_lk), then the lanes
//                  take rows strided and __ballot + popcount give the inlier count.  One 64-bit atomicMax of
//                  (count << 32) | (0xFFFFFFFF - h) picks the winner, lowest h on a tie, whatever the arrival order.
//   k_pnp_refine   one workgroup: the winner's inlier list, the refit on it and the whole refinement loop of solvePnPRansac, nothing
//                  going back to the host between passes.  The two row lists and the error list live in LDS; the model is carried
//                  by every thread with the same value, the reductions hand their results round through LDS.
//
// A call is one copy in (a zeroed header with the winner key, the kept rows), the two launches and one copy out (the result block and
// the inlier list).  The covariance is computed on the host in both flavours.  The arithmetic is ba_pnp.hpp.
//
// The resident tracker (include/visfs_tracker_pnp.h) runs the same two stages on rows that never leave the
// device: k_pnp_ransac_g and k_pnp_refine_g read their member's PnpRec at blockIdx.z and m from device memory (pnp::group_pnp) and
// share their bodies with the by-value kernels.
#include "ba_pnp.hpp"
#include "ba_flow.hpp"
#include "ba_group.hpp"      // pnp::group_pnp, pnp::check_params, pnp::finalize
#include "ba_host.hpp"
#include "../../include/visfs_pnp.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace pnp;
using namespace host;

namespace pnp {

constexpr int PN_T = 256;
constexpr size_t kHeaderBytes = 256;       // the winner key, then the rows / the Result, then the inlier list

struct RansacArgs {
    const Row* rows;
    int32_t m, iterations;
    uint64_t seed;
    Cam K;
    float thr;
    int32_t* samples;      // [iterations][4]
    int32_t* vc;           // [iterations][2]: valid, count
    double* models;        // [iterations][12]
    unsigned long long* key;
};

BA_HD void store_model(double* o, bool ok, const Rt& T) {
    o[0] = ok ? T.R.m00 : 0.0; o[1] = ok ? T.R.m01 : 0.0; o[2] = ok ? T.R.m02 : 0.0; o[3] = ok ? T.t.x : 0.0;
    o[4] = ok ? T.R.m10 : 0.0; o[5] = ok ? T.R.m11 : 0.0; o[6] = ok ? T.R.m12 : 0.0; o[7] = ok ? T.t.y : 0.0;
    o[8] = ok ? T.R.m20 : 0.0; o[9] = ok ? T.R.m21 : 0.0; o[10] = ok ? T.R.m22 : 0.0; o[11] = ok ? T.t.z : 0.0;
}
BA_HD Rt load_model(const double* o) {
    Rt T;
    T.R = Mat3{ o[0], o[1], o[2], o[4], o[5], o[6], o[8], o[9], o[10] };
    T.t = Vec3{ o[3], o[7], o[11] };
    return T;
}

// One body for the by-value kernel of the staged call and the record-reading kernel of the resident tracker.
__device__ __forceinline__ void pnp_ransac_body(const RansacArgs& A) {
    __shared__ Row s_rows[kMaxPoints];
    {
        const float* src = reinterpret_cast<const float*>(A.rows);
        float* dst = reinterpret_cast<float*>(s_rows);
        for (int i = threadIdx.x; i < 5 * A.m; i += PN_T) dst[i] = src[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = blockIdx.x * (PN_T / 64) + wave;
    if (h >= A.iterations) return;
    int32_t s[4];
    sample4(A.seed, h, A.m, s);
    Rt T;
    const bool ok = p3p_solve(A.K, s_rows[s[0]], s_rows[s[1]], s_rows[s[2]], s_rows[s[3]], T);
    int count = 0;
    if (ok) {
        for (int base = 0; base < A.m; base += 64) {
            const int i = base + lane;
            const bool in = i < A.m && reproj_error(T, A.K, s_rows[i]) <= A.thr;
            count += __popcll(__ballot(in));
        }
    }
    if (lane == 0) {
        A.samples[4 * h] = s[0]; A.samples[4 * h + 1] = s[1]; A.samples[4 * h + 2] = s[2]; A.samples[4 * h + 3] = s[3];
        A.vc[2 * h] = ok ? 1 : 0; A.vc[2 * h + 1] = count;
        store_model(A.models + 12 * (size_t)h, ok, T);
        if (ok) atomicMax(A.key, ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)h));
    }
}

__global__ __launch_bounds__(PN_T) void k_pnp_ransac(RansacArgs A) { pnp_ransac_body(A); }

// Member blockIdx.z of a tracker call: m comes from device memory.  Fewer rows than min_inliers: nothing of the pose guess runs for
// the member (the rows kernel has written its result).  The record's fields go into the argument struct once, in front of the body.
__global__ __launch_bounds__(PN_T) void k_pnp_ransac_g(const PnpRec* __restrict__ recs, PnpShape S) {
    const PnpRec* r = recs + blockIdx.z;
    if (r->skip) return;
    const int32_t m = min(*r->m, kMaxPoints);
    if (m < S.min_inliers || (int)blockIdx.x * (PN_T / 64) >= S.iterations) return;
    RansacArgs A;
    A.rows = r->rows; A.m = m; A.iterations = S.iterations; A.seed = S.seed; A.K = r->K; A.thr = S.thr;
    A.samples = r->samples; A.vc = r->vc; A.models = r->models; A.key = r->key;
    pnp_ransac_body(A);
}

struct RefineArgs {
    const Row* rows;
    int32_t m, cap;
    Cam K;
    int32_t min_inliers, refine_iterations;
    float thr0, sigma;
    const unsigned long long* key;
    const double* models;
    Result* res;
    int32_t* inliers;      // [m]
    double* pass_tq;       // [kMaxRefine][7]
    float* pass_thr;
    int32_t* pass_cnt;
    int32_t* pass_lists;   // [kMaxRefine][cap]
};

struct DevicePolicy {
    const RefineArgs& A;
    int32_t (*lists)[kMaxPoints];
    float* errs;
    double (*red)[28];
    int32_t* wcount;
    float* mv;
    int tid, wave, lane;

    __device__ void sums(const Rt& T, const Cam& K, int list, int n, double acc[28], bool full) {
        double a[28];
#pragma unroll
        for (int q = 0; q < 28; ++q) a[q] = 0.0;
        for (int k = tid; k < n; k += kSlots) {
            const Row r = A.rows[lists[list][k]];
            if (full) normal_row(T, K, r, a);
            else a[27] += cost_row(T, K, r);
        }
#pragma unroll
        for (int q = 0; q < 28; ++q) {
            if (!full && q != 27) continue;
            double v = a[q];
#pragma unroll
            for (int st = 32; st >= 1; st >>= 1) v += __shfl_down(v, st, 64);
            if (lane == 0) red[wave][q] = v;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 28; ++q) {
            if (!full && q != 27) continue;
            acc[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
        }
        __syncthreads();
    }
    __device__ int select(const Rt& T, const Cam& K, float thr, int list) {
        int base = 0;
        for (int c0 = 0; c0 < A.m; c0 += PN_T) {
            const int i = c0 + tid;
            float e = 0.0f;
            bool in = false;
            if (i < A.m) { e = reproj_error(T, K, A.rows[i]); in = e <= thr; }
            const unsigned long long b = __ballot(in);
            if (lane == 0) wcount[wave] = __popcll(b);
            __syncthreads();
            int off = base, total = 0;
#pragma unroll
            for (int w = 0; w < PN_T / 64; ++w) { if (w < wave) off += wcount[w]; total += wcount[w]; }
            if (in) {
                const int pos = off + __popcll(b & ((1ull << lane) - 1ull));
                lists[list][pos] = i;
                errs[pos] = e;
            }
            base += total;
            __syncthreads();
        }
        return base;
    }
    __device__ void spread(int n, float& mean, float& var) {
        if (tid == 0) {                                   // one lane, in list order: that order is the definition
            float buf = 0.0f;
            for (int i = 0; i < n; ++i) buf += errs[i];
            buf /= (float)n;
            double sum = 0.0;
            for (int i = 0; i < n; ++i) sum += (double)((errs[i] - buf) * (errs[i] - buf));
            mv[0] = buf;
            mv[1] = (float)(sum / (double)(n - 1));
        }
        __syncthreads();
        mean = mv[0]; var = mv[1];
        __syncthreads();
    }
    __device__ bool same(int n) {
        int diff = 0;
        for (int k = tid; k < n; k += PN_T) diff |= lists[0][k] != lists[1][k];
        return !__syncthreads_or(diff);
    }
    __device__ void record(int pass, const double tq[7], float thr, int list, int n) {
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 7; ++i) A.pass_tq[7 * pass + i] = tq[i];
            A.pass_thr[pass] = thr; A.pass_cnt[pass] = n;
        }
        for (int k = tid; k < n; k += PN_T) A.pass_lists[(size_t)pass * A.cap + k] = lists[list][k];
    }
    __device__ void finish(int list, int n) {
        for (int k = tid; k < n; k += PN_T) A.inliers[k] = lists[list][k];
    }
};

// The refinement from a start model: what the winner-reading body below and the refine-only kernel share.
template <bool Polish>
__device__ __forceinline__ void pnp_refine_run(const RefineArgs& A, bool have_winner, const Rt& W, Result& res) {
    __shared__ int32_t s_lists[2][kMaxPoints];
    __shared__ float s_errs[kMaxPoints];
    __shared__ double s_red[PN_T / 64][28];
    __shared__ int32_t s_wcount[PN_T / 64];
    __shared__ float s_mv[2];
    DevicePolicy pol{ A, s_lists, s_errs, s_red, s_wcount, s_mv, (int)threadIdx.x, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63) };
    refine_all<DevicePolicy, Polish>(pol, A.K, have_winner, W, A.min_inliers, A.refine_iterations, A.thr0, A.sigma, res);
    if (threadIdx.x == 0) *A.res = res;
}

__device__ __forceinline__ void pnp_refine_body(const RefineArgs& A) {
    const unsigned long long key = *A.key;
    Result res;
    res.winner = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
    res.winner_count = (int32_t)(key >> 32);
    Rt W = load_model(A.models + 12 * (size_t)(key ? res.winner : 0));
    pnp_refine_run<false>(A, key != 0, W, res);
}

__global__ __launch_bounds__(PN_T) void k_pnp_refine(RefineArgs A) { pnp_refine_body(A); }

__global__ __launch_bounds__(PN_T) void k_pnp_refine_g(const PnpRec* __restrict__ recs, PnpShape S) {
    const PnpRec* r = recs + blockIdx.z;
    if (r->skip) return;
    const int32_t m = min(*r->m, kMaxPoints);
    if (m < S.min_inliers) return;
    RefineArgs A;
    A.rows = r->rows; A.m = m; A.cap = r->cap; A.K = r->K; A.min_inliers = S.min_inliers; A.refine_iterations = S.refine_iterations;
    A.thr0 = S.thr; A.sigma = S.sigma; A.key = r->key; A.models = r->models; A.res = r->res; A.inliers = r->inliers;
    A.pass_tq = r->pass_tq; A.pass_thr = r->pass_thr; A.pass_cnt = r->pass_cnt; A.pass_lists = r->pass_lists;
    pnp_refine_body(A);
}

// Member blockIdx.z of a refine-only call (include/visfs_place_verify.h): no search, the loop of section 9e
// steps 5 and 6 on the member's rows started from the model another call has left in device memory.
__global__ __launch_bounds__(PN_T) void k_pnp_refine_from_g(const RefineFromRec* __restrict__ recs, PnpShape S) {
    const RefineFromRec* r = recs + blockIdx.z;
    if (!*r->ran) return;
    const int32_t m = min(*r->m, kMaxPoints);
    if (m < S.min_inliers) return;
    RefineArgs A;
    A.rows = r->rows; A.m = m; A.cap = r->cap; A.K = r->K; A.min_inliers = S.min_inliers; A.refine_iterations = S.refine_iterations;
    A.thr0 = S.thr; A.sigma = S.sigma; A.key = nullptr; A.models = nullptr; A.res = r->res; A.inliers = r->inliers;
    A.pass_tq = r->pass_tq; A.pass_thr = r->pass_thr; A.pass_cnt = r->pass_cnt; A.pass_lists = r->pass_lists;
    Result res;
    res.winner = -1; res.winner_count = 0;
    double tq[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) tq[i] = r->start->tq[i];
    const Rt W = tq_to_rt(tq);
    pnp_refine_run<true>(A, true, W, res);
}

int group_refine_from(hipStream_t stream, int n, const RefineFromRec* d_recs, const PnpShape& S, flow::GroupCounts* cnt) {
    hipLaunchKernelGGL(k_pnp_refine_from_g, dim3(1, 1, (unsigned)n), dim3(PN_T), 0, stream, d_recs, S);
    if (hipGetLastError() != hipSuccess) return VISFS_BA_ERR_DEVICE;
    ++cnt->launches;
    return VISFS_BA_OK;
}

int group_pnp(hipStream_t stream, int n, const PnpRec* d_recs, const PnpShape& S, flow::GroupCounts* cnt) {
    hipLaunchKernelGGL(k_pnp_ransac_g, dim3((unsigned)((S.iterations + PN_T / 64 - 1) / (PN_T / 64)), 1, (unsigned)n), dim3(PN_T), 0, stream,
                       d_recs, S);
    if (hipGetLastError() != hipSuccess) return VISFS_BA_ERR_DEVICE;
    ++cnt->launches;
    hipLaunchKernelGGL(k_pnp_refine_g, dim3(1, 1, (unsigned)n), dim3(PN_T), 0, stream, d_recs, S);
    if (hipGetLastError() != hipSuccess) return VISFS_BA_ERR_DEVICE;
    ++cnt->launches;
    return VISFS_BA_OK;
}

}  // namespace pnp

// ====================================================================== the object
struct visfs_pnp {
    int32_t cap = 0;
    std::string err;
    bool device = false;
    bool solved = false;
    int32_t last_m = 0, last_hyp = 0, last_passes = 0;
    Result res{};

    // host twin: what visfs_pnp_download reads
    std::vector<Row> rows;
    std::vector<int32_t> samples, vc, pass_cnt, pass_lists;
    std::vector<double> models, pass_tq;
    std::vector<float> pass_thr;

    // device
    visfs_ba_handle* ba = nullptr;
    int dev = 0;
    hipStream_t stream = nullptr;
    PinnedBuf<char> h_in;      // pinned: header + rows
    PinnedBuf<char> h_out;     // pinned: Result + inlier list
    DeviceBuf<char> d_in;
    DeviceBuf<char> d_out;
    DeviceBuf<char> d_state;   // hypotheses and passes
    int32_t *d_samples = nullptr, *d_vc = nullptr, *d_pass_cnt = nullptr, *d_pass_lists = nullptr;
    double *d_models = nullptr, *d_pass_tq = nullptr;
    float* d_pass_thr = nullptr;

    ~visfs_pnp() {                     // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

int device_init(visfs_pnp* p) {
    HIP_TRY(p, hipSetDevice(p->dev));
    const size_t cap = (size_t)p->cap;
    const size_t in_bytes = kHeaderBytes + up256(sizeof(Row) * cap), out_bytes = kHeaderBytes + up256(4 * cap);
    static_assert(sizeof(Result) <= kHeaderBytes, "the result block is one header");
    RC_TRY(p->h_in.alloc(p, in_bytes));
    RC_TRY(p->h_out.alloc(p, out_bytes));
    RC_TRY(p->d_in.alloc(p, in_bytes));
    RC_TRY(p->d_out.alloc(p, out_bytes));
    const size_t H = kMaxHypotheses, R = kMaxRefine;
    const size_t o_models = 0, o_ptq = o_models + up256(96 * H), o_samples = o_ptq + up256(56 * R), o_vc = o_samples + up256(16 * H),
                 o_pthr = o_vc + up256(8 * H), o_pcnt = o_pthr + up256(4 * R), o_plists = o_pcnt + up256(4 * R),
                 bytes = o_plists + up256(4 * R * cap);
    RC_TRY(p->d_state.alloc(p, bytes));
    p->d_models = reinterpret_cast<double*>(p->d_state.get() + o_models);
    p->d_pass_tq = reinterpret_cast<double*>(p->d_state.get() + o_ptq);
    p->d_samples = reinterpret_cast<int32_t*>(p->d_state.get() + o_samples);
    p->d_vc = reinterpret_cast<int32_t*>(p->d_state.get() + o_vc);
    p->d_pass_thr = reinterpret_cast<float*>(p->d_state.get() + o_pthr);
    p->d_pass_cnt = reinterpret_cast<int32_t*>(p->d_state.get() + o_pcnt);
    p->d_pass_lists = reinterpret_cast<int32_t*>(p->d_state.get() + o_plists);
    return VISFS_BA_OK;
}

// The host twin's reductions: the same leaves and the same tree as DevicePolicy, in sequence.
struct HostPolicy {
    visfs_pnp* p;
    const Row* rows;
    int32_t m;
    std::vector<int32_t> lists[2];
    std::vector<float> errs;
    std::vector<int32_t> out;

    void sums(const Rt& T, const Cam& K, int list, int n, double acc[28], bool full) {
        static thread_local double slot[kSlots][28];
        for (int s = 0; s < kSlots; ++s) {
            for (int q = 0; q < 28; ++q) slot[s][q] = 0.0;
            for (int k = s; k < n; k += kSlots) {
                const Row r = rows[lists[list][k]];
                if (full) normal_row(T, K, r, slot[s]);
                else slot[s][27] += cost_row(T, K, r);
            }
        }
        for (int q = 0; q < 28; ++q) {
            if (!full && q != 27) continue;
            for (int g = 0; g < kSlots; g += 64)
                for (int st = 32; st >= 1; st >>= 1)
                    for (int l = 0; l < st; ++l) slot[g + l][q] += slot[g + l + st][q];
            acc[q] = (slot[0][q] + slot[64][q]) + (slot[128][q] + slot[192][q]);
        }
    }
    int select(const Rt& T, const Cam& K, float thr, int list) {
        int n = 0;
        for (int i = 0; i < m; ++i) {
            const float e = reproj_error(T, K, rows[i]);
            if (e <= thr) { lists[list][n] = i; errs[n] = e; ++n; }
        }
        return n;
    }
    void spread(int n, float& mean, float& var) {
        float buf = 0.0f;
        for (int i = 0; i < n; ++i) buf += errs[i];
        buf /= (float)n;
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += (double)((errs[i] - buf) * (errs[i] - buf));
        mean = buf;
        var = (float)(sum / (double)(n - 1));
    }
    bool same(int n) { return std::equal(lists[0].begin(), lists[0].begin() + n, lists[1].begin()); }
    void record(int pass, const double tq[7], float thr, int list, int n) {
        for (int i = 0; i < 7; ++i) p->pass_tq[7 * pass + i] = tq[i];
        p->pass_thr[pass] = thr; p->pass_cnt[pass] = n;
        std::copy(lists[list].begin(), lists[list].begin() + n, p->pass_lists.begin() + (size_t)pass * m);
    }
    void finish(int list, int n) { out.assign(lists[list].begin(), lists[list].begin() + n); }
};

int host_solve(visfs_pnp* p, const visfs_pnp_params& prm, const Cam& K, int32_t m, int min_inliers, std::vector<int32_t>& inliers) {
    const int H = prm.iterations;
    p->samples.assign(4 * (size_t)H, 0); p->vc.assign(2 * (size_t)H, 0); p->models.assign(12 * (size_t)H, 0.0);
    p->pass_tq.assign(7 * kMaxRefine, 0.0); p->pass_thr.assign(kMaxRefine, 0.0f); p->pass_cnt.assign(kMaxRefine, 0);
    p->pass_lists.assign((size_t)kMaxRefine * m, 0);
    const Row* rows = p->rows.data();
    unsigned long long key = 0;
    for (int h = 0; h < H; ++h) {
        int32_t s[4];
        sample4(prm.seed, h, m, s);
        Rt T{};
        const bool ok = p3p_solve(K, rows[s[0]], rows[s[1]], rows[s[2]], rows[s[3]], T);
        int count = 0;
        if (ok) for (int i = 0; i < m; ++i) count += reproj_error(T, K, rows[i]) <= prm.reproj_error;
        for (int k = 0; k < 4; ++k) p->samples[4 * h + k] = s[k];
        p->vc[2 * h] = ok; p->vc[2 * h + 1] = count;
        store_model(p->models.data() + 12 * (size_t)h, ok, T);
        if (ok) key = std::max(key, ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)h));
    }
    HostPolicy pol;
    pol.p = p; pol.rows = rows; pol.m = m;
    pol.lists[0].assign(m, 0); pol.lists[1].assign(m, 0); pol.errs.assign(m, 0.0f);
    Result& res = p->res;
    res.winner = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)) : -1;
    res.winner_count = (int32_t)(key >> 32);
    const Rt W = load_model(p->models.data() + 12 * (size_t)(key ? res.winner : 0));
    refine_all(pol, K, key != 0, W, min_inliers, prm.refine_iterations, prm.reproj_error, prm.refine_sigma, res);
    inliers = pol.out;
    return VISFS_BA_OK;
}

int device_solve(visfs_pnp* p, const visfs_pnp_params& prm, const Cam& K, int32_t m, int min_inliers, std::vector<int32_t>& inliers) {
    HIP_TRY(p, hipSetDevice(p->dev));
    // (the rows were written into h_in behind the header by the caller, after the stream had drained)
    std::memset(p->h_in.get(), 0, kHeaderBytes);
    HIP_TRY(p, hipMemcpyAsync(p->d_in.get(), p->h_in.get(), kHeaderBytes + sizeof(Row) * (size_t)m, hipMemcpyHostToDevice, p->stream));
    RansacArgs A;
    A.rows = reinterpret_cast<const Row*>(p->d_in.get() + kHeaderBytes); A.m = m; A.iterations = prm.iterations; A.seed = prm.seed; A.K = K;
    A.thr = prm.reproj_error; A.samples = p->d_samples; A.vc = p->d_vc; A.models = p->d_models;
    A.key = reinterpret_cast<unsigned long long*>(p->d_in.get());
    hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)((prm.iterations + PN_T / 64 - 1) / (PN_T / 64))), dim3(PN_T), 0, p->stream, A);
    HIP_TRY(p, hipGetLastError());
    RefineArgs B;
    B.rows = A.rows; B.m = m; B.cap = p->cap; B.K = K; B.min_inliers = min_inliers; B.refine_iterations = prm.refine_iterations;
    B.thr0 = prm.reproj_error; B.sigma = prm.refine_sigma; B.key = A.key; B.models = p->d_models;
    B.res = reinterpret_cast<Result*>(p->d_out.get()); B.inliers = reinterpret_cast<int32_t*>(p->d_out.get() + kHeaderBytes);
    B.pass_tq = p->d_pass_tq; B.pass_thr = p->d_pass_thr; B.pass_cnt = p->d_pass_cnt; B.pass_lists = p->d_pass_lists;
    hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(PN_T), 0, p->stream, B);
    HIP_TRY(p, hipGetLastError());
    HIP_TRY(p, hipMemcpyAsync(p->h_out.get(), p->d_out.get(), kHeaderBytes + 4 * (size_t)m, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::memcpy(&p->res, p->h_out.get(), sizeof(Result));
    if (p->res.n_inliers < 0 || p->res.n_inliers > m) return fail(p, VISFS_BA_ERR_DEVICE, "the device returned an impossible inlier count");
    const int32_t* li = reinterpret_cast<const int32_t*>(p->h_out.get() + kHeaderBytes);
    inliers.assign(li, li + p->res.n_inliers);
    return VISFS_BA_OK;
}

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// getAngle3D (utilite/src/Math.cpp:3-11) on the xyz of two Vector4f with w = 0.
float angle3d(const float a[3], const float b[3]) {
    const float na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    float ua[3], ub[3];
    for (int i = 0; i < 3; ++i) { ua[i] = na > 0.0f ? a[i] / na : a[i]; ub[i] = nb > 0.0f ? b[i] / nb : b[i]; }
    float rad = ua[0] * ub[0] + ua[1] * ub[1] + ua[2] * ub[2];
    if (rad < -1.0f) rad = -1.0f;
    else if (rad > 1.0f) rad = 1.0f;
    return (float)std::acos((double)rad);
}

}  // namespace

namespace pnp {

// MultiviewGeometry.cpp:147-205 from the model and the inliers (kept-row numbers), on the host in every flavour (ba_group.hpp).
void finalize(const Result& res, const Row* rows, const double Tir[12], const Cam& K, const int32_t* inliers, size_t n,
              const int32_t* matches, const float* to_xyz, double* T_out, double* cov) {
    const Rt M = tq_to_rt(res.tq);
    const double pnp34[12] = { M.R.m00, M.R.m01, M.R.m02, M.t.x, M.R.m10, M.R.m11, M.R.m12, M.t.y, M.R.m20, M.R.m21, M.R.m22, M.t.z };
    double prod[12], T[12];
    visfs_ba::iso_mul(Tir, pnp34, prod);
    visfs_ba::iso_inv(prod, T);
    for (int i = 0; i < 12; ++i) T_out[i] = T[i];
    T_out[12] = T_out[13] = T_out[14] = 0.0; T_out[15] = 1.0;
    if (to_xyz) {
        std::vector<float> d2, ang;
        for (size_t i = 0; i < n; ++i) {
            const float* q = to_xyz + 3 * (size_t)matches[inliers[i]];
            if (!finite3(q)) continue;
            const Row& r = rows[inliers[i]];
            float np[3];
            for (int k = 0; k < 3; ++k) np[k] = (float)(T[4 * k] * (double)q[0] + T[4 * k + 1] * (double)q[1] + T[4 * k + 2] * (double)q[2] + T[4 * k + 3]);
            const float dx = r.X - np[0], dy = r.Y - np[1], dz = r.Z - np[2];
            d2.push_back(dx * dx + dy * dy + dz * dz);
            const float obj[3] = { r.X, r.Y, r.Z };
            float v1[3], v2[3];
            for (int k = 0; k < 3; ++k) { v1[k] = (float)((double)obj[k] - T[4 * k + 3]); v2[k] = (float)((double)np[k] - T[4 * k + 3]); }
            ang.push_back(angle3d(v1, v2));
        }
        if (!d2.empty()) {
            std::sort(d2.begin(), d2.end());
            std::sort(ang.begin(), ang.end());
            const double md = 2.1981 * (double)d2[d2.size() >> 1], ma = 2.1981 * (double)ang[ang.size() >> 1];
            for (int k = 0; k < 3; ++k) { cov[7 * k] *= md; cov[7 * (k + 3)] *= ma; }
        }
    } else {
        float err = 0.0f;
        for (size_t i = 0; i < n; ++i) {
            const Row& r = rows[inliers[i]];
            double pu, pv;
            project(M, K, r, pu, pv);
            const float dx = r.u - (float)pu, dy = r.v - (float)pv;
            err += dx * dx + dy * dy;
        }
        const double s = (double)std::sqrt(err / (float)n);
        for (int k = 0; k < 6; ++k) cov[7 * k] *= s;
    }
}

int check_params(const visfs_pnp_params& q, const visfs_pnp_camera& c, const char** why_out) {
    const char*& why = *why_out;
    if (!std::isfinite(q.reproj_error) || q.reproj_error < 0.0f || !std::isfinite(q.refine_sigma) || q.refine_sigma < 0.0f) {
        why = "a threshold is not finite or is negative"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    if (q.iterations < 1) { why = "iterations must be at least 1"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (q.refine_iterations < 0) { why = "refine_iterations must not be negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (q.iterations > kMaxHypotheses) { why = "iterations above 4096"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (q.refine_iterations > kMaxRefine) { why = "refine_iterations above 32"; return VISFS_BA_ERR_UNSUPPORTED; }
    bool fin = std::isfinite(c.fx) && std::isfinite(c.fy) && std::isfinite(c.cx) && std::isfinite(c.cy) && c.fx != 0.0 && c.fy != 0.0;
    for (int i = 0; i < 12; ++i) fin = fin && std::isfinite(c.Tir[i]);
    if (!fin) { why = "a camera value is not finite or a focal length is zero"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    return VISFS_BA_OK;
}

const Result& last_result(const visfs_pnp* p) { return p->res; }

// The twin of k_pnp_refine_from_g on a host solver, which keeps the state visfs_pnp_download reports (no hypotheses, the passes).
int host_refine_from(visfs_pnp* p, const Row* rows, int32_t m, const Cam& K, const PnpShape& S, const double start_tq[7], Result* res,
                     std::vector<int32_t>* inliers) {
    if (!p || p->device || m < 0 || m > p->cap) return VISFS_BA_ERR_BAD_ARGUMENT;
    p->rows.assign(rows, rows + m);
    p->samples.clear(); p->vc.clear(); p->models.clear();
    p->pass_tq.assign(7 * kMaxRefine, 0.0); p->pass_thr.assign(kMaxRefine, 0.0f); p->pass_cnt.assign(kMaxRefine, 0);
    p->pass_lists.assign((size_t)kMaxRefine * m, 0);
    p->solved = true; p->last_m = m; p->last_hyp = 0; p->last_passes = 0;
    p->res = Result{}; p->res.winner = -1;
    inliers->clear();
    if (m >= S.min_inliers) {
        HostPolicy pol;
        pol.p = p; pol.rows = p->rows.data(); pol.m = m;
        pol.lists[0].assign(m, 0); pol.lists[1].assign(m, 0); pol.errs.assign(m, 0.0f);
        const Rt W = tq_to_rt(start_tq);
        refine_all<HostPolicy, true>(pol, K, true, W, S.min_inliers, S.refine_iterations, S.thr, S.sigma, p->res);
        *inliers = pol.out;
        p->last_passes = p->res.n_passes;
    }
    *res = p->res;
    return VISFS_BA_OK;
}

}  // namespace pnp

// ====================================================================== exported C ABI
extern "C" {

int visfs_pnp_abi_version(void) { return VISFS_PNP_ABI_VERSION; }

void visfs_pnp_default_params(visfs_pnp_params* p) {
    if (!p) return;
    p->min_inliers = 12; p->iterations = 50; p->reproj_error = 2.0f; p->refine_iterations = 5; p->refine_sigma = 3.0f; p->seed = 0;
}

int visfs_pnp_create_host(int32_t capacity_points, visfs_pnp** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (capacity_points < 1) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (capacity_points > kMaxPoints) return VISFS_BA_ERR_UNSUPPORTED;
    return guarded(nullptr, [&]() -> int {
        visfs_pnp* p = new visfs_pnp();
        p->cap = capacity_points;
        *out = p;
        return (int)VISFS_BA_OK;
    });
}

int visfs_pnp_create(visfs_ba_handle* h, int32_t capacity_points, visfs_pnp** out) {
    if (!h || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (capacity_points < 1) { visfs_internal_set_error(h, "capacity_points must be at least 1"); return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (capacity_points > kMaxPoints) { visfs_internal_set_error(h, "capacity_points above 4096"); return VISFS_BA_ERR_UNSUPPORTED; }
    return guarded(nullptr, [&]() -> int {
        visfs_pnp* p = new visfs_pnp();
        p->cap = capacity_points;
        p->device = true; p->ba = h; p->dev = visfs_internal_device(h); p->stream = visfs_internal_stream(h);
        const int rc = device_init(p);
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, p->err.c_str()); delete p; return rc; }
        *out = p;
        return (int)VISFS_BA_OK;
    });
}

void visfs_pnp_destroy(visfs_pnp* p) {
    if (!p) return;
    delete p;
}

const char* visfs_pnp_last_error(const visfs_pnp* p) { return p ? p->err.c_str() : "null solver"; }

int visfs_pnp_solve(visfs_pnp* p, const visfs_pnp_params* params, const visfs_pnp_camera* camera, int32_t n, const float* from_xyz,
                    const float* to_xy, const float* to_xyz, double* T_out, double* cov_out, int32_t* matches_out, int32_t* n_matches,
                    int32_t* inliers_out, int32_t* n_inliers) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!params || !camera || !T_out || !cov_out || !n_matches || !n_inliers || n < 0 ||
        (n > 0 && (!from_xyz || !to_xy || !matches_out || !inliers_out)))
        return fail(p, VISFS_BA_ERR_BAD_ARGUMENT, "a required pointer is null or n is negative");
    return guarded(p, [&]() -> int {
        const char* why = "";
        const int rc = check_params(*params, *camera, &why);
        if (rc != VISFS_BA_OK) return fail(p, rc, why);
        if (n > p->cap) return fail(p, VISFS_BA_ERR_BAD_ARGUMENT, "n is above the capacity of the solver");
        if (p->device) {
            HIP_TRY(p, hipSetDevice(p->dev));
            HIP_TRY(p, hipStreamSynchronize(p->stream));            // (the pinned blocks are free again)
        }
        // step 1: the correspondences
        p->rows.clear();
        int32_t m = 0;
        for (int32_t i = 0; i < n; ++i) {
            if (!finite3(from_xyz + 3 * (size_t)i)) continue;
            p->rows.push_back(Row{ from_xyz[3 * (size_t)i], from_xyz[3 * (size_t)i + 1], from_xyz[3 * (size_t)i + 2], to_xy[2 * (size_t)i], to_xy[2 * (size_t)i + 1] });
            matches_out[m++] = i;
        }
        *n_matches = m; *n_inliers = 0;
        for (int i = 0; i < 16; ++i) T_out[i] = 0.0;
        for (int i = 0; i < 36; ++i) cov_out[i] = (i % 7 == 0) ? 1.0 : 0.0;
        const int min_inliers = params->min_inliers < 4 ? 4 : params->min_inliers;
        p->solved = true; p->last_m = m; p->last_hyp = 0; p->last_passes = 0;
        p->res = Result{}; p->res.winner = -1;
        if (m < min_inliers) return (int)VISFS_BA_OK;
        const Cam K{ camera->fx, camera->fy, camera->cx, camera->cy };
        std::vector<int32_t> inliers;
        int rc2;
        if (p->device) {
            std::memcpy(p->h_in.get() + kHeaderBytes, p->rows.data(), sizeof(Row) * (size_t)m);
            rc2 = device_solve(p, *params, K, m, min_inliers, inliers);
        } else {
            rc2 = host_solve(p, *params, K, m, min_inliers, inliers);
        }
        if (rc2 != VISFS_BA_OK) { p->solved = false; return rc2; }
        p->last_hyp = params->iterations; p->last_passes = p->res.n_passes;
        if ((int)inliers.size() < min_inliers) return (int)VISFS_BA_OK;
        finalize(p->res, p->rows.data(), camera->Tir, K, inliers.data(), inliers.size(), matches_out, to_xyz, T_out, cov_out);
        *n_inliers = (int32_t)inliers.size();
        for (size_t i = 0; i < inliers.size(); ++i) inliers_out[i] = matches_out[inliers[i]];
        return (int)VISFS_BA_OK;
    });
}

int visfs_pnp_last_sizes(const visfs_pnp* p, int32_t* m, int32_t* n_hypotheses, int32_t* n_passes) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!p->solved) return VISFS_BA_ERR_NOT_LOADED;
    if (m) *m = p->last_m;
    if (n_hypotheses) *n_hypotheses = p->last_hyp;
    if (n_passes) *n_passes = p->last_passes;
    return VISFS_BA_OK;
}

int visfs_pnp_download(visfs_pnp* p, int32_t* samples, int32_t* valid, double* models, int32_t* counts, int32_t* winner,
                       double* refit_tq, double* pass_tq, float* pass_threshold, int32_t* pass_count, int32_t* pass_inliers) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!p->solved) return fail(p, VISFS_BA_ERR_NOT_LOADED, "no visfs_pnp_solve call yet");
    return guarded(p, [&]() -> int {
        const size_t H = (size_t)p->last_hyp, R = (size_t)p->last_passes, m = (size_t)p->last_m;
        if (winner) *winner = p->res.winner;
        if (refit_tq) for (int i = 0; i < 7; ++i) refit_tq[i] = p->res.refit0[i];
        std::vector<int32_t> h_samples, h_vc, h_pcnt, h_plists;
        std::vector<double> h_models, h_ptq;
        std::vector<float> h_pthr;
        const std::vector<int32_t>*s = &p->samples, *vc = &p->vc, *pc = &p->pass_cnt, *pl = &p->pass_lists;
        const std::vector<double>*mo = &p->models, *pt = &p->pass_tq;
        const std::vector<float>* ph = &p->pass_thr;
        size_t stride = m;
        if (p->device && H > 0) {
            HIP_TRY(p, hipSetDevice(p->dev));
            HIP_TRY(p, hipStreamSynchronize(p->stream));
            h_samples.resize(4 * H); h_vc.resize(2 * H); h_models.resize(12 * H);
            h_ptq.resize(7 * kMaxRefine); h_pthr.resize(kMaxRefine); h_pcnt.resize(kMaxRefine); h_plists.resize((size_t)kMaxRefine * p->cap);
            HIP_TRY(p, hipMemcpy(h_samples.data(), p->d_samples, 16 * H, hipMemcpyDeviceToHost));
            HIP_TRY(p, hipMemcpy(h_vc.data(), p->d_vc, 8 * H, hipMemcpyDeviceToHost));
            HIP_TRY(p, hipMemcpy(h_models.data(), p->d_models, 96 * H, hipMemcpyDeviceToHost));
            if (R > 0) {
                HIP_TRY(p, hipMemcpy(h_ptq.data(), p->d_pass_tq, 56 * R, hipMemcpyDeviceToHost));
                HIP_TRY(p, hipMemcpy(h_pthr.data(), p->d_pass_thr, 4 * R, hipMemcpyDeviceToHost));
                HIP_TRY(p, hipMemcpy(h_pcnt.data(), p->d_pass_cnt, 4 * R, hipMemcpyDeviceToHost));
                HIP_TRY(p, hipMemcpy(h_plists.data(), p->d_pass_lists, 4 * R * (size_t)p->cap, hipMemcpyDeviceToHost));
            }
            s = &h_samples; vc = &h_vc; pc = &h_pcnt; pl = &h_plists; mo = &h_models; pt = &h_ptq; ph = &h_pthr;
            stride = (size_t)p->cap;
        }
        for (size_t h = 0; h < H; ++h) {
            if (samples) for (int k = 0; k < 4; ++k) samples[4 * h + k] = (*s)[4 * h + k];
            if (valid) valid[h] = (*vc)[2 * h];
            if (counts) counts[h] = (*vc)[2 * h + 1];
            if (models) for (int k = 0; k < 12; ++k) models[12 * h + k] = (*mo)[12 * h + k];
        }
        for (size_t k = 0; k < R; ++k) {
            if (pass_tq) for (int i = 0; i < 7; ++i) pass_tq[7 * k + i] = (*pt)[7 * k + i];
            if (pass_threshold) pass_threshold[k] = (*ph)[k];
            if (pass_count) pass_count[k] = (*pc)[k];
            if (pass_inliers)
                for (size_t i = 0; i < m; ++i) pass_inliers[k * m + i] = i < (size_t)(*pc)[k] ? (*pl)[k * stride + i] : -1;
        }
        return (int)VISFS_BA_OK;
    });
}

}  // extern "C"
