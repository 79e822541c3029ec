// ba_fund.hip — the fundamental-matrix cull (include/visfs_fund.h): two kernels and the two flavours of the object.
//
//   k_fund_ransac  one wavefront per hypothesis, four per workgroup.  The workgroup stages the rows in LDS once; every lane of a
//                  wavefront draws the same sample and runs the same seven-point solve (uniform, as the P3P of k_pnp_ransac), then
//                  the lanes take rows strided and score the up to three models of the hypothesis in one pass; __ballot + popcount
//                  give the counts.  One 64-bit atomicMax of (count << 32) | (0xFFFFFFFF - (3 h + k)) per model with seven inliers
//                  picks the winner, lowest h and then lowest k on a tie, whatever the arrival order.
//   k_fund_mask    the winner's model over the rows again: the mask, the ANDed status, and the result block.
//
// A call is one copy in (a header with the zeroed winner key and the two Hartley transforms, the kept rows at 16 B, their status
// bytes), the two launches and one copy out (the result block, the mask, the status).  The transforms are computed on the host in
// both flavours.  The arithmetic is ba_fund.hpp.
//
// The resident tracker (include/visfs_tracker.h) runs the same search on rows that never leave the device:
// k_fund_ransac_g and k_fund_mask_g read their member's CullRec at blockIdx.z and m from device memory (fund::group_cull), and the
// host twin of that tracker goes through fund::cull_host.
#include "ba_fund.hpp"
#include "ba_group.hpp"      // fund::group_cull, fund::cull_host
#include "ba_host.hpp"
#include "../../include/visfs_fund.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

// Internal entry points of ba_api.cpp (the handle's device and stream).
hipStream_t visfs_internal_stream(visfs_ba_handle* h);
int visfs_internal_device(visfs_ba_handle* h);
void visfs_internal_set_error(visfs_ba_handle* h, const char* msg);

using namespace fund;
using namespace host;

namespace fund {

constexpr int FD_T = 256;
constexpr size_t kHeaderBytes = 256;
static_assert(sizeof(Header) <= kHeaderBytes && sizeof(Result) <= kHeaderBytes, "header and result block are one header each");
static_assert(sizeof(Row) == 16, "a row is 16 B");

struct RansacArgs {
    const Header* head;
    const Row* rows;
    int32_t m, iterations;
    uint64_t seed;
    float thr2;
    int32_t* samples;      // [iterations][7]
    int32_t* nc;           // [iterations][4]: n_models, counts[3]
    double* models;        // [iterations][3][9]
    unsigned long long* key;
};

struct DevicePolicy {
    const RansacArgs& A;
    const Row* rows;       // LDS
    int lane;

    __device__ Row row(int i) const { return rows[i]; }
    __device__ void count(const double F[3][9], int n, int32_t counts[3]) const {
        counts[0] = counts[1] = counts[2] = 0;
        if (n == 0) return;
        for (int base = 0; base < A.m; base += 64) {
            const int i = base + lane;
            const bool live = i < A.m;
            const Row r = rows[live ? i : 0];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k < n) counts[k] += __popcll(__ballot(live && inlier(F[k], r, A.thr2)));
            }
        }
    }
    __device__ void record(int32_t h, const int32_t s[7], int n, const double Fh[3][9], const int32_t counts[3]) const {
        if (lane != 0) return;
#pragma unroll
        for (int k = 0; k < 7; ++k) A.samples[7 * (size_t)h + k] = s[k];
        A.nc[4 * (size_t)h] = n;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            A.nc[4 * (size_t)h + 1 + k] = counts[k];
#pragma unroll
            for (int i = 0; i < 9; ++i) A.models[27 * (size_t)h + 9 * k + i] = Fh[k][i];
            if (k < n && counts[k] >= kMinRows) atomicMax(A.key, winner_key(counts[k], h, k));
        }
    }
};

// One body for the by-value kernel of the staged call and the record-reading kernel of the resident tracker.
__device__ __forceinline__ void fund_ransac_body(const RansacArgs& A) {
    __shared__ Row s_rows[kMaxPoints];
    {
        const float4* src = reinterpret_cast<const float4*>(A.rows);
        float4* dst = reinterpret_cast<float4*>(s_rows);
        for (int i = threadIdx.x; i < A.m; i += FD_T) dst[i] = src[i];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    const int h = blockIdx.x * (FD_T / 64) + wave;
    if (h >= A.iterations) return;
    Call c;
    c.T1 = A.head->T1; c.T2 = A.head->T2; c.m = A.m; c.iterations = A.iterations; c.seed = A.seed; c.thr2 = A.thr2;
    DevicePolicy pol{ A, s_rows, (int)(threadIdx.x & 63) };
    // seven_rows: the models of the rows 0 .. 6 as hypothesis 0, unscored; every row is an inlier.  Only k_fund_ransac_g gets here:
    // visfs_fund_cull handles seven rows on the host and never launches the by-value kernel with them.
    if (A.m == kMinRows) {
        const int32_t s[7] = { 0, 1, 2, 3, 4, 5, 6 };
        double Fh[3][9];
        const int n = solve_sample(pol, c, s, Fh);
        const int32_t counts[3] = { 0, 0, 0 };
        pol.record(h, s, n, Fh, counts);
        if (pol.lane == 0) *A.key = n > 0 ? winner_key(kMinRows, 0, 0) : 0ull;
        return;
    }
    hypothesis(pol, c, h);
}

__global__ __launch_bounds__(FD_T) void k_fund_ransac(RansacArgs A) { fund_ransac_body(A); }

// Member blockIdx.z of a tracker call: m comes from device memory.  Fewer than seven rows: nothing runs.  Seven: hypothesis 0 alone.
__global__ __launch_bounds__(FD_T) void k_fund_ransac_g(const CullRec* __restrict__ recs, CullShape S) {
    const CullRec* r = recs + blockIdx.z;
    if (r->skip) return;
    const int32_t m = min(*r->m, kMaxPoints);
    if (m < kMinRows) return;
    RansacArgs A;                              // the record's fields once, into scalars, in front of the body
    Header* const head = r->head;
    A.head = head; A.rows = r->rows; A.m = m; A.iterations = m == kMinRows ? 1 : S.iterations; A.seed = S.seed; A.thr2 = S.thr2;
    A.samples = r->samples; A.nc = r->nc; A.models = r->models; A.key = &head->key;
    if ((int)blockIdx.x * (FD_T / 64) >= A.iterations) return;
    fund_ransac_body(A);
}

struct MaskArgs {
    const Header* head;
    const Row* rows;
    const uint8_t* status_in;  // [m]
    int32_t m;
    float thr2;
    const double* models;
    Result* res;
    uint8_t* mask;             // [m]
    uint8_t* status;           // [m]
};

__global__ __launch_bounds__(FD_T) void k_fund_mask(MaskArgs A) {
    Call c;
    c.T1 = A.head->T1; c.T2 = A.head->T2; c.m = A.m; c.iterations = 0; c.seed = 0; c.thr2 = A.thr2;
    const unsigned long long key = A.head->key;
    const Result res = winner_of(key, A.models, c);
    const int i = blockIdx.x * FD_T + threadIdx.x;
    if (i < A.m) {
        const bool in = key != 0 && inlier(res.F, A.rows[i], A.thr2);
        A.mask[i] = in ? 1 : 0;
        A.status[i] = (in && A.status_in[i] != 0) ? 1 : 0;
    }
    if (i == 0) *A.res = res;
}

// The winner's mask of member blockIdx.z over the rows that entered, scattered to their from-rows, and the status after the AND
// (the rows kernel has written both for the rows that did not enter).
__global__ __launch_bounds__(FD_T) void k_fund_mask_g(const CullRec* __restrict__ recs, CullShape S) {
    const CullRec& r = recs[blockIdx.z];
    if (r.skip) return;
    const int32_t m = min(*r.m, kMaxPoints);
    if (m < kMinRows) return;
    const int k = blockIdx.x * FD_T + threadIdx.x;
    if (k >= m) return;
    Call c;
    c.T1 = r.head->T1; c.T2 = r.head->T2; c.m = m; c.iterations = 0; c.seed = 0; c.thr2 = S.thr2;
    const unsigned long long key = r.head->key;
    Result res = winner_of(key, r.models, c);
    const bool seven = m == kMinRows;
    if (seven) res.count = kMinRows;
    const bool in = seven || (key != 0 && inlier(res.F, r.rows[k], S.thr2));
    const int32_t i = r.keep[k];
    r.mask[i] = in ? 1 : 0;
    r.status[i] = (in && r.st[k] != 0) ? 1 : 0;
    if (k == 0) *r.res = res;
}

int group_cull(hipStream_t stream, int n, const CullRec* d_recs, int32_t max_rows, const CullShape& S, flow::GroupCounts* cnt) {
    hipLaunchKernelGGL(k_fund_ransac_g, dim3((unsigned)((S.iterations + FD_T / 64 - 1) / (FD_T / 64)), 1, (unsigned)n), dim3(FD_T), 0, stream,
                       d_recs, S);
    if (hipGetLastError() != hipSuccess) return VISFS_BA_ERR_DEVICE;
    ++cnt->launches;
    hipLaunchKernelGGL(k_fund_mask_g, dim3((unsigned)((max_rows + FD_T - 1) / FD_T), 1, (unsigned)n), dim3(FD_T), 0, stream, d_recs, S);
    if (hipGetLastError() != hipSuccess) return VISFS_BA_ERR_DEVICE;
    ++cnt->launches;
    return VISFS_BA_OK;
}

}  // namespace fund

// ====================================================================== the object
struct visfs_fund {
    int32_t cap = 0;
    std::string err;
    bool device = false;
    bool called = false;
    bool state_on_host = true;     // where visfs_fund_download finds the hypotheses of the last call
    int32_t last_m = 0, last_hyp = 0;
    Result res{};
    Hartley T1{}, T2{};
    bool have_T = false;

    std::vector<Row> rows;
    std::vector<int32_t> keep;     // input row numbers of the kept rows
    std::vector<uint8_t> st, mask_k, status_k;
    // host twin (and the seven-row call of both flavours): what visfs_fund_download reads
    std::vector<int32_t> samples, nc;
    std::vector<double> models;

    // device
    visfs_ba_handle* ba = nullptr;
    int dev = 0;
    hipStream_t stream = nullptr;
    PinnedBuf<char> h_in;      // pinned: header + rows + status
    PinnedBuf<char> h_out;     // pinned: Result + mask + status
    DeviceBuf<char> d_in;
    DeviceBuf<char> d_out;
    DeviceBuf<char> d_state;   // hypotheses
    int32_t *d_samples = nullptr, *d_nc = nullptr;
    double* d_models = nullptr;

    ~visfs_fund() {                     // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

int device_init(visfs_fund* p) {
    HIP_TRY(p, hipSetDevice(p->dev));
    const size_t cap = (size_t)p->cap;
    const size_t in_bytes = kHeaderBytes + up256(17 * cap), out_bytes = kHeaderBytes + up256(2 * cap);
    RC_TRY(p->h_in.alloc(p, in_bytes));
    RC_TRY(p->h_out.alloc(p, out_bytes));
    RC_TRY(p->d_in.alloc(p, in_bytes));
    RC_TRY(p->d_out.alloc(p, out_bytes));
    const size_t H = kMaxHypotheses;
    const size_t o_models = 0, o_samples = o_models + up256(216 * H), o_nc = o_samples + up256(28 * H), bytes = o_nc + up256(16 * H);
    RC_TRY(p->d_state.alloc(p, bytes));
    p->d_models = reinterpret_cast<double*>(p->d_state.get() + o_models);
    p->d_samples = reinterpret_cast<int32_t*>(p->d_state.get() + o_samples);
    p->d_nc = reinterpret_cast<int32_t*>(p->d_state.get() + o_nc);
    return VISFS_BA_OK;
}

// The host twin's side of fund::hypothesis: the same functions over the rows in sequence.
struct HostPolicy {
    int32_t* samples; int32_t* nc; double* models;     // per hypothesis
    const Row* rows;
    int32_t m;
    float thr2;
    unsigned long long key = 0;

    Row row(int i) const { return rows[i]; }
    void count(const double F[3][9], int n, int32_t counts[3]) const {
        counts[0] = counts[1] = counts[2] = 0;
        for (int k = 0; k < n; ++k)
            for (int i = 0; i < m; ++i) counts[k] += inlier(F[k], rows[i], thr2) ? 1 : 0;
    }
    void record(int32_t h, const int32_t s[7], int n, const double Fh[3][9], const int32_t counts[3]) {
        for (int k = 0; k < 7; ++k) samples[7 * (size_t)h + k] = s[k];
        nc[4 * (size_t)h] = n;
        for (int k = 0; k < 3; ++k) {
            nc[4 * (size_t)h + 1 + k] = counts[k];
            for (int i = 0; i < 9; ++i) models[27 * (size_t)h + 9 * k + i] = Fh[k][i];
            if (k < n && counts[k] >= kMinRows) key = std::max(key, winner_key(counts[k], h, k));
        }
    }
};

void host_state(visfs_fund* p, int H) {
    p->samples.assign(7 * (size_t)H, 0); p->nc.assign(4 * (size_t)H, 0); p->models.assign(27 * (size_t)H, 0.0);
    p->state_on_host = true;
}

// m == 7 (both flavours): the models of the rows 0 .. 6, recorded as the one hypothesis of the call; every kept row is an inlier.
// mask and status are per row that entered.
Result seven_rows_core(HostPolicy pol, const Call& c, const uint8_t* st, uint8_t* mask, uint8_t* status) {
    const int32_t s[7] = { 0, 1, 2, 3, 4, 5, 6 };
    double Fh[3][9];
    const int n = solve_sample(pol, c, s, Fh);
    const int32_t counts[3] = { 0, 0, 0 };
    pol.record(0, s, n, Fh, counts);
    Result res = winner_of(n > 0 ? winner_key(kMinRows, 0, 0) : 0ull, pol.models, c);
    res.count = kMinRows;
    for (int i = 0; i < c.m; ++i) { mask[i] = 1; status[i] = st[i] ? 1 : 0; }
    return res;
}

Result host_cull_core(HostPolicy pol, const Call& c, const uint8_t* st, uint8_t* mask, uint8_t* status) {
    for (int h = 0; h < c.iterations; ++h) hypothesis(pol, c, h);
    const Result res = winner_of(pol.key, pol.models, c);
    for (int i = 0; i < c.m; ++i) {
        const bool in = pol.key != 0 && inlier(res.F, pol.rows[i], c.thr2);
        mask[i] = in ? 1 : 0;
        status[i] = (in && st[i] != 0) ? 1 : 0;
    }
    return res;
}

void seven_rows(visfs_fund* p, const Call& c) {
    host_state(p, 1);
    p->res = seven_rows_core(HostPolicy{ p->samples.data(), p->nc.data(), p->models.data(), p->rows.data(), c.m, c.thr2 }, c, p->st.data(),
                             p->mask_k.data(), p->status_k.data());
}

void host_cull(visfs_fund* p, const Call& c) {
    host_state(p, c.iterations);
    p->res = host_cull_core(HostPolicy{ p->samples.data(), p->nc.data(), p->models.data(), p->rows.data(), c.m, c.thr2 }, c, p->st.data(),
                            p->mask_k.data(), p->status_k.data());
}

int device_cull(visfs_fund* p, const Call& c) {
    const size_t m = (size_t)c.m;
    Header hd{};
    hd.T1 = c.T1; hd.T2 = c.T2;
    std::memset(p->h_in.get(), 0, kHeaderBytes);
    std::memcpy(p->h_in.get(), &hd, sizeof hd);
    std::memcpy(p->h_in.get() + kHeaderBytes, p->rows.data(), sizeof(Row) * m);
    std::memcpy(p->h_in.get() + kHeaderBytes + sizeof(Row) * m, p->st.data(), m);
    HIP_TRY(p, hipMemcpyAsync(p->d_in.get(), p->h_in.get(), kHeaderBytes + 17 * m, hipMemcpyHostToDevice, p->stream));
    RansacArgs A;
    A.head = reinterpret_cast<const Header*>(p->d_in.get()); A.rows = reinterpret_cast<const Row*>(p->d_in.get() + kHeaderBytes);
    A.m = c.m; A.iterations = c.iterations; A.seed = c.seed; A.thr2 = c.thr2;
    A.samples = p->d_samples; A.nc = p->d_nc; A.models = p->d_models; A.key = reinterpret_cast<unsigned long long*>(p->d_in.get());
    hipLaunchKernelGGL(k_fund_ransac, dim3((unsigned)((c.iterations + FD_T / 64 - 1) / (FD_T / 64))), dim3(FD_T), 0, p->stream, A);
    HIP_TRY(p, hipGetLastError());
    MaskArgs B;
    B.head = A.head; B.rows = A.rows; B.status_in = reinterpret_cast<const uint8_t*>(p->d_in.get() + kHeaderBytes + sizeof(Row) * m);
    B.m = c.m; B.thr2 = c.thr2; B.models = p->d_models; B.res = reinterpret_cast<Result*>(p->d_out.get());
    B.mask = reinterpret_cast<uint8_t*>(p->d_out.get() + kHeaderBytes); B.status = B.mask + m;
    hipLaunchKernelGGL(k_fund_mask, dim3((unsigned)((c.m + FD_T - 1) / FD_T)), dim3(FD_T), 0, p->stream, B);
    HIP_TRY(p, hipGetLastError());
    HIP_TRY(p, hipMemcpyAsync(p->h_out.get(), p->d_out.get(), kHeaderBytes + 2 * m, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::memcpy(&p->res, p->h_out.get(), sizeof(Result));
    if (p->res.count < 0 || p->res.count > c.m) return fail(p, VISFS_BA_ERR_DEVICE, "the device returned an impossible inlier count");
    std::memcpy(p->mask_k.data(), p->h_out.get() + kHeaderBytes, m);
    std::memcpy(p->status_k.data(), p->h_out.get() + kHeaderBytes + m, m);
    p->state_on_host = false;
    return VISFS_BA_OK;
}

}  // namespace

// The cull of a host-twin tracker on its from-rows: the steps of visfs_fund_cull in sequence, into the arrays of `r`.
void fund::cull_host(const CullRec& r, const float* from_xy, const float* to_xy, const uint8_t* lk_st, int32_t n_from, const CullShape& S) {
    int32_t m = 0;
    for (int32_t i = 0; i < n_from; ++i) {
        const float* a = from_xy + 2 * (size_t)i;
        const float* b = to_xy + 2 * (size_t)i;
        if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(b[0]) && std::isfinite(b[1]))) continue;
        r.rows[m] = Row{ a[0], a[1], b[0], b[1] };
        r.keep[m] = i;
        r.st[m] = lk_st[i] ? 1 : 0;
        ++m;
    }
    *r.m = m;
    for (int32_t i = 0; i < n_from; ++i) { r.mask[i] = 0; r.status[i] = (m < kMinRows && lk_st[i]) ? 1 : 0; }
    if (m < kMinRows) return;
    Call c;
    std::vector<double> term((size_t)m);
    c.T1 = hartley(r.rows, m, false, term.data()); c.T2 = hartley(r.rows, m, true, term.data());
    c.m = m; c.iterations = S.iterations; c.seed = S.seed; c.thr2 = S.thr2;
    *r.head = Header{ 0ull, 0ull, c.T1, c.T2 };
    std::vector<uint8_t> mask_k((size_t)m), status_k((size_t)m);
    const HostPolicy pol{ r.samples, r.nc, r.models, r.rows, m, c.thr2 };
    *r.res = m == kMinRows ? seven_rows_core(pol, c, r.st, mask_k.data(), status_k.data())
                           : host_cull_core(pol, c, r.st, mask_k.data(), status_k.data());
    for (int32_t k = 0; k < m; ++k) { r.mask[r.keep[k]] = mask_k[(size_t)k]; r.status[r.keep[k]] = status_k[(size_t)k]; }
}

// ====================================================================== exported C ABI
extern "C" {

int visfs_fund_abi_version(void) { return VISFS_FUND_ABI_VERSION; }

void visfs_fund_default_params(visfs_fund_params* p) {
    if (!p) return;
    p->pixel_error = 1.0f; p->iterations = 1000; p->seed = 0;
}

int visfs_fund_create_host(int32_t capacity_points, visfs_fund** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (capacity_points < 1) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (capacity_points > kMaxPoints) return VISFS_BA_ERR_UNSUPPORTED;
    return guarded(nullptr, [&]() -> int {
        visfs_fund* p = new visfs_fund();
        p->cap = capacity_points;
        *out = p;
        return (int)VISFS_BA_OK;
    });
}

int visfs_fund_create(visfs_ba_handle* h, int32_t capacity_points, visfs_fund** out) {
    if (!h || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (capacity_points < 1) { visfs_internal_set_error(h, "capacity_points must be at least 1"); return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (capacity_points > kMaxPoints) { visfs_internal_set_error(h, "capacity_points above 4096"); return VISFS_BA_ERR_UNSUPPORTED; }
    return guarded(nullptr, [&]() -> int {
        visfs_fund* p = new visfs_fund();
        p->cap = capacity_points;
        p->device = true; p->ba = h; p->dev = visfs_internal_device(h); p->stream = visfs_internal_stream(h);
        const int rc = device_init(p);
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, p->err.c_str()); delete p; return rc; }
        *out = p;
        return (int)VISFS_BA_OK;
    });
}

void visfs_fund_destroy(visfs_fund* p) {
    if (!p) return;
    delete p;
}

const char* visfs_fund_last_error(const visfs_fund* p) { return p ? p->err.c_str() : "null cull"; }

int visfs_fund_cull(visfs_fund* p, const visfs_fund_params* params, int32_t n, const float* from_xy, const float* to_xy,
                    const uint8_t* status_in, uint8_t* status_out, uint8_t* mask_out, double* F_out, int32_t* n_inliers,
                    int32_t* applied) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!params || !n_inliers || !applied || n < 0 || (n > 0 && (!from_xy || !to_xy || !status_in || !status_out || !mask_out)))
        return fail(p, VISFS_BA_ERR_BAD_ARGUMENT, "a required pointer is null or n is negative");
    return guarded(p, [&]() -> int {
        if (!std::isfinite(params->pixel_error)) return fail(p, VISFS_BA_ERR_BAD_ARGUMENT, "pixel_error is not finite");
        if (params->iterations < 1) return fail(p, VISFS_BA_ERR_BAD_ARGUMENT, "iterations must be at least 1");
        if (params->iterations > kMaxHypotheses) return fail(p, VISFS_BA_ERR_UNSUPPORTED, "iterations above 4096");
        if (n > p->cap) return fail(p, VISFS_BA_ERR_BAD_ARGUMENT, "n is above the capacity of the cull");
        if (p->device) {
            HIP_TRY(p, hipSetDevice(p->dev));
            HIP_TRY(p, hipStreamSynchronize(p->stream));            // (the pinned blocks are free again)
        }
        // step 1: the rows
        p->rows.clear(); p->keep.clear(); p->st.clear();
        for (int32_t i = 0; i < n; ++i) {
            const float* a = from_xy + 2 * (size_t)i;
            const float* b = to_xy + 2 * (size_t)i;
            if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(b[0]) && std::isfinite(b[1]))) continue;
            p->rows.push_back(Row{ a[0], a[1], b[0], b[1] });
            p->keep.push_back(i);
            p->st.push_back(status_in[i] ? 1 : 0);
        }
        const int32_t m = (int32_t)p->rows.size();
        p->called = true; p->last_m = m; p->last_hyp = 0; p->have_T = false; p->state_on_host = true;
        p->res = Result{}; p->res.winner_h = p->res.winner_k = -1;
        *n_inliers = 0; *applied = 0;
        if (F_out) for (int i = 0; i < 9; ++i) F_out[i] = 0.0;
        if (m < kMinRows) {
            for (int32_t i = 0; i < n; ++i) { status_out[i] = status_in[i] ? 1 : 0; mask_out[i] = 0; }
            return (int)VISFS_BA_OK;
        }
        // step 2: the conditioning
        Call c;
        std::vector<double> term((size_t)m);
        c.T1 = hartley(p->rows.data(), m, false, term.data()); c.T2 = hartley(p->rows.data(), m, true, term.data());
        c.m = m; c.iterations = params->iterations; c.seed = params->seed;
        c.thr2 = cull_thr2(params->pixel_error);
        p->T1 = c.T1; p->T2 = c.T2; p->have_T = true;
        p->mask_k.assign((size_t)m, 0); p->status_k.assign((size_t)m, 0);
        if (m == kMinRows) {
            seven_rows(p, c);
            p->last_hyp = 1;
        } else {
            if (p->device) {
                const int rc = device_cull(p, c);
                if (rc != VISFS_BA_OK) { p->called = false; return rc; }
            } else {
                host_cull(p, c);
            }
            p->last_hyp = c.iterations;
        }
        for (int32_t i = 0; i < n; ++i) { status_out[i] = 0; mask_out[i] = 0; }
        int32_t inl = 0;
        for (int32_t k = 0; k < m; ++k) {
            mask_out[p->keep[k]] = p->mask_k[k];
            status_out[p->keep[k]] = p->status_k[k];
            inl += p->mask_k[k];
        }
        *n_inliers = inl; *applied = 1;
        if (F_out) for (int i = 0; i < 9; ++i) F_out[i] = p->res.F[i];
        return (int)VISFS_BA_OK;
    });
}

int visfs_fund_last_sizes(const visfs_fund* p, int32_t* m, int32_t* n_hypotheses) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!p->called) return VISFS_BA_ERR_NOT_LOADED;
    if (m) *m = p->last_m;
    if (n_hypotheses) *n_hypotheses = p->last_hyp;
    return VISFS_BA_OK;
}

int visfs_fund_download(visfs_fund* p, int32_t* samples, int32_t* n_models, double* models, int32_t* counts, int32_t* winner_h,
                        int32_t* winner_k, double* T1, double* T2) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!p->called) return fail(p, VISFS_BA_ERR_NOT_LOADED, "no visfs_fund_cull call yet");
    return guarded(p, [&]() -> int {
        const size_t H = (size_t)p->last_hyp;
        if (winner_h) *winner_h = p->res.winner_h;
        if (winner_k) *winner_k = p->res.winner_k;
        for (int i = 0; i < 9; ++i) { if (T1) T1[i] = 0.0; if (T2) T2[i] = 0.0; }
        if (p->have_T) { if (T1) hartley_matrix(p->T1, T1); if (T2) hartley_matrix(p->T2, T2); }
        std::vector<int32_t> h_samples, h_nc;
        std::vector<double> h_models;
        const std::vector<int32_t>*s = &p->samples, *nc = &p->nc;
        const std::vector<double>* mo = &p->models;
        if (!p->state_on_host && H > 0) {
            HIP_TRY(p, hipSetDevice(p->dev));
            HIP_TRY(p, hipStreamSynchronize(p->stream));
            h_samples.resize(7 * H); h_nc.resize(4 * H); h_models.resize(27 * H);
            HIP_TRY(p, hipMemcpy(h_samples.data(), p->d_samples, 28 * H, hipMemcpyDeviceToHost));
            HIP_TRY(p, hipMemcpy(h_nc.data(), p->d_nc, 16 * H, hipMemcpyDeviceToHost));
            HIP_TRY(p, hipMemcpy(h_models.data(), p->d_models, 216 * H, hipMemcpyDeviceToHost));
            s = &h_samples; nc = &h_nc; mo = &h_models;
        }
        for (size_t h = 0; h < H; ++h) {
            if (samples) for (int k = 0; k < 7; ++k) samples[7 * h + k] = (*s)[7 * h + k];
            if (n_models) n_models[h] = (*nc)[4 * h];
            if (counts) for (int k = 0; k < 3; ++k) counts[3 * h + k] = (*nc)[4 * h + 1 + k];
            if (models) for (int k = 0; k < 27; ++k) models[27 * h + k] = (*mo)[27 * h + k];
        }
        return (int)VISFS_BA_OK;
    });
}

}  // extern "C"
