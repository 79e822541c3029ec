// Sub-cell refinement of a scan's pose on a probability grid (include/visfs_scan_refine.h).
//
//   k_scan_refine   grid (m): one workgroup of kRefineLanes work items refines job blockIdx.x from start to end: every lane sums
//                   its returns' Jacobian rows and residuals at the pose asked for (bicubic on the uint16 cells, ten sums), the
//                   lanes' partials are added through LDS by the fixed tree, work item 0 steps the Levenberg-Marquardt control
//                   (ba_scan_refine.hpp: lm_advance) and leaves the next pose in LDS; the record and the trace are written at the
//                   end.  Nothing is read back during the loop and no workgroup waits for another.
// A single call is one upload (the job, the points), one launch, one download (the record) and one wait.  The one-core twin
// (host_refine) runs the lanes one after the other through the same functions.  The group call (ba_scan_group.hip) appends the
// launch to its match sequence.
#pragma clang fp contract(off)
#include "ba_scan_refine.hpp"
#include "ba_host.hpp"

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

using namespace scanrefine;
using namespace host;

namespace scanrefine {

__global__ __launch_bounds__(kRefineLanes) void k_scan_refine(const Job* __restrict__ jobs, Prm P, const double* __restrict__ pts,
                                                              visfs_scan_refine_result* __restrict__ out, double* __restrict__ trace) {
    __shared__ double s_p[kSums][kRefineLanes];
    __shared__ Lm s_m;
    const int t = threadIdx.x;
    const Job J = jobs[blockIdx.x];
    double* tr = trace + (int64_t)blockIdx.x * kMaxTrials * kTraceItems;
    if (t == 0) lm_start(J, P, s_m);
    __syncthreads();
    if (s_m.run) {
        const double c0 = s_m.c0, s0 = s_m.s0;
        for (;;) {
            double a[kSums];
            lane_sums(J, P, pts, c0, s0, s_m.ex, s_m.ey, s_m.ed, t, a);
#pragma unroll
            for (int k = 0; k < kSums; ++k) s_p[k][t] = a[k];
            for (int s = kRefineLanes / 2; s > 0; s >>= 1) {
                __syncthreads();
                if (t < s) {
#pragma unroll
                    for (int k = 0; k < kSums; ++k) s_p[k][t] += s_p[k][t + s];
                }
            }
            __syncthreads();
            if (t == 0) {
                double sums[kSums];
#pragma unroll
                for (int k = 0; k < kSums; ++k) sums[k] = s_p[k][0];
                lm_advance(s_m, P, sums, tr);
            }
            __syncthreads();
            if (s_m.done) break;
        }
    }
    if (t == 0) lm_result(s_m, out[blockIdx.x]);
}

int launch_refine(hipStream_t stream, int32_t m, const Job* d_jobs, const Prm& P, const double* d_pts, visfs_scan_refine_result* d_out, double* d_trace) {
    hipLaunchKernelGGL(k_scan_refine, dim3((unsigned)m), dim3(kRefineLanes), 0, stream, d_jobs, P, d_pts, d_out, d_trace);
    return (int)hipGetLastError();
}

void host_refine(const Job& J, const Prm& P, const double* pts, visfs_scan_refine_result* out, double* trace) {
    Lm m;
    if (lm_start(J, P, m)) {
        std::vector<double> p((size_t)kSums * kRefineLanes);
        while (!m.done) {
            for (int t = 0; t < kRefineLanes; ++t) {
                double a[kSums];
                lane_sums(J, P, pts, m.c0, m.s0, m.ex, m.ey, m.ed, t, a);
                for (int k = 0; k < kSums; ++k) p[(size_t)k * kRefineLanes + t] = a[k];
            }
            for (int s = kRefineLanes / 2; s > 0; s >>= 1)
                for (int t = 0; t < s; ++t)
                    for (int k = 0; k < kSums; ++k) p[(size_t)k * kRefineLanes + t] += p[(size_t)k * kRefineLanes + t + s];
            double sums[kSums];
            for (int k = 0; k < kSums; ++k) sums[k] = p[(size_t)k * kRefineLanes];
            lm_advance(m, P, sums, trace);
        }
    }
    lm_result(m, *out);
}

int check_call(const visfs_scan_refine_params& p, const double a[3], const double tg[2], int32_t n, const double* xyz, const char** why) {
    if (n > VISFS_SCAN_REFINE_MAX_POINTS) { *why = "more than 16384 points"; return VISFS_BA_ERR_UNSUPPORTED; }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(a[i])) { *why = "the initial pose is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    for (int i = 0; i < 2; ++i) if (!std::isfinite(tg[i])) { *why = "the target is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    for (int64_t i = 0; i < 3 * (int64_t)n; ++i) if (!std::isfinite(xyz[i])) { *why = "a point is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    const double w[4] = { p.occupied_space_weight, p.translation_weight, p.rotation_weight, p.function_tolerance };
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(w[i]) || w[i] < 0.0) { *why = "the weights and the tolerance must be finite and not negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p.max_iterations < 1 || p.max_iterations > VISFS_SCAN_REFINE_MAX_ITERATIONS) { *why = "max_iterations must lie in [1, 50]"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    return VISFS_BA_OK;
}

Prm make_prm(const visfs_scan_refine_params& p, int32_t n) {
    Prm P;
    P.s = n > 0 ? p.occupied_space_weight / std::sqrt((double)n) : 0.0;
    P.wt = p.translation_weight; P.wr = p.rotation_weight; P.ftol = p.function_tolerance;
    P.max_it = p.max_iterations; P.n = n;
    return P;
}

static void start_of(Job& J, const double a[3], const double tg[2]) {
    J.x0 = a[0]; J.y0 = a[1]; J.yaw0 = a[2]; J.c0 = std::cos(a[2]); J.s0 = std::sin(a[2]); J.tx = tg[0]; J.ty = tg[1];
}

Job stack_job(const visfs_scan_stack* st, const double a[3], const double tg[2]) {
    Job J;
    const scanfast::LevelView& v = st->lv.v[0];
    J.g.cells = v.p; J.g.nx = J.g.ax = st->L.nx; J.g.ny = J.g.ay = st->L.ny; J.g.gain = 1;
    J.res = st->L.res; J.max_x = st->L.max_x; J.max_y = st->L.max_y;
    start_of(J, a, tg);
    return J;
}

void not_refined(int32_t status, double x, double y, double yaw, visfs_scan_refine_result* out) {
    std::memset(out, 0, sizeof *out);
    out->status = status; out->x = x; out->y = y; out->yaw = yaw;
}

// the buffers of the single calls on one object
struct State {
    Staged<char> up;
    DeviceBuf<visfs_scan_refine_result> d_out; PinnedBuf<visfs_scan_refine_result> h_out;
    DeviceBuf<double> d_trace[2];                 // [0] of the call in work, [1] the hook's: they change hands after a call that ran to its end
    std::vector<double> trace;                    // host twin
    int32_t trials = 0;                           // of the last successful call
};

void state_free(State* s) { delete s; }

}  // namespace scanrefine

namespace {

constexpr size_t kTraceBytes = (size_t)kMaxTrials * kTraceItems * sizeof(double);

std::vector<double> points_xy(int32_t n, const double* xyz) {
    std::vector<double> p(2 * (size_t)n);
    for (int32_t i = 0; i < n; ++i) { p[2 * i] = xyz[3 * i]; p[2 * i + 1] = xyz[3 * i + 1]; }
    return p;
}

// One refinement on the grid of `J` (device memory when `device`), n > 0.
int run_single(State& st, bool device, int dev, hipStream_t stream, const Job& J, const Prm& P, const double* xyz, visfs_scan_refine_result* out,
               std::string& why) {
    const std::vector<double> pts = points_xy(P.n, xyz);
    if (!device) {
        std::vector<double> trace((size_t)kMaxTrials * kTraceItems, 0.0);
        host_refine(J, P, pts.data(), out, trace.data());
        st.trace.swap(trace);
        st.trials = out->trials;
        return VISFS_BA_OK;
    }
    HIP_TRY(&why, hipSetDevice(dev));
    const size_t bytes = sizeof(Job) + pts.size() * sizeof(double);
    RC_TRY(st.up.reserve(&why, bytes, bytes + bytes / 2));
    if (!st.d_out || !st.h_out) {
        RC_TRY(st.d_out.alloc(&why, 1));
        RC_TRY(st.h_out.alloc(&why, 1));
    }
    for (DeviceBuf<double>& t : st.d_trace) if (!t) RC_TRY(t.alloc(&why, (size_t)kMaxTrials * kTraceItems));
    std::memcpy(st.up.h.get(), &J, sizeof(Job));
    std::memcpy(st.up.h.get() + sizeof(Job), pts.data(), pts.size() * sizeof(double));
    HIP_TRY(&why, hipMemcpyAsync(st.up.d.get(), st.up.h.get(), bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(&why, (hipError_t)launch_refine(stream, 1, reinterpret_cast<const Job*>(st.up.d.get()), P, reinterpret_cast<const double*>(st.up.d.get() + sizeof(Job)), st.d_out.get(),
                                     st.d_trace[0].get()));
    HIP_TRY(&why, hipMemcpyAsync(st.h_out.get(), st.d_out.get(), sizeof(visfs_scan_refine_result), hipMemcpyDeviceToHost, stream));
    HIP_TRY(&why, hipStreamSynchronize(stream));
    *out = *st.h_out.get();
    std::swap(st.d_trace[0], st.d_trace[1]);
    st.trials = out->trials;
    return VISFS_BA_OK;
}

int download_trace(State* st, bool device, int dev, hipStream_t stream, int32_t cap, double* trace, int32_t* trials, std::string& why) {
    const int32_t n = st ? st->trials : 0;
    *trials = n;
    if (!trace || n == 0) return VISFS_BA_OK;
    if (cap < n) { why = "the hook's array is too small"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    const size_t bytes = (size_t)n * kTraceItems * sizeof(double);
    if (!device) { std::memcpy(trace, st->trace.data(), bytes); return VISFS_BA_OK; }
    HIP_TRY(&why, hipSetDevice(dev));
    HIP_TRY(&why, hipMemcpyAsync(trace, st->d_trace[1].get(), bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(&why, hipStreamSynchronize(stream));
    return VISFS_BA_OK;
}

void submaps_state_destroy(void* v) { state_free(static_cast<State*>(v)); }

State* state_of(visfs_submaps* s) {
    void** slot = visfs_internal_refine_slot(s, submaps_state_destroy);
    if (!*slot) *slot = new State();
    return static_cast<State*>(*slot);
}

State* state_of(visfs_scan_stack* st) {
    if (!st->refine) st->refine = new State();
    return st->refine;
}


}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_scan_refine_abi_version(void) { return VISFS_SCAN_REFINE_ABI_VERSION; }

void visfs_scan_refine_default_params(visfs_scan_refine_params* p) {
    if (!p) return;
    p->occupied_space_weight = 1.0; p->translation_weight = 10.0; p->rotation_weight = 40.0;
    p->function_tolerance = 1e-6; p->max_iterations = 20;
}

int visfs_scan_refine(visfs_submaps* s, int32_t index, const visfs_scan_refine_params* p, const double a[3], const double tg[2], int32_t n,
                      const double* xyz, visfs_scan_refine_result* out) {
    if (!s || !p || !a || !tg || !out || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        if (index < 0) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        const char* why = "";
        int rc = check_call(*p, a, tg, n, xyz, &why);
        if (rc != VISFS_BA_OK) return visfs_internal_scan_fail(s, rc, why);
        submap::ScanAccess acc;
        if ((rc = visfs_internal_scan_access(s, index, &acc)) != VISFS_BA_OK) return rc;
        if (acc.count > 0 && index >= acc.count) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        State* st = state_of(s);
        if (acc.count == 0 || n == 0) {                                    // no sub-map yet, or nothing to refine: the start back
            not_refined(VISFS_BA_OK, a[0], a[1], a[2], out);
            st->trials = 0;
            return (int)VISFS_BA_OK;
        }
        Job J;
        J.g.cells = acc.grid.cells; J.g.nx = acc.L.nx; J.g.ny = acc.L.ny; J.g.ax = acc.grid.nx; J.g.ay = acc.grid.ny; J.g.ox = acc.grid.ox; J.g.oy = acc.grid.oy;
        J.res = acc.L.res; J.max_x = acc.L.max_x; J.max_y = acc.L.max_y;
        start_of(J, a, tg);
        std::string text;
        rc = run_single(*st, acc.device, acc.dev, acc.stream, J, make_prm(*p, n), xyz, out, text);
        return rc == VISFS_BA_OK ? rc : visfs_internal_scan_fail(s, rc, text.c_str());
    });
}

int visfs_scan_stack_refine(visfs_scan_stack* st, const visfs_scan_refine_params* p, const double a[3], const double tg[2], int32_t n,
                            const double* xyz, visfs_scan_refine_result* out) {
    if (!st || !p || !a || !tg || !out || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(st, [&]() -> int {
        const char* why = "";
        int rc = check_call(*p, a, tg, n, xyz, &why);
        if (rc != VISFS_BA_OK) return fail(st, rc, why);
        State* rs = state_of(st);
        if (n == 0) { not_refined(VISFS_BA_OK, a[0], a[1], a[2], out); rs->trials = 0; return (int)VISFS_BA_OK; }
        std::string text;
        rc = run_single(*rs, st->device, st->dev, st->stream, stack_job(st, a, tg), make_prm(*p, n), xyz, out, text);
        return rc == VISFS_BA_OK ? rc : fail(st, rc, text);
    });
}

int visfs_scan_refine_download(visfs_submaps* s, int32_t cap, double* trace, int32_t* trials) {
    if (!s || !trials || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        submap::ScanAccess acc;
        int rc = visfs_internal_scan_access(s, -1, &acc);                  // the device and the stream
        if (rc != VISFS_BA_OK) return rc;
        std::string text;
        rc = download_trace(state_of(s), acc.device, acc.dev, acc.stream, cap, trace, trials, text);
        return rc == VISFS_BA_OK ? rc : visfs_internal_scan_fail(s, rc, text.c_str());
    });
}

int visfs_scan_stack_refine_download(visfs_scan_stack* st, int32_t cap, double* trace, int32_t* trials) {
    if (!st || !trials || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(st, [&]() -> int {
        std::string text;
        const int rc = download_trace(st->refine, st->device, st->dev, st->stream, cap, trace, trials, text);
        return rc == VISFS_BA_OK ? rc : fail(st, rc, text);
    });
}

}  // extern "C"
