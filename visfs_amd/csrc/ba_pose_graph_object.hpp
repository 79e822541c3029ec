// The object behind include/visfs_pose_graph.h and what its sources share: the two executors of posegraph::run (one workgroup on
// the device, a loop on one core), struct visfs_pose_graph, and the packing of a plan's upload and of the work arrays.
// ba_pose_graph.hip holds the optimisation and its hooks, ba_pose_graph_cov.hip the covariances (DESIGN.md sections 9p and 9q).
#pragma once
#pragma clang fp contract(off)
#include "ba_host.hpp"
#include "ba_pose_graph.hpp"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

namespace posegraph {

// one workgroup: the collective operations of `run`
struct DeviceExec {
    double* part;                             // LDS [kLanes]
    int32_t t;
    // The work item's index as a value the compiler cannot trace: the addresses formed from it are then computed where they are
    // used, not once for the whole kernel and kept in registers across every loop (which spilled to scratch).
    __device__ int32_t lane() const {
        int32_t l = t;
        asm volatile("" : "+v"(l));
        return l;
    }
    template <class F> __device__ void par(int32_t n, F f) {
#pragma nounroll
        for (int32_t i = lane(); i < n; i += kLanes) f(i);
        __syncthreads();
    }
    template <class F> __device__ double sum(int32_t n, F f) {
        double a = 0.0;
#pragma nounroll
        for (int32_t i = lane(); i < n; i += kLanes) a += f(i);
        part[t] = a;
        for (int32_t s = kLanes / 2; s > 0; s >>= 1) {
            __syncthreads();
            if (t < s) part[t] += part[t + s];
        }
        __syncthreads();
        const double r = part[0];
        __syncthreads();
        return r;
    }
    template <class F> __device__ double maxv(int32_t n, F f) {
        double a = -kRejectedCost;
        for (int32_t i = lane(); i < n; i += kLanes) { const double b = f(i); if (b > a) a = b; }
        part[t] = a;
        for (int32_t s = kLanes / 2; s > 0; s >>= 1) {
            __syncthreads();
            if (t < s && part[t + s] > part[t]) part[t] = part[t + s];
        }
        __syncthreads();
        const double r = part[0];
        __syncthreads();
        return r;
    }
    template <class F> __device__ void one(F f) {
        __syncthreads();
        if (t == 0) f();
        __syncthreads();
    }
};

// the same on one core
struct HostExec {
    std::vector<double> part = std::vector<double>((size_t)kLanes);
    template <class F> void par(int32_t n, F f) { for (int32_t i = 0; i < n; ++i) f(i); }
    template <class F> double sum(int32_t n, F f) {
        for (int32_t t = 0; t < kLanes; ++t) {
            double a = 0.0;
            for (int32_t i = t; i < n; i += kLanes) a += f(i);
            part[(size_t)t] = a;
        }
        for (int32_t s = kLanes / 2; s > 0; s >>= 1)
            for (int32_t t = 0; t < s; ++t) part[(size_t)t] += part[(size_t)(t + s)];
        return part[0];
    }
    template <class F> double maxv(int32_t n, F f) {
        double a = -kRejectedCost;
        for (int32_t i = 0; i < n; ++i) { const double b = f(i); if (b > a) a = b; }
        return a;
    }
    template <class F> void one(F f) { f(); }
};

struct CovObject;                             // ba_pose_graph_cov.hip: what the covariance calls of an object own
void cov_release(CovObject* c);

}  // namespace posegraph

struct visfs_pose_graph {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    int32_t maxN = 0, maxE = 0;
    std::string err;
    size_t up_bytes = 0, work_doubles = 0;
    host::PinnedBuf<char> h_up; host::DeviceBuf<char> d_up;          // the upload: pinned, device
    host::DeviceBuf<double> d_work; host::PinnedBuf<char> h_out;     // the work (its tail is the download), the pinned download
    std::vector<char> up;                             // twin
    std::vector<double> work;
    posegraph::View view;                             // of the last run
    int32_t trials = 0;
    host::Counts counts;
    posegraph::CovObject* cov = nullptr;              // made at the first covariance call

    visfs_pose_graph() = default;
    visfs_pose_graph(const visfs_pose_graph&) = delete;
    ~visfs_pose_graph() { posegraph::cov_release(cov); }
};

namespace posegraph {

inline size_t up_capacity(int32_t N, int32_t E) {
    return sizeof(double) * ((size_t)kPoseDoubles * N + (size_t)kEdgeDoubles * E + 3 * (size_t)N) +
           sizeof(int32_t) * (2 * (size_t)E + (size_t)N + 2 * ((size_t)N + 1) + 2 * (size_t)E + (size_t)E + 2);
}

constexpr size_t kResDoubles = (sizeof(visfs_pose_graph_result) + 7) / 8;

inline size_t out_doubles(int32_t N, int32_t E) { return kResDoubles + 3 * (size_t)N + (size_t)E; }

inline size_t work_capacity(int32_t N, int32_t E) {
    const size_t n = (size_t)N;
    return 6 * n + 34 * (size_t)E + 21 * n + 54 * n + 9 * n + 2 * (size_t)kMaxLevels * 9 * n + 21 * n + (size_t)kMaxTrials * kTraceItems + out_doubles(N, E);
}

// The upload of a plan packed at `dst` (host memory); the view's upload pointers set relative to `base` (where dst will lie).
inline size_t pack(const Plan& pl, const double* hook_r, char* dst, const char* base, View& v) {
    size_t off = 0;
    auto put = [&](const void* src, size_t bytes) -> const char* {
        if (src && bytes) std::memcpy(dst + off, src, bytes); else if (bytes) std::memset(dst + off, 0, bytes);
        const char* at = base + off;
        off += (bytes + 7) & ~(size_t)7;
        return at;
    };
    v.N = pl.N; v.E = pl.E; v.n = pl.n;
    v.pose0 = reinterpret_cast<const double*>(put(pl.pose0.data(), pl.pose0.size() * sizeof(double)));
    v.ed = reinterpret_cast<const double*>(put(pl.ed.data(), pl.ed.size() * sizeof(double)));
    v.hook_r = reinterpret_cast<const double*>(put(hook_r, 3 * (size_t)pl.n * sizeof(double)));
    v.eij = reinterpret_cast<const int32_t*>(put(pl.eij.data(), pl.eij.size() * sizeof(int32_t)));
    v.row_of = reinterpret_cast<const int32_t*>(put(pl.row_of.data(), pl.row_of.size() * sizeof(int32_t)));
    v.inc_ptr = reinterpret_cast<const int32_t*>(put(pl.inc_ptr.data(), pl.inc_ptr.size() * sizeof(int32_t)));
    v.inc = reinterpret_cast<const int32_t*>(put(pl.inc.data(), pl.inc.size() * sizeof(int32_t)));
    v.chain_ptr = reinterpret_cast<const int32_t*>(put(pl.chain_ptr.data(), pl.chain_ptr.size() * sizeof(int32_t)));
    v.chain = reinterpret_cast<const int32_t*>(put(pl.chain.data(), pl.chain.size() * sizeof(int32_t)));
    return off;
}

// the work arrays of a view carved from `w`; returns where the download starts
inline double* carve(View& v, double* w) {
    const size_t N = (size_t)v.N, E = (size_t)v.E, n = (size_t)v.n;
    auto take = [&](size_t count) { double* p = w; w += count; return p; };
    v.x = take(3 * N); v.xt = take(3 * N);
    v.eb = take(27 * E); v.eg = take(6 * E); v.chi2 = take(E);
    v.g = take(3 * n); v.D = take(9 * n); v.C = take(9 * n);
    for (int k = 0; k < 2; ++k) { v.pD[k] = take(9 * n); v.pA[k] = take(9 * n); v.pC[k] = take(9 * n); }
    v.Dinv = take(9 * n);
    v.al = take((size_t)kMaxLevels * 9 * n); v.ga = take((size_t)kMaxLevels * 9 * n);
    v.r = take(3 * n); v.z = take(3 * n); v.p = take(3 * n); v.q = take(3 * n); v.dx = take(3 * n);
    v.t[0] = take(3 * n); v.t[1] = take(3 * n);
    v.trace = take((size_t)kMaxTrials * kTraceItems);
    double* out = w;
    v.res = reinterpret_cast<visfs_pose_graph_result*>(take(kResDoubles));
    v.out_poses = take(3 * N); v.out_chi2 = take(E);
    return out;
}

}  // namespace posegraph
