// Marginal and relative covariances of the 2-D pose graph (include/visfs_pose_graph_cov.h).
//
//   k_pose_graph_cov_setup    grid (1) x kLanes: posegraph::cov_setup: the linearisation at the poses handed in, the cyclic-reduction
//                             set-up at lambda = 0, the head (status, levels, cost) to device memory.
//   k_pose_graph_cov_solve    grid (3 sources) x kLanes: workgroup c leaves at once when the set-up failed, else runs the conjugate
//                             gradients of column c on its own slice of the arena and writes its iteration count and flag.  The
//                             coefficients (edge blocks, D, C, the reduction's levels, Dinv) are shared and only read.  No workgroup
//                             waits for another; each depends on launch 1 alone, through the order of the stream.
//   k_pose_graph_cov_gather   one work item per query: posegraph::cov_query on the columns' solutions.
// A call is one upload (the plan, the sources and the queries), three launches, one download (head, flags, joint, relative) and one
// wait.  The one-core twin runs the same three stages with one column's workspace and the stored solutions.
// The buffers of these calls are the object's CovObject, made at the first covariance call: visfs_pose_graph_optimize and its hooks
// touch none of it, and a covariance call touches neither their work arrays nor their view.
#pragma clang fp contract(off)
#include "ba_pose_graph_object.hpp"
#include "ba_pose_graph_cov.hpp"
#include "ba_host.hpp"

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace posegraph;
using namespace host;

namespace posegraph {

constexpr int kGatherLanes = 64;

struct CovObject {
    // device
    size_t up_bytes = 0, fixed_doubles = 0;
    PinnedBuf<char> h_up; DeviceBuf<char> d_up;
    DeviceBuf<double> d_work;                         // the work arrays of the View, then head, flags, joint, relative
    DeviceBuf<double> d_arena;
    PinnedBuf<char> h_out;
    // twin
    std::vector<char> up;
    std::vector<double> work, column, solutions;
    // the last successful call
    bool valid = false;
    int32_t n = 0, sources = 0;
    const double* sol = nullptr;
    int64_t sol_stride = 0;
    std::vector<int32_t> flags;
    Counts counts;
};

void cov_release(CovObject* c) {
    delete c;
}

__global__ __launch_bounds__(kLanes) void k_pose_graph_cov_setup(View v, CovView q, int32_t precond) {
    __shared__ double s_part[kLanes];
    __shared__ State s_state;
    DeviceExec x{ s_part, (int32_t)threadIdx.x };
    cov_setup(x, v, precond, s_state, q.head);
}

__global__ __launch_bounds__(kLanes) void k_pose_graph_cov_solve(View v, CovView q, Prm P) {
    __shared__ double s_part[kLanes];
    __shared__ State s_state;
    __shared__ alignas(View) unsigned char s_col_bytes[sizeof(View)];         // View has member initialisers, LDS takes none
    View& s_col = *reinterpret_cast<View*>(s_col_bytes);
    if (q.head->status != VISFS_BA_OK) return;                               // the same word for every work item: all leave
    const int32_t c = (int32_t)blockIdx.x;
    if (c >= 3 * q.sources) return;
    DeviceExec x{ s_part, (int32_t)threadIdx.x };
    // The column's view lies in LDS: a private copy cannot be split into registers (the ping-pong buffers are indexed at run time)
    // and would go to scratch.
    static_assert(sizeof(View) % sizeof(uint64_t) == 0, "View is copied in 8-byte words");
    const uint64_t* from = reinterpret_cast<const uint64_t*>(&v);
    uint64_t* to = reinterpret_cast<uint64_t*>(s_col_bytes);
    x.par((int32_t)(sizeof(View) / sizeof(uint64_t)), [&](int32_t i) { to[i] = from[i]; });
    x.one([&]() { cov_column_view(s_col, q.arena + (int64_t)c * (kCovColumnVectors * 3 * (int64_t)v.n)); });
    cov_column(x, s_col, P, s_state, q.head->levels, q.src_row[c / 3], c % 3, q.flags + 2 * c);
}

__global__ __launch_bounds__(kGatherLanes) void k_pose_graph_cov_gather(View v, CovView q) {
    if (q.head->status != VISFS_BA_OK) return;
    const int32_t k = (int32_t)(blockIdx.x * kGatherLanes + threadIdx.x);
    if (k < q.Q) cov_query(v, q, k);
}

}  // namespace posegraph

namespace {

constexpr size_t kHeadDoubles = (sizeof(CovHead) + 7) / 8;

size_t cov_extra_bytes() {
    return sizeof(int32_t) * ((size_t)kCovMaxSources + 4 * (size_t)kCovMaxQueries) + sizeof(double) * kEdgeDoubles + 64;
}
size_t cov_out_doubles(int32_t columns, int32_t Q) { return kHeadDoubles + (size_t)columns + 45 * (size_t)Q; }

// The sources and the queries packed behind the plan's upload at dst + off; the view's pointers relative to `base`.
size_t pack_cov(const CovPlan& cp, char* dst, const char* base, size_t off, CovView& q) {
    auto put = [&](const void* src, size_t bytes) -> const char* {
        if (src && bytes) std::memcpy(dst + off, src, bytes); else if (bytes) std::memset(dst + off, 0, bytes);
        const char* at = base + off;
        off += (bytes + 7) & ~(size_t)7;
        return at;
    };
    q.Q = cp.Q; q.sources = (int32_t)cp.sources.size();
    q.zero_edge = reinterpret_cast<const double*>(put(nullptr, kEdgeDoubles * sizeof(double)));
    q.src_row = reinterpret_cast<const int32_t*>(put(cp.src_row.data(), cp.src_row.size() * sizeof(int32_t)));
    q.query = reinterpret_cast<const int32_t*>(put(cp.query.data(), cp.query.size() * sizeof(int32_t)));
    q.query_src = reinterpret_cast<const int32_t*>(put(cp.query_src.data(), cp.query_src.size() * sizeof(int32_t)));
    return off;
}

// head, flags, joint and relative carved from `w` (the download, in this order)
void carve_cov(CovView& q, double* w) {
    const size_t columns = 3 * (size_t)q.sources;
    q.head = reinterpret_cast<CovHead*>(w); w += kHeadDoubles;
    q.flags = reinterpret_cast<int32_t*>(w); w += columns;
    q.joint = w; w += 36 * (size_t)q.Q;
    q.relative = w;
}

// The buffers of the covariance calls: the fixed part at the first call, the arena whenever a call needs a larger one.
int cov_reserve(visfs_pose_graph* pg, int32_t columns, int32_t n) {
    if (!pg->cov) pg->cov = new CovObject();
    CovObject* c = pg->cov;
    if (c->fixed_doubles == 0) {
        c->up_bytes = up_capacity(pg->maxN, pg->maxE) + 128 + cov_extra_bytes();
        const size_t fixed = work_capacity(pg->maxN, pg->maxE) + cov_out_doubles(3 * kCovMaxSources, kCovMaxQueries);
        if (!pg->device) {
            c->up.assign(c->up_bytes, 0);
            c->work.assign(fixed, 0.0);
        } else {
            HIP_TRY(pg, hipSetDevice(pg->dev));
            RC_TRY(c->h_up.alloc(pg, c->up_bytes));
            RC_TRY(c->d_up.alloc(pg, c->up_bytes));
            RC_TRY(c->d_work.alloc(pg, fixed));
            RC_TRY(c->h_out.alloc(pg, cov_out_doubles(3 * kCovMaxSources, kCovMaxQueries) * sizeof(double)));
        }
        c->fixed_doubles = fixed;
    }
    if (!pg->device) {
        c->column.assign((size_t)kCovColumnVectors * 3 * (size_t)n, 0.0);
        return VISFS_BA_OK;
    }
    const size_t need = (size_t)columns * kCovColumnVectors * 3 * (size_t)n;
    if (need > c->d_arena.cap()) {
        HIP_TRY(pg, hipSetDevice(pg->dev));
        c->valid = false;                                                    // the stored columns go with the old arena
        RC_TRY(c->d_arena.alloc(pg, need));
    }
    return VISFS_BA_OK;
}

// The three stages on the plan; the download lands at *out (host memory).
int run_cov(visfs_pose_graph* pg, const Plan& pl, const CovPlan& cp, const Prm& P, CovView& q, const double** out) {
    const int32_t columns = 3 * (int32_t)cp.sources.size();
    int rc = cov_reserve(pg, columns, pl.n);
    if (rc != VISFS_BA_OK) return rc;
    CovObject* c = pg->cov;
    c->valid = false;
    View v;
    if (!pg->device) {
        const size_t off = pack(pl, nullptr, c->up.data(), c->up.data(), v);
        (void)pack_cov(cp, c->up.data(), c->up.data(), off, q);
        carve(v, c->work.data());
        double* o = c->work.data() + work_capacity(pg->maxN, pg->maxE);
        carve_cov(q, o);
        c->solutions.assign((size_t)columns * 3 * (size_t)pl.n, 0.0);
        q.arena = c->column.data();
        q.sol = c->solutions.data(); q.sol_stride = 3 * (int64_t)pl.n;
        HostExec x;
        State s;
        cov_setup(x, v, P.precond, s, q.head);
        if (q.head->status == VISFS_BA_OK) {
            View col = v;
            cov_column_view(col, q.arena);
            for (int32_t k = 0; k < columns; ++k) {
                cov_column(x, col, P, s, q.head->levels, q.src_row[k / 3], k % 3, q.flags + 2 * k);
                std::memcpy(c->solutions.data() + (size_t)k * 3 * (size_t)pl.n, col.dx, 3 * (size_t)pl.n * sizeof(double));
            }
            for (int32_t k = 0; k < q.Q; ++k) cov_query(v, q, k);
        }
        c->counts = {};
        *out = o;
        return VISFS_BA_OK;
    }
    HIP_TRY(pg, hipSetDevice(pg->dev));
    const size_t off = pack(pl, nullptr, c->h_up.get(), c->d_up.get(), v);
    const size_t bytes = pack_cov(cp, c->h_up.get(), c->d_up.get(), off, q);
    carve(v, c->d_work.get());
    double* d_out = c->d_work.get() + work_capacity(pg->maxN, pg->maxE);
    carve_cov(q, d_out);
    q.arena = c->d_arena.get();
    q.sol_stride = kCovColumnVectors * 3 * (int64_t)pl.n;
    q.sol = c->d_arena.get() + kCovSolutionVector * 3 * (int64_t)pl.n;
    const size_t out_bytes = cov_out_doubles(columns, cp.Q) * sizeof(double);
    int32_t launches = 0;
    HIP_TRY(pg, hipMemcpyAsync(c->d_up.get(), c->h_up.get(), bytes, hipMemcpyHostToDevice, pg->stream));
    hipLaunchKernelGGL(k_pose_graph_cov_setup, dim3(1), dim3(kLanes), 0, pg->stream, v, q, P.precond);
    HIP_TRY(pg, hipGetLastError());
    ++launches;
    if (columns > 0) {
        hipLaunchKernelGGL(k_pose_graph_cov_solve, dim3((unsigned)columns), dim3(kLanes), 0, pg->stream, v, q, P);
        HIP_TRY(pg, hipGetLastError());
        ++launches;
    }
    hipLaunchKernelGGL(k_pose_graph_cov_gather, dim3((unsigned)((cp.Q + kGatherLanes - 1) / kGatherLanes)), dim3(kGatherLanes), 0, pg->stream, v, q);
    HIP_TRY(pg, hipGetLastError());
    ++launches;
    HIP_TRY(pg, hipMemcpyAsync(c->h_out.get(), d_out, out_bytes, hipMemcpyDeviceToHost, pg->stream));
    HIP_TRY(pg, hipStreamSynchronize(pg->stream));
    c->counts = { launches, 2, 1 };
    *out = reinterpret_cast<const double*>(c->h_out.get());
    return VISFS_BA_OK;
}

int check_params(visfs_pose_graph* pg, const visfs_pose_graph_cov_params* p) {
    if (p->max_pcg_iterations < 1) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "max_pcg_iterations must be at least 1");
    if (p->preconditioner != 0 && p->preconditioner != 1) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "preconditioner must be 0 or 1");
    if (!std::isfinite(p->pcg_tolerance) || p->pcg_tolerance < 0.0) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "the tolerance must be finite and not negative");
    return VISFS_BA_OK;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_pose_graph_cov_abi_version(void) { return VISFS_POSE_GRAPH_COV_ABI_VERSION; }

void visfs_pose_graph_cov_default_params(visfs_pose_graph_cov_params* p) {
    if (!p) return;
    p->pcg_tolerance = 1e-8; p->max_pcg_iterations = 500; p->preconditioner = 1;
}

int visfs_pose_graph_covariance(visfs_pose_graph* pg, const visfs_pose_graph_cov_params* p, int32_t N, const double* poses, const uint8_t* fixed, int32_t E,
                                const visfs_pose_graph_edge* edges, int32_t Q, const int32_t* queries, double* joint_out, double* relative_out,
                                visfs_pose_graph_cov_result* result) {
    if (!pg || !p || !poses || !fixed || !edges || !queries || !result) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(pg, [&]() -> int {
        int rc = check_params(pg, p);
        if (rc != VISFS_BA_OK) return rc;
        Plan pl;
        CovPlan cp;
        std::string why;
        if ((rc = make_plan(N, poses, fixed, E, edges, pg->maxN, pg->maxE, pl, why)) != VISFS_BA_OK) return fail(pg, rc, why);
        if ((rc = make_cov_plan(pl, fixed, Q, queries, cp, why)) != VISFS_BA_OK) return fail(pg, rc, why);
        Prm P;
        P.pcg_tol2 = p->pcg_tolerance * p->pcg_tolerance;
        P.max_pcg = p->max_pcg_iterations; P.budget = kCovBudget; P.precond = p->preconditioner;
        CovView q;
        const double* out = nullptr;
        if ((rc = run_cov(pg, pl, cp, P, q, &out)) != VISFS_BA_OK) return rc;
        CovObject* c = pg->cov;
        const int32_t columns = 3 * q.sources;
        CovHead head;
        std::memcpy(&head, out, sizeof head);
        if (head.status != VISFS_BA_OK) return fail(pg, VISFS_BA_ERR_SINGULAR, "a pivot of the preconditioner is not positive");
        c->flags.assign(2 * (size_t)columns, 0);
        if (columns) std::memcpy(c->flags.data(), out + kHeadDoubles, 2 * (size_t)columns * sizeof(int32_t));
        visfs_pose_graph_cov_result r;
        std::memset(&r, 0, sizeof r);
        r.status = VISFS_BA_OK; r.sources = q.sources; r.columns = columns; r.free_vertices = pl.n; r.cost = head.cost;
        for (int32_t k = 0; k < columns; ++k) {
            const int32_t it = c->flags[2 * (size_t)k], flag = c->flags[2 * (size_t)k + 1];
            if (flag == kCovBrokeDown) return fail(pg, VISFS_BA_ERR_SINGULAR, "the conjugate gradients of a column broke down");
            if (flag == kCovUnconverged) ++r.unconverged_columns;
            if (it > r.pcg_iterations_max) r.pcg_iterations_max = it;
            r.pcg_iterations_total += it;
        }
        const double* joint = out + kHeadDoubles + (size_t)columns;
        if (joint_out) std::memcpy(joint_out, joint, 36 * (size_t)Q * sizeof(double));
        if (relative_out) std::memcpy(relative_out, joint + 36 * (size_t)Q, 9 * (size_t)Q * sizeof(double));
        *result = r;
        c->valid = true; c->n = pl.n; c->sources = q.sources; c->sol = q.sol; c->sol_stride = q.sol_stride;
        pg->err.clear();
        return (int)VISFS_BA_OK;
    });
}

int visfs_pose_graph_cov_download_columns(visfs_pose_graph* pg, int32_t source, double* columns, int32_t* iterations) {
    if (!pg) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(pg, [&]() -> int {
        const CovObject* c = pg->cov;
        if (!c || !c->valid) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "no successful covariance call to read from");
        if (source < 0 || source >= c->sources) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "the source is out of range");
        const size_t m = 3 * (size_t)c->n;
        for (int k = 0; k < 3; ++k) {
            const int32_t col = 3 * source + k;
            if (iterations) iterations[k] = c->flags[2 * (size_t)col];
            if (!columns) continue;
            const double* src = c->sol + (int64_t)col * c->sol_stride;
            if (!pg->device) { std::memcpy(columns + k * m, src, m * sizeof(double)); continue; }
            HIP_TRY(pg, hipSetDevice(pg->dev));
            HIP_TRY(pg, hipMemcpyAsync(columns + k * m, src, m * sizeof(double), hipMemcpyDeviceToHost, pg->stream));
        }
        if (pg->device && columns) HIP_TRY(pg, hipStreamSynchronize(pg->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_pose_graph_cov_plan(int32_t N, const uint8_t* fixed, int32_t E, const visfs_pose_graph_edge* edges, int32_t Q, const int32_t* queries,
                              int32_t* n_sources, int32_t* sources, int32_t* query_sources) {
    if (!fixed || !edges || !queries || !n_sources || !sources || !query_sources) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int {
        Plan pl;
        CovPlan cp;
        std::string why;
        const std::vector<double> poses(3 * (size_t)(N > 0 ? N : 0), 0.0);
        int rc = make_plan(N, poses.data(), fixed, E, edges, VISFS_POSE_GRAPH_MAX_VERTICES, VISFS_POSE_GRAPH_MAX_EDGES, pl, why);
        if (rc != VISFS_BA_OK) return rc;
        if ((rc = make_cov_plan(pl, fixed, Q, queries, cp, why)) != VISFS_BA_OK) return rc;
        *n_sources = (int32_t)cp.sources.size();
        if (!cp.sources.empty()) std::memcpy(sources, cp.sources.data(), cp.sources.size() * sizeof(int32_t));
        std::memcpy(query_sources, cp.query_src.data(), cp.query_src.size() * sizeof(int32_t));
        return (int)VISFS_BA_OK;
    });
}

int visfs_pose_graph_cov_last_counts(const visfs_pose_graph* pg, int32_t* launches, int32_t* copies, int32_t* waits) {
    return pg ? (pg->cov ? pg->cov->counts : Counts{}).read(launches, copies, waits) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

int visfs_pose_graph_cov_search_window(const double relative[9], double sigmas, double* linear, double* angular) {
    if (!relative || !linear || !angular) return VISFS_BA_ERR_BAD_ARGUMENT;
    for (int k = 0; k < 9; ++k) if (!std::isfinite(relative[k])) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!std::isfinite(sigmas) || sigmas < 0.0) return VISFS_BA_ERR_BAD_ARGUMENT;
    const double a = relative[0], d = relative[4], b = 0.5 * (relative[1] + relative[3]), t = relative[8];
    if (a < 0.0 || d < 0.0 || t < 0.0) return VISFS_BA_ERR_BAD_ARGUMENT;
    const double h = 0.5 * (a - d);
    const double top = 0.5 * (a + d) + std::sqrt(h * h + b * b);                // the larger eigenvalue of [[a, b], [b, d]]
    if (!std::isfinite(top)) return VISFS_BA_ERR_BAD_ARGUMENT;
    *linear = sigmas * std::sqrt(top);
    *angular = sigmas * std::sqrt(t);
    return VISFS_BA_OK;
}

}  // extern "C"
