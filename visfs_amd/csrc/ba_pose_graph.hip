// The 2-D pose graph over the loop-closure constraints (include/visfs_pose_graph.h).
//
//   k_pose_graph   grid (1): one workgroup of kLanes work items runs posegraph::run from start to end: the edge-parallel
//                  linearisation, the row-parallel gathers, the cyclic-reduction set-up, the preconditioned conjugate gradients, the
//                  trial and the Levenberg-Marquardt control, separated by workgroup barriers.  Vectors and coefficients live in
//                  device memory, LDS holds the lanes' partial sums and the State.  Nothing is read back during the loop and no
//                  workgroup waits for another.
// A call is one upload (the plan), one launch, one download (the record, the poses, chi2) and one wait.  The one-core twin runs the
// same `run` with loops for the collective operations.
#pragma clang fp contract(off)
#include "ba_pose_graph_object.hpp"
#include "ba_host.hpp"

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ba_submap.hpp"

using namespace posegraph;
using namespace host;

namespace posegraph {

__global__ __launch_bounds__(kLanes) void k_pose_graph(View v, Prm P) {
    __shared__ double s_part[kLanes];
    __shared__ State s_state;
    DeviceExec x{ s_part, (int32_t)threadIdx.x };
    run(x, v, P, s_state);
}

}  // namespace posegraph

namespace {

// One run of `mode` on the plan: the record, the poses and chi2 land at `out` (out_doubles of them, host memory).
int run_plan(visfs_pose_graph* pg, const Plan& pl, const Prm& P, const double* hook_r, const double** out) {
    View v;
    if (!pg->device) {
        const size_t bytes = pack(pl, hook_r, pg->up.data(), pg->up.data(), v);
        (void)bytes;
        double* o = carve(v, pg->work.data());
        HostExec x;
        State s;
        run(x, v, P, s);
        pg->view = v;
        *out = o;
        return VISFS_BA_OK;
    }
    HIP_TRY(pg, hipSetDevice(pg->dev));
    const size_t bytes = pack(pl, hook_r, pg->h_up.get(), pg->d_up.get(), v);
    double* d_out = carve(v, pg->d_work.get());
    const size_t out_bytes = out_doubles(pl.N, pl.E) * sizeof(double);
    HIP_TRY(pg, hipMemcpyAsync(pg->d_up.get(), pg->h_up.get(), bytes, hipMemcpyHostToDevice, pg->stream));
    hipLaunchKernelGGL(k_pose_graph, dim3(1), dim3(kLanes), 0, pg->stream, v, P);
    HIP_TRY(pg, hipGetLastError());
    HIP_TRY(pg, hipMemcpyAsync(pg->h_out.get(), d_out, out_bytes, hipMemcpyDeviceToHost, pg->stream));
    HIP_TRY(pg, hipStreamSynchronize(pg->stream));
    pg->view = v;
    *out = reinterpret_cast<const double*>(pg->h_out.get());
    return VISFS_BA_OK;
}

// a work array of the last run to host memory (hooks)
int fetch(visfs_pose_graph* pg, const double* src, size_t count, double* dst) {
    if (!dst || count == 0) return VISFS_BA_OK;
    if (!pg->device) { std::memcpy(dst, src, count * sizeof(double)); return VISFS_BA_OK; }
    HIP_TRY(pg, hipSetDevice(pg->dev));
    HIP_TRY(pg, hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, pg->stream));
    HIP_TRY(pg, hipStreamSynchronize(pg->stream));
    return VISFS_BA_OK;
}

Prm hook_prm(int32_t mode) {
    Prm P;
    P.mode = mode; P.max_it = 1; P.max_pcg = 1; P.budget = 1;
    return P;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_pose_graph_abi_version(void) { return VISFS_POSE_GRAPH_ABI_VERSION; }

void visfs_pose_graph_default_params(visfs_pose_graph_params* p) {
    if (!p) return;
    p->function_tolerance = 1e-6; p->pcg_tolerance = 1e-8;
    p->max_iterations = 20; p->max_pcg_iterations = 500; p->pcg_budget = 10000; p->preconditioner = 1;
}

int visfs_pose_graph_create(visfs_ba_handle* h, int32_t max_vertices, int32_t max_edges, visfs_pose_graph** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (max_vertices < 1 || max_edges < 1) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (max_vertices > VISFS_POSE_GRAPH_MAX_VERTICES || max_edges > VISFS_POSE_GRAPH_MAX_EDGES) return VISFS_BA_ERR_UNSUPPORTED;
    return guarded(nullptr, [&]() -> int {
        visfs_pose_graph* pg = new visfs_pose_graph();
        pg->maxN = max_vertices; pg->maxE = max_edges;
        pg->up_bytes = up_capacity(max_vertices, max_edges) + 128;
        pg->work_doubles = work_capacity(max_vertices, max_edges);
        if (!h) {
            pg->up.assign(pg->up_bytes, 0);
            pg->work.assign(pg->work_doubles, 0.0);
            *out = pg;
            return (int)VISFS_BA_OK;
        }
        pg->device = true; pg->dev = visfs_internal_device(h); pg->stream = visfs_internal_stream(h);
        const int rc = [&]() -> int {
            HIP_TRY(pg, hipSetDevice(pg->dev));
            RC_TRY(pg->h_up.alloc(pg, pg->up_bytes));
            RC_TRY(pg->d_up.alloc(pg, pg->up_bytes));
            RC_TRY(pg->d_work.alloc(pg, pg->work_doubles));
            RC_TRY(pg->h_out.alloc(pg, out_doubles(max_vertices, max_edges) * sizeof(double)));
            return (int)VISFS_BA_OK;
        }();
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, pg->err.c_str()); delete pg; return rc; }
        *out = pg;
        return (int)VISFS_BA_OK;
    });
}

void visfs_pose_graph_destroy(visfs_pose_graph* pg) {
    delete pg;
}

const char* visfs_pose_graph_last_error(const visfs_pose_graph* pg) { return pg ? pg->err.c_str() : ""; }

int visfs_pose_graph_optimize(visfs_pose_graph* pg, const visfs_pose_graph_params* p, int32_t N, const double* poses, const uint8_t* fixed, int32_t E,
                              const visfs_pose_graph_edge* edges, double* poses_out, double* chi2_out, visfs_pose_graph_result* result) {
    if (!pg || !p || !poses || !fixed || !edges || !poses_out || !result) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(pg, [&]() -> int {
        if (p->max_iterations < 1 || p->max_iterations > VISFS_POSE_GRAPH_MAX_ITERATIONS) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "max_iterations must lie in [1, 50]");
        if (p->max_pcg_iterations < 1 || p->pcg_budget < 1) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "max_pcg_iterations and pcg_budget must be at least 1");
        if (p->preconditioner != 0 && p->preconditioner != 1) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "preconditioner must be 0 or 1");
        const double w[2] = { p->function_tolerance, p->pcg_tolerance };
        for (double a : w) if (!std::isfinite(a) || a < 0.0) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "the tolerances must be finite and not negative");
        Plan pl;
        std::string why;
        int rc = make_plan(N, poses, fixed, E, edges, pg->maxN, pg->maxE, pl, why);
        if (rc != VISFS_BA_OK) return fail(pg, rc, why);
        Prm P;
        P.ftol = p->function_tolerance; P.pcg_tol2 = p->pcg_tolerance * p->pcg_tolerance;
        P.max_it = p->max_iterations; P.max_pcg = p->max_pcg_iterations; P.budget = p->pcg_budget; P.precond = p->preconditioner;
        P.mode = kOptimize;
        const double* out = nullptr;
        if ((rc = run_plan(pg, pl, P, nullptr, &out)) != VISFS_BA_OK) return rc;
        std::memcpy(result, out, sizeof *result);
        std::memcpy(poses_out, out + kResDoubles, 3 * (size_t)N * sizeof(double));
        if (chi2_out) std::memcpy(chi2_out, out + kResDoubles + 3 * (size_t)N, (size_t)E * sizeof(double));
        pg->trials = result->trials;
        pg->counts = { pg->device ? 1 : 0, pg->device ? 2 : 0, pg->device ? 1 : 0 };
        pg->err.clear();
        return (int)VISFS_BA_OK;
    });
}

int visfs_pose_graph_download_trace(visfs_pose_graph* pg, int32_t cap, double* trace, int32_t* trials) {
    if (!pg || !trials || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(pg, [&]() -> int {
        const int32_t n = pg->trials < kMaxTrials ? pg->trials : kMaxTrials;
        *trials = n;
        if (!trace || n == 0) return (int)VISFS_BA_OK;
        if (cap < n) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "the hook's array is too small");
        return fetch(pg, pg->view.trace, (size_t)n * kTraceItems, trace);
    });
}

int visfs_pose_graph_linearize(visfs_pose_graph* pg, int32_t N, const double* poses, const uint8_t* fixed, int32_t E, const visfs_pose_graph_edge* edges,
                               int32_t* n_rows, double* edge_blocks, double* g, double* D, double* C, double* cost, double* chi2) {
    if (!pg || !poses || !fixed || !edges) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(pg, [&]() -> int {
        Plan pl;
        std::string why;
        int rc = make_plan(N, poses, fixed, E, edges, pg->maxN, pg->maxE, pl, why);
        if (rc != VISFS_BA_OK) return fail(pg, rc, why);
        const double* out = nullptr;
        if ((rc = run_plan(pg, pl, hook_prm(kLinearize), nullptr, &out)) != VISFS_BA_OK) return rc;
        pg->trials = 0;
        visfs_pose_graph_result res;
        std::memcpy(&res, out, sizeof res);
        if (n_rows) *n_rows = pl.n;
        if (cost) *cost = res.initial_cost;
        if (chi2) std::memcpy(chi2, out + kResDoubles + 3 * (size_t)N, (size_t)E * sizeof(double));
        const View& v = pg->view;
        if ((rc = fetch(pg, v.eb, 27 * (size_t)E, edge_blocks)) != VISFS_BA_OK) return rc;
        if ((rc = fetch(pg, v.g, 3 * (size_t)pl.n, g)) != VISFS_BA_OK) return rc;
        if ((rc = fetch(pg, v.D, 9 * (size_t)pl.n, D)) != VISFS_BA_OK) return rc;
        return fetch(pg, v.C, 9 * (size_t)pl.n, C);
    });
}

int visfs_pose_graph_precondition(visfs_pose_graph* pg, int32_t preconditioner, double lambda, int32_t N, const double* poses, const uint8_t* fixed, int32_t E,
                                  const visfs_pose_graph_edge* edges, const double* r, double* z) {
    if (!pg || !poses || !fixed || !edges || !r || !z) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(pg, [&]() -> int {
        if (preconditioner != 0 && preconditioner != 1) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "preconditioner must be 0 or 1");
        if (!std::isfinite(lambda) || lambda < 0.0) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "lambda must be finite and not negative");
        Plan pl;
        std::string why;
        int rc = make_plan(N, poses, fixed, E, edges, pg->maxN, pg->maxE, pl, why);
        if (rc != VISFS_BA_OK) return fail(pg, rc, why);
        for (int64_t k = 0; k < 3 * (int64_t)pl.n; ++k) if (!std::isfinite(r[k])) return fail(pg, VISFS_BA_ERR_BAD_ARGUMENT, "r is not finite");
        Prm P = hook_prm(kPrecondition);
        P.hook_lambda = lambda; P.precond = preconditioner;
        const double* out = nullptr;
        if ((rc = run_plan(pg, pl, P, r, &out)) != VISFS_BA_OK) return rc;
        pg->trials = 0;
        visfs_pose_graph_result res;
        std::memcpy(&res, out, sizeof res);
        if (res.status != VISFS_BA_OK) return fail(pg, res.status, "a pivot of the preconditioner is not positive");
        return fetch(pg, pg->view.z, 3 * (size_t)pl.n, z);
    });
}

int visfs_pose_graph_plan(int32_t N, const uint8_t* fixed, int32_t E, const visfs_pose_graph_edge* edges, int32_t* n_rows, int32_t* row_of, int32_t* inc_ptr,
                          int32_t* inc, int32_t* chain_ptr, int32_t* chain) {
    if (!fixed || !edges || !n_rows || !row_of || !inc_ptr || !inc || !chain_ptr || !chain) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int {
        Plan pl;
        std::string why;
        const std::vector<double> poses(3 * (size_t)(N > 0 ? N : 0), 0.0);
        const int rc = make_plan(N, poses.data(), fixed, E, edges, VISFS_POSE_GRAPH_MAX_VERTICES, VISFS_POSE_GRAPH_MAX_EDGES, pl, why);
        if (rc != VISFS_BA_OK) return rc;
        *n_rows = pl.n;
        std::memcpy(row_of, pl.row_of.data(), pl.row_of.size() * sizeof(int32_t));
        std::memcpy(inc_ptr, pl.inc_ptr.data(), pl.inc_ptr.size() * sizeof(int32_t));
        if (!pl.inc.empty()) std::memcpy(inc, pl.inc.data(), pl.inc.size() * sizeof(int32_t));
        std::memcpy(chain_ptr, pl.chain_ptr.data(), pl.chain_ptr.size() * sizeof(int32_t));
        if (!pl.chain.empty()) std::memcpy(chain, pl.chain.data(), pl.chain.size() * sizeof(int32_t));
        return (int)VISFS_BA_OK;
    });
}

int visfs_pose_graph_last_counts(const visfs_pose_graph* pg, int32_t* launches, int32_t* copies, int32_t* waits) {
    return pg ? pg->counts.read(launches, copies, waits) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

int visfs_pose_graph_edge_from_refine(const double a[3], const visfs_scan_refine_result* r, double z[3], double W[9]) {
    if (!a || !r || !z || !W || !r->refined) return VISFS_BA_ERR_BAD_ARGUMENT;
    const double in[6] = { a[0], a[1], a[2], r->x, r->y, r->yaw };
    for (double v : in) if (!std::isfinite(v)) return VISFS_BA_ERR_BAD_ARGUMENT;
    for (double v : r->information) if (!std::isfinite(v)) return VISFS_BA_ERR_BAD_ARGUMENT;
    const double c = std::cos(a[2]), s = std::sin(a[2]);
    const double dx = r->x - a[0], dy = r->y - a[1], dth = r->yaw - a[2];
    z[0] = c * dx + s * dy;
    z[1] = c * dy - s * dx;
    z[2] = dth - kTwoPi * std::rint(dth / kTwoPi);
    const double B[9] = { c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0 };           // blkdiag(R, 1)
    double T[9], M[9];
    mm3(r->information, B, T);
    mtm3(B, T, 1.0, M);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W[3 * i + j] = 0.5 * (M[3 * i + j] + M[3 * j + i]);
    return VISFS_BA_OK;
}

}  // extern "C"
