// Covariances of the 2-D pose graph (include/visfs_pose_graph_cov.h): what the kernels of
// ba_pose_graph_cov.hip and the one-core twin share, and the host plan of a call.
//
// Three stages, each written once over the executors of ba_pose_graph_object.hpp: `cov_setup` (the linearisation at the poses handed
// in and the set-up of the preconditioner at lambda = 0), `cov_column` (H x = e_col by posegraph::pcg on a View whose vectors are
// the column's own slice while the coefficients are shared and only read) and `cov_query` (the joint and the relative covariance of
// one pair from the solved columns).  The lane sums are those of section 9p, so a column is the same bytes on the device and on
// the host whichever workgroup runs it.
#pragma once
#pragma clang fp contract(off)

#include "ba_pose_graph.hpp"
#include "../../include/visfs_pose_graph_cov.h"

#include <string>
#include <vector>

namespace posegraph {

constexpr int kCovMaxQueries = VISFS_POSE_GRAPH_COV_MAX_QUERIES;
constexpr int kCovMaxSources = VISFS_POSE_GRAPH_COV_MAX_SOURCES;
constexpr int kCovColumnVectors = 8;                  // r, z, p, q, dx, t[0], t[1] and the right-hand side, [n][3] each
constexpr int kCovBudget = 0x7fffffff;                // a column has no budget beyond max_pcg_iterations

enum CovFlag : int32_t { kCovConverged = 0, kCovUnconverged = 1, kCovBrokeDown = 2 };

// what launch 1 leaves for the others
struct CovHead {
    int32_t status, levels;
    double cost;
};

// The queries and the columns of a call, in device memory on the device and in host memory on the twin.
struct CovView {
    int32_t Q = 0, sources = 0;
    const int32_t* src_row = nullptr;     // [sources]: the row of a source
    const int32_t* query = nullptr;       // [Q][2]: vertices a, b
    const int32_t* query_src = nullptr;   // [Q][2]: their sources, -1 for a fixed vertex
    const double* zero_edge = nullptr;    // [10]: an edge record of zeros (cov_query)
    CovHead* head = nullptr;
    int32_t* flags = nullptr;             // [3 sources][2]: iterations, CovFlag
    double* joint = nullptr;              // [Q][36]
    double* relative = nullptr;           // [Q][9]
    double* arena = nullptr;              // the columns' workspaces, kCovColumnVectors * 3 n doubles each
    const double* sol = nullptr;          // column c's solution [n][3] lies at sol + c * sol_stride
    int64_t sol_stride = 0;
};

// The view of one column: `c`, a copy of the call's view, gets its vectors in the workspace `w`; the coefficients stay shared.
PG_HD void cov_column_view(View& c, double* w) {
    const int64_t m = 3 * (int64_t)c.n;
    c.r = w; c.z = w + m; c.p = w + 2 * m; c.q = w + 3 * m; c.dx = w + 4 * m; c.t[0] = w + 5 * m; c.t[1] = w + 6 * m; c.g = w + 7 * m;
}
constexpr int kCovSolutionVector = 4;                 // dx is the fifth vector of a workspace

// Launch 1: the linearisation at the poses handed in, the preconditioner of H at lambda = 0.
template <class X> __host__ __device__ void cov_setup(X& x, const View& v, int32_t precond, State& s, CovHead* head) {
    x.one([&]() {
        s.cost = s.cost0 = s.before = 0.0; s.lambda = 0.0; s.nu = 2.0; s.lam = 0.0;
        s.q = s.it = s.trials = s.term = s.done = s.fail = s.rot = s.rot_seen = s.accepted = s.pcg_total = s.pcg_it = s.levels = s.budget_hit = 0;
        s.status = VISFS_BA_OK;
    });
    x.par(v.N, [&](int32_t i) { v.x[3 * i] = v.pose0[kPoseDoubles * i]; v.x[3 * i + 1] = v.pose0[kPoseDoubles * i + 1]; v.x[3 * i + 2] = 0.0; });
    const double cost = linearize(x, v);
    const bool ok = pcr_setup(x, v, s, 0.0, precond);
    x.one([&]() {
        head->status = ok ? VISFS_BA_OK : VISFS_BA_ERR_SINGULAR;
        head->levels = s.levels;
        head->cost = cost;
    });
}

// Launch 2, one column: H x = e with e the unit vector of coordinate `comp` of row `row`.  `c` is the column's view.
template <class X> __host__ __device__ void cov_column(X& x, const View& c, const Prm& P, State& s, int32_t levels, int32_t row, int32_t comp,
                                                       int32_t* flag) {
    x.one([&]() { s.levels = levels; s.pcg_total = 0; s.pcg_it = 0; s.budget_hit = 0; s.fail = 0; });
    x.par(c.n, [&](int32_t r) {
        for (int m = 0; m < 3; ++m) c.g[3 * r + m] = (r == row && m == comp) ? -1.0 : 0.0;      // pcg solves H dx = -g
    });
    const bool ok = pcg(x, c, P, s, 0.0);
    x.one([&]() {
        flag[0] = s.pcg_it;
        flag[1] = !ok ? kCovBrokeDown : (s.pcg_it >= P.max_pcg ? kCovUnconverged : kCovConverged);
    });
}

// The block of rows `row` in the three solved columns of source `src`: B[3 i + k] = x_(3 src + k)[3 row + i].
PG_HD void cov_block(const CovView& q, int32_t src, int32_t row, double B[9]) {
    for (int k = 0; k < 3; ++k) {
        const double* x = q.sol + (int64_t)(3 * src + k) * q.sol_stride + 3 * (int64_t)row;
        for (int i = 0; i < 3; ++i) B[3 * i + k] = x[i];
    }
}

// Launch 3, one query.  The one place that fixes the order of these operations:
//   Sigma_aa = (X_a[a] + X_a[a]^T) / 2, Sigma_bb likewise, Sigma_ab = (X_b[a] + X_a[b]^T) / 2 with X_s[r] the block of row r in the
//   columns of source s; the blocks of a fixed vertex are zero;
//   relative = (J joint) J^T with J = [J_i J_j] of an edge i = a, j = b at the poses handed in, every sum from left to right.
PG_HD void cov_query(const View& v, const CovView& q, int32_t k) {
    const int32_t sa = q.query_src[2 * k], sb = q.query_src[2 * k + 1];
    const int32_t ra = sa >= 0 ? q.src_row[sa] : -1, rb = sb >= 0 ? q.src_row[sb] : -1;
    double Saa[9], Sbb[9], Sab[9], A[9], B[9];
    for (int m = 0; m < 9; ++m) Saa[m] = Sbb[m] = Sab[m] = 0.0;
    if (sa >= 0) {
        cov_block(q, sa, ra, A);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Saa[3 * i + j] = 0.5 * (A[3 * i + j] + A[3 * j + i]);
    }
    if (sb >= 0) {
        cov_block(q, sb, rb, A);
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Sbb[3 * i + j] = 0.5 * (A[3 * i + j] + A[3 * j + i]);
    }
    if (sa >= 0 && sb >= 0) {
        cov_block(q, sb, ra, A);                       // X_b[a]
        cov_block(q, sa, rb, B);                       // X_a[b]
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Sab[3 * i + j] = 0.5 * (A[3 * i + j] + B[3 * j + i]);
    }
    double* J6 = q.joint + (int64_t)36 * k;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            J6[6 * i + j] = Saa[3 * i + j];
            J6[6 * i + 3 + j] = Sab[3 * i + j];
            J6[6 * (3 + i) + j] = Sab[3 * j + i];
            J6[6 * (3 + i) + 3 + j] = Sbb[3 * i + j];
        }
    // the derivatives of the relative pose: the edge functions of section 9p on an edge (a, b) with a zero measurement
    View e = v;
    e.eij = q.query + 2 * (int64_t)k;
    e.ed = q.zero_edge;
    EdgeEval o;
    edge_eval(e, v.x, 0, o);
    double Ji[9], Jj[9], J[18], T[18];
    edge_jacobians(o, Ji, Jj);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { J[6 * i + j] = Ji[3 * i + j]; J[6 * i + 3 + j] = Jj[3 * i + j]; }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 6; ++j) {
            double a = 0.0;
            for (int m = 0; m < 6; ++m) a += J[6 * i + m] * J6[6 * m + j];
            T[6 * i + j] = a;
        }
    double* R = q.relative + (int64_t)9 * k;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0.0;
            for (int m = 0; m < 6; ++m) a += T[6 * i + m] * J[6 * j + m];
            R[3 * i + j] = a;
        }
}

// ---------------------------------------------------------------- the host plan (no HIP)
struct CovPlan {
    int32_t Q = 0;
    std::vector<int32_t> sources;         // vertices
    std::vector<int32_t> src_row;         // their rows
    std::vector<int32_t> query, query_src;
};

// The checks a covariance call adds to those of make_plan, and the sources: the distinct free vertices of the queries in order of
// first appearance, a before b.
inline int make_cov_plan(const Plan& pl, const uint8_t* fixed, int32_t Q, const int32_t* queries, CovPlan& cp, std::string& why) {
    if (Q < 1 || Q > kCovMaxQueries) { why = "the number of queries must lie in [1, 1024]"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    const int32_t N = pl.N;
    for (int64_t k = 0; k < 2 * (int64_t)Q; ++k)
        if (queries[k] < 0 || queries[k] >= N) { why = "a query's vertex is out of range"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    cp.Q = Q;
    cp.query.assign(queries, queries + 2 * (size_t)Q);
    cp.query_src.assign(2 * (size_t)Q, -1);
    std::vector<int32_t> src_of((size_t)N, -1);
    for (size_t k = 0; k < 2 * (size_t)Q; ++k) {
        const int32_t vtx = queries[k];
        if (pl.row_of[(size_t)vtx] < 0) continue;
        if (src_of[(size_t)vtx] < 0) {
            src_of[(size_t)vtx] = (int32_t)cp.sources.size();
            cp.sources.push_back(vtx);
            cp.src_row.push_back(pl.row_of[(size_t)vtx]);
        }
        cp.query_src[k] = src_of[(size_t)vtx];
    }
    if ((int32_t)cp.sources.size() > kCovMaxSources) { why = "more than 64 distinct free vertices among the queries"; return VISFS_BA_ERR_UNSUPPORTED; }
    // every free vertex must reach a fixed one through edges: union-find, the fixed vertices being one set (N)
    std::vector<int32_t> parent((size_t)N + 1);
    for (int32_t i = 0; i <= N; ++i) parent[(size_t)i] = i;
    auto find = [&](int32_t a) {
        while (parent[(size_t)a] != a) { parent[(size_t)a] = parent[(size_t)parent[(size_t)a]]; a = parent[(size_t)a]; }
        return a;
    };
    auto node = [&](int32_t vtx) { return fixed[vtx] ? N : vtx; };
    for (int32_t k = 0; k < pl.E; ++k) {
        const int32_t a = find(node(pl.eij[2 * (size_t)k])), b = find(node(pl.eij[2 * (size_t)k + 1]));
        if (a != b) parent[(size_t)(a < b ? a : b)] = a < b ? b : a;          // the larger index stays the root: N, if it is there
    }
    for (int32_t i = 0; i < N; ++i)
        if (!fixed[i] && find(i) != N) { why = "a free vertex is not linked to any fixed vertex: the covariance does not exist"; return VISFS_BA_ERR_SINGULAR; }
    return VISFS_BA_OK;
}

}  // namespace posegraph
