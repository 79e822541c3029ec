// The 2-D pose graph (include/visfs_pose_graph.h): what the kernel of ba_pose_graph.hip and the one-core twin
// share, and the host plan.
//
// The whole optimisation is written once, `run`, over an executor X that supplies four collective operations: `par` (every item of a
// range once, then a barrier), `sum` (the lane reduction: lane t adds its items t, t + kLanes, ... in increasing order, the lanes'
// partials are added by the tree p[t] += p[t + s], s = kLanes / 2 ... 1), `maxv` and `one` (work item 0 alone, between barriers).
// On the device X is one workgroup of kLanes work items with the partials in LDS; on the host it is a loop.  Every double is formed
// by the same + - * / sqrt in the same order on both: contraction is off, the only transcendentals (cos and sin of the initial yaws)
// come from the host, the rotation by yaw - initial yaw from scanrefine::sincos_poly.  The scalars that steer the loop live in one
// State that only `one` writes, so every work item takes the same branches.
#pragma once
#pragma clang fp contract(off)

#include "ba_scan_refine.hpp"
#include "../../include/visfs_pose_graph.h"

#include <cmath>
#include <string>
#include <vector>

namespace posegraph {

#define PG_HD __host__ __device__ inline

constexpr int kLanes = VISFS_POSE_GRAPH_LANES;
constexpr int kMaxLevels = 13;
constexpr int kMaxTrials = VISFS_POSE_GRAPH_MAX_TRIALS;
constexpr int kTrialsPerIteration = 10;
constexpr int kTraceItems = VISFS_POSE_GRAPH_TRACE_ITEMS;
constexpr int kEdgeDoubles = 10;                      // z[3], information 00 01 02 11 12 22, huber_delta
constexpr int kPoseDoubles = 5;                       // x, y, initial yaw, its cos and sin
constexpr double kRejectedCost = 1.7976931348623157e308;
constexpr double kTwoPi = 6.283185307179586476925286766559;

enum Mode : int32_t { kOptimize = 0, kLinearize = 1, kPrecondition = 2 };

struct Prm {
    double ftol = 0.0, pcg_tol2 = 0.0, hook_lambda = 0.0;
    int32_t max_it = 0, max_pcg = 0, budget = 0, precond = 1, mode = kOptimize;
};

// Everything a run reads and writes, in device memory on the device and in host memory on the twin.
struct View {
    int32_t N = 0, E = 0, n = 0, pad = 0;
    // the upload
    const double* pose0 = nullptr;        // [N][5]
    const double* ed = nullptr;           // [E][10]
    const double* hook_r = nullptr;       // [n][3] (kPrecondition)
    const int32_t* eij = nullptr;         // [E][2]
    const int32_t* row_of = nullptr;      // [N]: the row of a free vertex, -1 for a fixed one
    const int32_t* inc_ptr = nullptr;     // [n + 1]
    const int32_t* inc = nullptr;         // 2 * edge + (1 when the row is the edge's j)
    const int32_t* chain_ptr = nullptr;   // [n + 1]
    const int32_t* chain = nullptr;       // 2 * edge + (1 when the row is the edge's j, row + 1 its i)
    // the work
    double* x = nullptr;                  // [N][3]: x, y, yaw - initial yaw in force
    double* xt = nullptr;                 // [N][3]: of the trial
    double* eb = nullptr;                 // [E][27]: H_ii, H_ij, H_jj
    double* eg = nullptr;                 // [E][6]: the edge's share of g_i and g_j
    double* chi2 = nullptr;               // [E]
    double* g = nullptr;                  // [n][3]
    double* D = nullptr;                  // [n][9]
    double* C = nullptr;                  // [n][9]
    double* pD[2] = { nullptr, nullptr }; // the cyclic reduction's levels, ping-pong
    double* pA[2] = { nullptr, nullptr };
    double* pC[2] = { nullptr, nullptr };
    double* Dinv = nullptr;               // [n][9]
    double* al = nullptr;                 // [kMaxLevels][n][9]
    double* ga = nullptr;
    double* r = nullptr;                  // [n][3] each
    double* z = nullptr;
    double* p = nullptr;
    double* q = nullptr;
    double* dx = nullptr;
    double* t[2] = { nullptr, nullptr };
    double* trace = nullptr;              // [kMaxTrials][kTraceItems]
    // the download: the record, then the poses [N][3], then chi2 [E]
    visfs_pose_graph_result* res = nullptr;
    double* out_poses = nullptr;
    double* out_chi2 = nullptr;
};

struct State {
    double cost, cost0, before, lambda, nu, lam;
    int32_t q, it, trials, term, done, fail, rot, rot_seen, accepted, pcg_total, pcg_it, levels, status, budget_hit;
};

PG_HD bool finite(double v) { return (v - v) == 0.0; }

// ---------------------------------------------------------------- 3 x 3 blocks, row-major
PG_HD void mm3(const double* A, const double* B, double* R) {               // R = A B
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
PG_HD void mtm3(const double* A, const double* B, double w, double* R) {    // R = w A^T B
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = w * ((A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j]);
}
PG_HD void mv3(const double* M, const double* v, double* o) {               // o = M v
    for (int k = 0; k < 3; ++k) o[k] = (M[3 * k] * v[0] + M[3 * k + 1] * v[1]) + M[3 * k + 2] * v[2];
}
PG_HD void mtv3(const double* M, const double* v, double* o) {              // o = M^T v
    for (int k = 0; k < 3; ++k) o[k] = (M[k] * v[0] + M[3 + k] * v[1]) + M[6 + k] * v[2];
}
PG_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// The inverse of the symmetric S (its upper triangle is read) through S = L D L^T; false when a pivot is not positive.
PG_HD bool inv3_ldl(const double* S, double* I) {
    const double d0 = S[0];
    if (!(d0 > 0.0)) return false;
    const double l10 = S[1] / d0, l20 = S[2] / d0;
    const double d1 = S[4] - l10 * S[1];
    if (!(d1 > 0.0)) return false;
    const double u12 = S[5] - l20 * S[1];
    const double l21 = u12 / d1;
    const double d2 = (S[8] - l20 * S[2]) - l21 * u12;
    if (!(d2 > 0.0)) return false;
    const double m10 = -l10, m21 = -l21, m20 = l10 * l21 - l20;             // L^-1
    const double i22 = 1.0 / d2, i12 = m21 / d2, i02 = m20 / d2;
    const double i11 = 1.0 / d1 + m21 * i12, i01 = m10 / d1 + m20 * i12;
    const double i00 = (1.0 / d0 + m10 * (m10 / d1)) + m20 * i02;
    I[0] = i00; I[1] = i01; I[2] = i02; I[3] = i01; I[4] = i11; I[5] = i12; I[6] = i02; I[7] = i12; I[8] = i22;
    return finite(i00) && finite(i11) && finite(i22) && finite(i01) && finite(i02) && finite(i12);
}

// ---------------------------------------------------------------- one edge
struct EdgeEval { double e[3], oe[3], chi2, w, rho, c, s, ux, uy; };

// The residual, chi2, the robust weight and cost of edge k at the poses x ([N][3]: x, y, yaw - initial yaw).
PG_HD void edge_eval(const View& v, const double* __restrict__ x, int32_t k, EdgeEval& o) {
    const int32_t i = v.eij[2 * k], j = v.eij[2 * k + 1];
    const double* pi = v.pose0 + (int64_t)kPoseDoubles * i;
    const double* pj = v.pose0 + (int64_t)kPoseDoubles * j;
    const double* d = v.ed + (int64_t)kEdgeDoubles * k;
    const double di = x[3 * i + 2], dj = x[3 * j + 2];
    double sd, cd;
    scanrefine::sincos_poly(di, sd, cd);
    o.c = pi[3] * cd - pi[4] * sd;
    o.s = pi[4] * cd + pi[3] * sd;
    const double dx = x[3 * j] - x[3 * i], dy = x[3 * j + 1] - x[3 * i + 1];
    o.ux = o.c * dx + o.s * dy;
    o.uy = o.c * dy - o.s * dx;
    o.e[0] = o.ux - d[0];
    o.e[1] = o.uy - d[1];
    const double dth = ((pj[2] + dj) - (pi[2] + di)) - d[2];
    o.e[2] = dth - kTwoPi * rint(dth / kTwoPi);
    o.oe[0] = (d[3] * o.e[0] + d[4] * o.e[1]) + d[5] * o.e[2];
    o.oe[1] = (d[4] * o.e[0] + d[6] * o.e[1]) + d[7] * o.e[2];
    o.oe[2] = (d[5] * o.e[0] + d[7] * o.e[1]) + d[8] * o.e[2];
    o.chi2 = (o.e[0] * o.oe[0] + o.e[1] * o.oe[1]) + o.e[2] * o.oe[2];
    o.w = 1.0; o.rho = o.chi2;
    const double delta = d[9];
    if (delta > 0.0) {
        const double sq = sqrt(o.chi2 > 0.0 ? o.chi2 : 0.0);
        if (sq > delta) { o.w = delta / sq; o.rho = 2.0 * delta * sq - delta * delta; }
    }
}

PG_HD double edge_cost(const View& v, const double* __restrict__ x, int32_t k) {
    EdgeEval o;
    edge_eval(v, x, k, o);
    return o.rho;
}

// The derivatives of an edge's residual by the poses of its i and of its j, row-major, from the edge's evaluation.
PG_HD void edge_jacobians(const EdgeEval& o, double Ji[9], double Jj[9]) {
    Ji[0] = -o.c; Ji[1] = -o.s; Ji[2] = o.uy; Ji[3] = o.s; Ji[4] = -o.c; Ji[5] = -o.ux; Ji[6] = 0.0; Ji[7] = 0.0; Ji[8] = -1.0;
    Jj[0] = o.c; Jj[1] = o.s; Jj[2] = 0.0; Jj[3] = -o.s; Jj[4] = o.c; Jj[5] = 0.0; Jj[6] = 0.0; Jj[7] = 0.0; Jj[8] = 1.0;
}

// Edge k's chi2, gradient shares and three blocks at v.x; returns its cost.
PG_HD double edge_linearize(const View& v, int32_t k) {
    EdgeEval o;
    edge_eval(v, v.x, k, o);
    v.chi2[k] = o.chi2;
    const double* d = v.ed + (int64_t)kEdgeDoubles * k;
    const double Om[9] = { d[3], d[4], d[5], d[4], d[6], d[7], d[5], d[7], d[8] };
    double Ji[9], Jj[9];
    edge_jacobians(o, Ji, Jj);
    double* eb = v.eb + (int64_t)27 * k;
    double* eg = v.eg + (int64_t)6 * k;
    double OJ[9], t[3];
    mm3(Om, Ji, OJ);
    mtm3(Ji, OJ, o.w, eb);
    mm3(Om, Jj, OJ);
    mtm3(Ji, OJ, o.w, eb + 9);
    mtm3(Jj, OJ, o.w, eb + 18);
    mtv3(Ji, o.oe, t);
    eg[0] = o.w * t[0]; eg[1] = o.w * t[1]; eg[2] = o.w * t[2];
    mtv3(Jj, o.oe, t);
    eg[3] = o.w * t[0]; eg[4] = o.w * t[1]; eg[5] = o.w * t[2];
    return o.rho;
}

// g, D and C of row r from the row's lists, in their order
PG_HD void gather_row(const View& v, int32_t r) {
    double g[3] = { 0.0, 0.0, 0.0 }, D[9];
    for (int k = 0; k < 9; ++k) D[k] = 0.0;
    for (int32_t a = v.inc_ptr[r]; a < v.inc_ptr[r + 1]; ++a) {
        const int32_t code = v.inc[a], k = code >> 1, side = code & 1;
        const double* b = v.eb + (int64_t)27 * k + 18 * side;
        const double* h = v.eg + (int64_t)6 * k + 3 * side;
        for (int m = 0; m < 9; ++m) D[m] += b[m];
        for (int m = 0; m < 3; ++m) g[m] += h[m];
    }
    for (int m = 0; m < 9; ++m) v.D[9 * r + m] = D[m];
    for (int m = 0; m < 3; ++m) v.g[3 * r + m] = g[m];
    for (int m = 0; m < 9; ++m) D[m] = 0.0;
    for (int32_t a = v.chain_ptr[r]; a < v.chain_ptr[r + 1]; ++a) {
        const int32_t code = v.chain[a], k = code >> 1, flip = code & 1;
        const double* b = v.eb + (int64_t)27 * k + 9;
        if (!flip) { for (int m = 0; m < 9; ++m) D[m] += b[m]; }
        else { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) D[3 * i + j] += b[3 * j + i]; }
    }
    for (int m = 0; m < 9; ++m) v.C[9 * r + m] = D[m];
}

// q_r = (H p)_r + lambda p_r over the row's incidence list
PG_HD void hp_row(const View& v, double lam, int32_t r, double q[3]) {
    const double pr[3] = { v.p[3 * r], v.p[3 * r + 1], v.p[3 * r + 2] };
    double acc[3] = { 0.0, 0.0, 0.0 }, t[3];
    for (int32_t a = v.inc_ptr[r]; a < v.inc_ptr[r + 1]; ++a) {
        const int32_t code = v.inc[a], k = code >> 1, side = code & 1;
        const double* b = v.eb + (int64_t)27 * k;
        mv3(b + 18 * side, pr, t);
        acc[0] += t[0]; acc[1] += t[1]; acc[2] += t[2];
        const int32_t ro = v.row_of[v.eij[2 * k + (1 - side)]];
        if (ro >= 0) {
            const double* po = v.p + 3 * ro;
            if (!side) mv3(b + 9, po, t); else mtv3(b + 9, po, t);
            acc[0] += t[0]; acc[1] += t[1]; acc[2] += t[2];
        }
    }
    for (int m = 0; m < 3; ++m) q[m] = acc[m] + lam * pr[m];
}

// ---------------------------------------------------------------- the preconditioner
// Level 0 of the cyclic reduction: (A, D + lambda I, C) of row r; block-Jacobi keeps the diagonal only.
PG_HD void pcr_start(const View& v, double lam, int32_t precond, int32_t r) {
    double* D = v.pD[0] + 9 * r; double* A = v.pA[0] + 9 * r; double* C = v.pC[0] + 9 * r;
    for (int m = 0; m < 9; ++m) D[m] = v.D[9 * r + m];
    D[0] += lam; D[4] += lam; D[8] += lam;
    const bool up = precond && r > 0, down = precond && r + 1 < v.n;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[3 * i + j] = up ? v.C[9 * (r - 1) + 3 * j + i] : 0.0;
            C[3 * i + j] = down ? v.C[9 * r + 3 * i + j] : 0.0;
        }
}

// One level at distance s of row r: alpha and gamma stored, (A, D, C) of the next level written.
PG_HD void pcr_level(const View& v, int32_t cur, int32_t level, int32_t s, int32_t r) {
    const int32_t n = v.n;
    const double* D = v.pD[cur]; const double* A = v.pA[cur]; const double* C = v.pC[cur];
    double* Dn = v.pD[cur ^ 1] + 9 * r; double* An = v.pA[cur ^ 1] + 9 * r; double* Cn = v.pC[cur ^ 1] + 9 * r;
    double* al = v.al + ((int64_t)level * n + r) * 9;
    double* ga = v.ga + ((int64_t)level * n + r) * 9;
    double T[9], W[9];
    for (int m = 0; m < 9; ++m) Dn[m] = D[9 * r + m];
    if (r - s >= 0) {
        mm3(A + 9 * r, v.Dinv + 9 * (r - s), T);
        for (int m = 0; m < 9; ++m) { T[m] = -T[m]; al[m] = T[m]; }
        mm3(T, C + 9 * (r - s), W);
        for (int m = 0; m < 9; ++m) Dn[m] += W[m];
        mm3(T, A + 9 * (r - s), W);
        for (int m = 0; m < 9; ++m) An[m] = W[m];
    } else {
        for (int m = 0; m < 9; ++m) { al[m] = 0.0; An[m] = 0.0; }
    }
    if (r + s < n) {
        mm3(C + 9 * r, v.Dinv + 9 * (r + s), T);
        for (int m = 0; m < 9; ++m) { T[m] = -T[m]; ga[m] = T[m]; }
        mm3(T, A + 9 * (r + s), W);
        for (int m = 0; m < 9; ++m) Dn[m] += W[m];
        mm3(T, C + 9 * (r + s), W);
        for (int m = 0; m < 9; ++m) Cn[m] = W[m];
    } else {
        for (int m = 0; m < 9; ++m) { ga[m] = 0.0; Cn[m] = 0.0; }
    }
}

// out_r = (in_r + alpha_r in_{r-s}) + gamma_r in_{r+s}
PG_HD void pcr_apply_level(const View& v, int32_t level, int32_t s, const double* in, double* out, int32_t r) {
    const int32_t n = v.n;
    double a[3] = { in[3 * r], in[3 * r + 1], in[3 * r + 2] }, t[3];
    if (r - s >= 0) { mv3(v.al + ((int64_t)level * n + r) * 9, in + 3 * (r - s), t); a[0] += t[0]; a[1] += t[1]; a[2] += t[2]; }
    if (r + s < n) { mv3(v.ga + ((int64_t)level * n + r) * 9, in + 3 * (r + s), t); a[0] += t[0]; a[1] += t[1]; a[2] += t[2]; }
    out[3 * r] = a[0]; out[3 * r + 1] = a[1]; out[3 * r + 2] = a[2];
}

// The set-up of M = the block-tridiagonal part of H + lambda I (or its block diagonal); false when a pivot is not positive.
template <class X> __host__ __device__ bool pcr_setup(X& x, const View& v, State& s, double lam, int32_t precond) {
    const int32_t n = v.n;
    x.one([&]() { s.fail = 0; s.levels = 0; });
    x.par(n, [&](int32_t r) { pcr_start(v, lam, precond, r); });
    int32_t cur = 0, level = 0;
    if (precond)
        for (int32_t d = 1; d < n; d <<= 1) {
            x.par(n, [&](int32_t r) { if (!inv3_ldl(v.pD[cur] + 9 * r, v.Dinv + 9 * r)) s.fail = 1; });
            if (s.fail) return false;
            x.par(n, [&](int32_t r) { pcr_level(v, cur, level, d, r); });
            cur ^= 1; ++level;
        }
    x.par(n, [&](int32_t r) { if (!inv3_ldl(v.pD[cur] + 9 * r, v.Dinv + 9 * r)) s.fail = 1; });
    if (s.fail) return false;
    x.one([&]() { s.levels = level; });
    return true;
}

// The levels applied to src; what is left to do is Dinv times the buffer returned.
template <class X> __host__ __device__ const double* pcr_apply(X& x, const View& v, const State& s, const double* src) {
    const double* in = src;
    const int32_t levels = s.levels;
    for (int32_t l = 0; l < levels; ++l) {
        double* out = v.t[l & 1];
        const int32_t d = 1 << l;
        x.par(v.n, [&](int32_t r) { pcr_apply_level(v, l, d, in, out, r); });
        in = out;
    }
    return in;
}

// ---------------------------------------------------------------- the linear solve
// (H + lambda I) dx = -g by preconditioned conjugate gradients; false rejects the trial.  Sets s.budget_hit when the call's budget ends it.
template <class X> __host__ __device__ bool pcg(X& x, const View& v, const Prm& P, State& s, double lam) {
    const int32_t n = v.n;
    x.par(n, [&](int32_t r) { for (int m = 0; m < 3; ++m) { v.r[3 * r + m] = -v.g[3 * r + m]; v.dx[3 * r + m] = 0.0; } });
    const double* in = pcr_apply(x, v, s, v.r);
    double rz = x.sum(n, [&](int32_t r) {
        mv3(v.Dinv + 9 * r, in + 3 * r, v.z + 3 * r);
        for (int m = 0; m < 3; ++m) v.p[3 * r + m] = v.z[3 * r + m];
        return dot3(v.r + 3 * r, v.z + 3 * r);
    });
    const double rz0 = rz;
    const int32_t total = s.pcg_total;
    int32_t it = 0;
    bool ok = finite(rz) && rz >= 0.0, budget = false;
    while (ok) {
        if (rz <= P.pcg_tol2 * rz0 || it >= P.max_pcg) break;
        if (total + it >= P.budget) { budget = true; break; }
        const double pq = x.sum(n, [&](int32_t r) {
            hp_row(v, lam, r, v.q + 3 * r);
            return dot3(v.p + 3 * r, v.q + 3 * r);
        });
        if (!(pq > 0.0) || !finite(pq)) { ok = false; break; }
        const double a = rz / pq;
        x.par(n, [&](int32_t r) {
            for (int m = 0; m < 3; ++m) {
                v.dx[3 * r + m] = v.dx[3 * r + m] + a * v.p[3 * r + m];
                v.r[3 * r + m] = v.r[3 * r + m] - a * v.q[3 * r + m];
            }
        });
        in = pcr_apply(x, v, s, v.r);
        const double rzn = x.sum(n, [&](int32_t r) {
            mv3(v.Dinv + 9 * r, in + 3 * r, v.z + 3 * r);
            return dot3(v.r + 3 * r, v.z + 3 * r);
        });
        const double beta = rzn / rz;
        x.par(n, [&](int32_t r) { for (int m = 0; m < 3; ++m) v.p[3 * r + m] = v.z[3 * r + m] + beta * v.p[3 * r + m]; });
        rz = rzn; ++it;
    }
    x.one([&]() { s.pcg_it = it; s.pcg_total = total + it; s.budget_hit = budget ? 1 : 0; });
    return ok && !budget;
}

// ---------------------------------------------------------------- the control (as scanrefine::lm_decide)
PG_HD void lm_decide(State& s, const Prm& P, bool valid, double tcost, double scale, double* __restrict__ trace) {
    const double temp = (valid && finite(tcost)) ? tcost : kRejectedCost;
    double rho = -1.0;
    if (temp != kRejectedCost) {
        rho = (s.cost - temp) / (scale + 1e-3);
        if (!(rho > 0.0) && !(rho <= 0.0)) rho = -1.0;
    }
    const bool accepted = rho > 0.0;
    if (s.trials < kMaxTrials) {
        double* tr = trace + (int64_t)s.trials * kTraceItems;
        tr[0] = temp; tr[1] = s.lam; tr[2] = accepted ? 1.0 : 0.0; tr[3] = (double)s.pcg_it;
    }
    s.accepted = accepted ? 1 : 0;
    if (s.rot) s.rot_seen = 1;
    if (accepted) {
        const double u = 2.0 * rho - 1.0;
        double alpha = 1.0 - u * u * u;
        if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
        s.lambda *= (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
        s.nu = 2.0;
        s.before = s.cost;
        s.cost = tcost;
    } else {
        s.lambda *= s.nu;
        s.nu *= 2.0;
    }
    ++s.q; ++s.trials;
    const bool lam_ok = finite(s.lambda);
    if (!accepted && rho < 0.0 && s.q < kTrialsPerIteration && lam_ok) return;     // the next trial of this iteration
    ++s.it;
    if (s.q == kTrialsPerIteration || rho == 0.0 || !lam_ok) { s.done = 1; s.term = VISFS_POSE_GRAPH_NO_PROGRESS; }
    else if (P.ftol > 0.0 && s.before - s.cost <= P.ftol * s.before) { s.done = 1; s.term = VISFS_POSE_GRAPH_TOLERANCE; }
    else if (s.it >= P.max_it) { s.done = 1; s.term = VISFS_POSE_GRAPH_ITERATIONS; }
    // the loop ends for want of progress while the bound cut a trial of this iteration short: the caller moves the anchor and calls again
    if (s.done && s.term != VISFS_POSE_GRAPH_ITERATIONS && s.rot_seen) s.term = VISFS_POSE_GRAPH_ROTATION_BOUND;
    s.q = 0; s.rot_seen = 0;
}

template <class X> __host__ __device__ double linearize(X& x, const View& v) {
    const double cost = x.sum(v.E, [&](int32_t k) { return edge_linearize(v, k); });
    x.par(v.n, [&](int32_t r) { gather_row(v, r); });
    return cost;
}

// The whole call.  `s` is the executor's one State (LDS on the device).
template <class X> __host__ __device__ void run(X& x, const View& v, const Prm& P, State& s) {
    const int32_t n = v.n;
    x.one([&]() {
        s.cost = s.cost0 = s.before = 0.0; s.lambda = 0.0; s.nu = 2.0; s.lam = 0.0;
        s.q = s.it = s.trials = s.term = s.done = s.fail = s.rot = s.rot_seen = s.accepted = s.pcg_total = s.pcg_it = s.levels = s.budget_hit = 0;
        s.status = VISFS_BA_OK;
    });
    x.par(v.N, [&](int32_t i) { v.x[3 * i] = v.pose0[kPoseDoubles * i]; v.x[3 * i + 1] = v.pose0[kPoseDoubles * i + 1]; v.x[3 * i + 2] = 0.0; });
    const double cost0 = linearize(x, v);
    if (P.mode == kPrecondition) {
        const bool ok = pcr_setup(x, v, s, P.hook_lambda, P.precond);
        if (ok) {
            const double* in = pcr_apply(x, v, s, v.hook_r);
            x.par(n, [&](int32_t r) { mv3(v.Dinv + 9 * r, in + 3 * r, v.z + 3 * r); });
        }
        x.one([&]() { s.status = ok ? VISFS_BA_OK : VISFS_BA_ERR_SINGULAR; });
    } else if (P.mode == kOptimize) {
        const double top = x.maxv(n, [&](int32_t r) {
            double m = v.D[9 * r];
            if (v.D[9 * r + 4] > m) m = v.D[9 * r + 4];
            if (v.D[9 * r + 8] > m) m = v.D[9 * r + 8];
            return m;
        });
        x.one([&]() {
            s.cost = s.cost0 = s.before = cost0;
            s.lambda = 1e-5 * top; s.nu = 2.0;
            if (!finite(cost0)) { s.done = 1; s.term = VISFS_POSE_GRAPH_NO_PROGRESS; }
        });
        while (!s.done) {
            x.one([&]() { s.lam = s.lambda; s.rot = 0; s.pcg_it = 0; });
            const double lam = s.lam;
            bool ok = pcr_setup(x, v, s, lam, P.precond);
            if (ok) ok = pcg(x, v, P, s, lam);
            if (s.budget_hit) { x.one([&]() { s.done = 1; s.term = VISFS_POSE_GRAPH_PCG_BUDGET; }); break; }
            if (ok) {
                x.one([&]() { s.fail = 0; });
                x.par(v.N, [&](int32_t i) {
                    const int32_t r = v.row_of[i];
                    double a = v.x[3 * i], b = v.x[3 * i + 1], c = v.x[3 * i + 2];
                    if (r >= 0) {
                        a += v.dx[3 * r]; b += v.dx[3 * r + 1]; c += v.dx[3 * r + 2];
                        if (!finite(a) || !finite(b) || !finite(c)) s.fail = 1;
                        else if (c > VISFS_POSE_GRAPH_MAX_ROTATION || c < -VISFS_POSE_GRAPH_MAX_ROTATION) s.rot = 1;
                    }
                    v.xt[3 * i] = a; v.xt[3 * i + 1] = b; v.xt[3 * i + 2] = c;
                });
                ok = !s.fail && !s.rot;
            }
            double tcost = 0.0, scale = 0.0;
            if (ok) {
                tcost = x.sum(v.E, [&](int32_t k) { return edge_cost(v, v.xt, k); });
                scale = x.sum(n, [&](int32_t r) {
                    double a = 0.0;
                    for (int m = 0; m < 3; ++m) a += v.dx[3 * r + m] * (lam * v.dx[3 * r + m] + (-v.g[3 * r + m]));
                    return a;
                });
            }
            x.one([&]() { lm_decide(s, P, ok, tcost, scale, v.trace); });
            if (s.accepted) {
                x.par(v.N, [&](int32_t i) { for (int m = 0; m < 3; ++m) v.x[3 * i + m] = v.xt[3 * i + m]; });
                (void)linearize(x, v);
            }
        }
    }
    x.par(v.N, [&](int32_t i) {
        v.out_poses[3 * i] = v.x[3 * i]; v.out_poses[3 * i + 1] = v.x[3 * i + 1];
        v.out_poses[3 * i + 2] = v.pose0[kPoseDoubles * i + 2] + v.x[3 * i + 2];
    });
    x.par(v.E, [&](int32_t k) { v.out_chi2[k] = v.chi2[k]; });
    x.one([&]() {
        visfs_pose_graph_result& o = *v.res;
        o.status = s.status; o.iterations = s.it; o.trials = s.trials; o.termination = s.term; o.pcg_iterations = s.pcg_total;
        o.free_vertices = n;
        o.initial_cost = P.mode == kOptimize ? s.cost0 : cost0;
        o.final_cost = P.mode == kOptimize ? s.cost : cost0;
    });
}

// ---------------------------------------------------------------- the host plan (no HIP)
struct Plan {
    int32_t N = 0, E = 0, n = 0;
    std::vector<int32_t> row_of, inc_ptr, inc, chain_ptr, chain, eij;
    std::vector<double> pose0, ed;        // [N][5] with the cos and sin of the yaws, [E][10]
};

// The checks of a call and its lists.  Free vertices take the rows 0 .. n - 1 in vertex order; a row's incidence list holds its
// edges in increasing edge index; its chain list those that link it to row + 1.
inline bool host_finite(double v) { return v - v == 0.0; }

// positive semi-definite by the pivots of the symmetric elimination (LDL^T), to 1e-12 of the largest entry
inline bool information_ok(const double* W, const char** why) {
    double top = 0.0;
    for (int m = 0; m < 9; ++m) {
        if (!host_finite(W[m])) { *why = "an information matrix is not finite"; return false; }
        const double a = W[m] < 0.0 ? -W[m] : W[m];
        if (a > top) top = a;
    }
    const double tol = 1e-12 * top;
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            const double d = W[3 * i + j] - W[3 * j + i];
            if (d > tol || -d > tol) { *why = "an information matrix is not symmetric"; return false; }
        }
    double A[9];
    for (int m = 0; m < 9; ++m) A[m] = W[m];
    for (int k = 0; k < 3; ++k) {
        const double d = A[4 * k];
        if (d < -tol) { *why = "an information matrix is not positive semi-definite"; return false; }
        if (d <= tol) {                                                    // a zero pivot: its column must vanish with it
            for (int i = k + 1; i < 3; ++i) {
                const double a = A[3 * i + k] < 0.0 ? -A[3 * i + k] : A[3 * i + k];
                if (a > 1e-6 * top) { *why = "an information matrix is not positive semi-definite"; return false; }
            }
            continue;
        }
        for (int i = k + 1; i < 3; ++i) {
            const double l = A[3 * i + k] / d;
            for (int j = k + 1; j < 3; ++j) A[3 * i + j] -= l * A[3 * k + j];
        }
    }
    return true;
}

inline int make_plan(int32_t N, const double* poses, const uint8_t* fixed, int32_t E, const visfs_pose_graph_edge* edges, int32_t maxN, int32_t maxE,
                     Plan& pl, std::string& why) {
    if (N < 1 || E < 1) { why = "at least one vertex and one edge"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (N > maxN || N > VISFS_POSE_GRAPH_MAX_VERTICES) { why = "more vertices than the object was created for"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (E > maxE || E > VISFS_POSE_GRAPH_MAX_EDGES) { why = "more edges than the object was created for"; return VISFS_BA_ERR_UNSUPPORTED; }
    for (int64_t i = 0; i < 3 * (int64_t)N; ++i) if (!host_finite(poses[i])) { why = "a pose is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    pl.N = N; pl.E = E;
    pl.row_of.assign((size_t)N, -1);
    int32_t n = 0;
    for (int32_t i = 0; i < N; ++i) if (!fixed[i]) pl.row_of[(size_t)i] = n++;
    pl.n = n;
    if (n == N) { why = "no vertex is fixed"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    std::vector<int32_t> count((size_t)n + 1, 0), ccount((size_t)n + 1, 0);
    for (int32_t k = 0; k < E; ++k) {
        const visfs_pose_graph_edge& e = edges[k];
        if (e.i < 0 || e.j < 0 || e.i >= N || e.j >= N || e.i == e.j) { why = "an edge's vertices are out of range or equal"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        for (int m = 0; m < 3; ++m) if (!host_finite(e.z[m])) { why = "a measurement is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        const char* text = "";
        if (!information_ok(e.information, &text)) { why = text; return VISFS_BA_ERR_BAD_ARGUMENT; }
        if (!host_finite(e.huber_delta) || e.huber_delta < 0.0) { why = "huber_delta must be finite and not negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        const int32_t ri = pl.row_of[(size_t)e.i], rj = pl.row_of[(size_t)e.j];
        if (ri >= 0) ++count[(size_t)ri];
        if (rj >= 0) ++count[(size_t)rj];
        if (ri >= 0 && rj >= 0 && (rj == ri + 1 || ri == rj + 1)) ++ccount[(size_t)(ri < rj ? ri : rj)];
    }
    for (int32_t r = 0; r < n; ++r) if (count[(size_t)r] == 0) { why = "a free vertex has no edge"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    pl.inc_ptr.assign((size_t)n + 1, 0); pl.chain_ptr.assign((size_t)n + 1, 0);
    for (int32_t r = 0; r < n; ++r) {
        pl.inc_ptr[(size_t)r + 1] = pl.inc_ptr[(size_t)r] + count[(size_t)r];
        pl.chain_ptr[(size_t)r + 1] = pl.chain_ptr[(size_t)r] + ccount[(size_t)r];
    }
    pl.inc.assign((size_t)pl.inc_ptr[(size_t)n], 0); pl.chain.assign((size_t)pl.chain_ptr[(size_t)n], 0);
    std::vector<int32_t> at(pl.inc_ptr.begin(), pl.inc_ptr.end() - 1), cat(pl.chain_ptr.begin(), pl.chain_ptr.end() - 1);
    pl.eij.resize(2 * (size_t)E); pl.ed.resize((size_t)kEdgeDoubles * E);
    for (int32_t k = 0; k < E; ++k) {                                       // increasing edge index: every list comes out sorted
        const visfs_pose_graph_edge& e = edges[k];
        const int32_t ri = pl.row_of[(size_t)e.i], rj = pl.row_of[(size_t)e.j];
        if (ri >= 0) pl.inc[(size_t)at[(size_t)ri]++] = 2 * k;
        if (rj >= 0) pl.inc[(size_t)at[(size_t)rj]++] = 2 * k + 1;
        if (ri >= 0 && rj >= 0) {
            if (rj == ri + 1) pl.chain[(size_t)cat[(size_t)ri]++] = 2 * k;
            else if (ri == rj + 1) pl.chain[(size_t)cat[(size_t)rj]++] = 2 * k + 1;
        }
        pl.eij[2 * (size_t)k] = e.i; pl.eij[2 * (size_t)k + 1] = e.j;
        double* d = pl.ed.data() + (size_t)kEdgeDoubles * k;
        const double* W = e.information;
        d[0] = e.z[0]; d[1] = e.z[1]; d[2] = e.z[2];
        d[3] = W[0]; d[4] = W[1]; d[5] = W[2]; d[6] = W[4]; d[7] = W[5]; d[8] = W[8];
        d[9] = e.huber_delta;
    }
    pl.pose0.resize((size_t)kPoseDoubles * N);
    for (int32_t i = 0; i < N; ++i) {
        double* p = pl.pose0.data() + (size_t)kPoseDoubles * i;
        p[0] = poses[3 * i]; p[1] = poses[3 * i + 1]; p[2] = poses[3 * i + 2];
        p[3] = std::cos(p[2]); p[4] = std::sin(p[2]);
    }
    return VISFS_BA_OK;
}

}  // namespace posegraph
