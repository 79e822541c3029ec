// Sub-cell refinement of a scan's pose (include/visfs_scan_refine.h): what the kernel of ba_scan_refine.hip and
// the one-core twin share, and what the group call (ba_scan_group.hip) needs to launch it.
//
// The device and the twin agree byte for byte because every double is formed by the same + - * / in the same order: this header is
// included after `#pragma clang fp contract(off)` and before anything else that includes ba_math.hpp, so the inline functions of
// both compile without contraction in both passes; the only transcendentals (cos and sin of the initial yaw) come from the host,
// the rotation by yaw - initial yaw from one Horner polynomial below; the sums are formed per lane and added by a fixed tree.
#pragma once
#pragma clang fp contract(off)

#include "ba_math.hpp"
#include "ba_scan_stack.hpp"
#include "../../include/visfs_scan_refine.h"

namespace scanrefine {

constexpr int kRefineLanes = VISFS_SCAN_REFINE_LANES;   // the workgroup size: results depend on it (the reduction order)
constexpr int kSums = 10;                               // six of J^T J (00 01 02 11 12 22), three of J^T e, one of e^2
constexpr int kMaxTrials = VISFS_SCAN_REFINE_MAX_TRIALS;
constexpr int kTrialsPerIteration = 10;
constexpr int kTraceItems = 6;                          // cost, lambda, accepted, x, y, delta
constexpr double kRejectedCost = 1.7976931348623157e308;

// Level 0 of what is refined against: the limits' cell counts, the allocation [ay][ax] and where the limits' cell (0, 0) lies in
// it (submap::GridView).  gain = 1: the cells are a stack's P_0 (scan::cell_gain), 0: a sub-map's values.
struct Grid {
    const uint16_t* cells = nullptr;
    int32_t nx = 0, ny = 0, ax = 0, ay = 0, ox = 0, oy = 0, gain = 0;
};

// Grid2D's value -> correspondence cost as getCorrespondenceCost returns it (ba_submap.hip: Tables::cost_f), without a table:
// value 0 (unknown) is the maximal cost.
__host__ __device__ inline float value_cost(int32_t v) {
    if (v == 0) return (float)submap::kMaxCorrespondenceCost;
    const double k = (submap::kMaxCorrespondenceCost - submap::kMinCorrespondenceCost) / 32766.0;
    return (float)((double)v * k + (submap::kMinCorrespondenceCost - k));
}

// GridArrayAdapter::GetValue (visfs_ba::grid_value) on the cells: outside the limits the constant, inside the float cost widened;
// a cell inside the limits that the allocation does not hold yet is unknown.  Found by visfs_ba::bicubic through its argument.
__host__ __device__ inline double grid_value(const Grid& g, int row, int col) {
    const int y = row - visfs_ba::kGridPadding, x = col - visfs_ba::kGridPadding;
    if (y < 0 || x < 0 || y >= g.ny || x >= g.nx) return visfs_ba::kMaxCorrespondenceCost;
    const int32_t px = x - g.ox, py = y - g.oy;
    int32_t v = 0;
    if (px >= 0 && py >= 0 && px < g.ax && py < g.ay) v = g.cells[(int64_t)py * g.ax + px];
    if (g.gain) v = v == 0 ? 0 : scan::kMaxValue - v;
    else v &= scan::kMaxValue;
    return (double)value_cost(v);
}

// sin and cos of d, |d| <= 1: the Taylor terms through d^21 (the first one left out is below 2^-70)
__host__ __device__ inline void sincos_poly(double d, double& s, double& c) {
    const double z = d * d;
    double p = 1.0 / 51090942171709440000.0;                                // 1 / 21!
    p = -1.0 / 121645100408832000.0 + z * p;                                // 19!
    p = 1.0 / 355687428096000.0 + z * p;                                    // 17!
    p = -1.0 / 1307674368000.0 + z * p;                                     // 15!
    p = 1.0 / 6227020800.0 + z * p;                                         // 13!
    p = -1.0 / 39916800.0 + z * p;                                          // 11!
    p = 1.0 / 362880.0 + z * p;                                             // 9!
    p = -1.0 / 5040.0 + z * p;
    p = 1.0 / 120.0 + z * p;
    p = -1.0 / 6.0 + z * p;
    p = 1.0 + z * p;
    s = d * p;
    double q = 1.0 / 2432902008176640000.0;                                 // 1 / 20!
    q = -1.0 / 6402373705728000.0 + z * q;                                  // 18!
    q = 1.0 / 20922789888000.0 + z * q;                                     // 16!
    q = -1.0 / 87178291200.0 + z * q;                                       // 14!
    q = 1.0 / 479001600.0 + z * q;                                          // 12!
    q = -1.0 / 3628800.0 + z * q;                                           // 10!
    q = 1.0 / 40320.0 + z * q;
    q = -1.0 / 720.0 + z * q;
    q = 1.0 / 24.0 + z * q;
    q = -1.0 / 2.0 + z * q;
    c = 1.0 + z * q;
}

__host__ __device__ inline bool finite(double v) { return (v - v) == 0.0; }

// what every member of a call shares
struct Prm {
    double s = 0.0;                           // occupied_space_weight / sqrt(n)
    double wt = 0.0, wr = 0.0, ftol = 0.0;
    int32_t max_it = 0, n = 0;
};

// One pose to refine, as the kernel reads it at blockIdx.x.  from_match = 0: the start and the target stand here.  from_match = 1
// (the group call): they are formed from the member's match record where the match left it: skipped when it overflowed or its
// score lies below min_score, else the winner as scan::fill_result forms it, its rotation from the match's table, the guess as
// target.
struct Job {
    Grid g;
    int32_t from_match = 0, na = 0, nl = 0, S = 0;
    double res = 0.0, max_x = 0.0, max_y = 0.0;
    double x0 = 0.0, y0 = 0.0, yaw0 = 0.0, c0 = 1.0, s0 = 0.0, tx = 0.0, ty = 0.0;
    double gx = 0.0, gy = 0.0, gyaw = 0.0, step = 0.0, min_score = 0.0;
    const scanfast::Ctrl* ctrl = nullptr;
    const double* rot = nullptr;              // [S][2]
};

// Return (px, py) at the pose (x, y) with rotation (C, S): its residual and Jacobian row added to the lane's ten sums.
__host__ __device__ inline void add_return(const Grid& g, double res, double max_x, double max_y, double s, double C, double S, double x, double y,
                                           double px, double py, double a[kSums]) {
    const double Xr = C * px - S * py, Yr = S * px + C * py;
    const double X = Xr + x, Y = Yr + y;
    double r = (max_x - X) / res - 0.5 + (double)visfs_ba::kGridPadding;     // laser_grid_coords
    double c = (max_y - Y) / res - 0.5 + (double)visfs_ba::kGridPadding;
    // beyond four cells off the limits every sample is the constant: held there, so that the interpolator's integers stay in range
    const double lo = (double)(visfs_ba::kGridPadding - 4);
    const double rhi = (double)(visfs_ba::kGridPadding + 4) + (double)g.ny, chi = (double)(visfs_ba::kGridPadding + 4) + (double)g.nx;
    if (r < lo) r = lo;
    if (r > rhi) r = rhi;
    if (c < lo) c = lo;
    if (c > chi) c = chi;
    double f, dfdr, dfdc;
    visfs_ba::bicubic(g, r, c, f, dfdr, dfdc);
    const double e = s * f;
    const double gr = (s * dfdr) / res, gc = (s * dfdc) / res;              // dr/dX = dc/dY = -1 / res
    const double j0 = -gr, j1 = -gc, j2 = gr * Yr - gc * Xr;                 // dX/dyaw = -Yr, dY/dyaw = Xr
    a[0] += j0 * j0; a[1] += j0 * j1; a[2] += j0 * j2; a[3] += j1 * j1; a[4] += j1 * j2; a[5] += j2 * j2;
    a[6] += j0 * e; a[7] += j1 * e; a[8] += j2 * e;
    a[9] += e * e;
}

// Lane t's sums over the returns t, t + kRefineLanes, ... in increasing order, at the pose (x, y, yaw0 + d)
__host__ __device__ inline void lane_sums(const Job& J, const Prm& P, const double* __restrict__ pts, double c0, double s0, double x, double y, double d,
                                          int32_t t, double a[kSums]) {
    double sd, cd;
    sincos_poly(d, sd, cd);
    const double C = c0 * cd - s0 * sd, S = s0 * cd + c0 * sd;
    for (int k = 0; k < kSums; ++k) a[k] = 0.0;
    for (int32_t i = t; i < P.n; i += kRefineLanes) add_return(J.g, J.res, J.max_x, J.max_y, P.s, C, S, x, y, pts[2 * i], pts[2 * i + 1], a);
}

// The Levenberg-Marquardt control of SURVEY section 3.4 on the 3 x 3 system, as one state machine that work item 0 and the twin
// both step: `advance` takes the ten sums at the pose (ex, ey, ed) it asked for and either asks for the next pose or is done.
struct Lm {
    double x, y, d;                           // the pose in force (d = yaw - initial yaw)
    double H[6], g[3], cost;                  // J^T J, J^T e and e^2 there, the priors included
    double lambda, nu, cost0, before;
    double ex, ey, ed;                        // the pose to evaluate
    double dx[3], lam;                        // the step that gave it, and its lambda
    double c0, s0, yaw0, tx, ty;
    int32_t phase, q, it, trials, term, done, run, status;
};

// (H + lambda I) dx = -g by LDL^T; false when a pivot is not positive or the step is not finite
__host__ __device__ inline bool solve3(const double H[6], const double g[3], double lambda, double dx[3]) {
    const double a00 = H[0] + lambda, a01 = H[1], a02 = H[2], a11 = H[3] + lambda, a12 = H[4], a22 = H[5] + lambda;
    const double d0 = a00;
    if (!(d0 > 0.0)) return false;
    const double l10 = a01 / d0, l20 = a02 / d0;
    const double d1 = a11 - l10 * a01;
    if (!(d1 > 0.0)) return false;
    const double u12 = a12 - l20 * a01;
    const double l21 = u12 / d1;
    const double d2 = (a22 - l20 * a02) - l21 * u12;
    if (!(d2 > 0.0)) return false;
    const double b0 = -g[0], b1 = -g[1], b2 = -g[2];
    const double z0 = b0, z1 = b1 - l10 * z0, z2 = (b2 - l20 * z0) - l21 * z1;
    const double w2 = z2 / d2;
    const double w1 = z1 / d1 - l21 * w2;
    const double w0 = (z0 / d0 - l10 * w1) - l20 * w2;
    dx[0] = w0; dx[1] = w1; dx[2] = w2;
    return finite(w0) && finite(w1) && finite(w2);
}

// The trial about to be judged: rejected (valid = false: no sums), or evaluated with the system T.
__host__ __device__ inline void lm_decide(Lm& m, const Prm& P, bool valid, const double TH[6], const double Tg[3], double Tcost, double* __restrict__ trace) {
    const double temp = (valid && finite(Tcost)) ? Tcost : kRejectedCost;
    double rho = -1.0;
    if (temp != kRejectedCost) {
        double scale = 0.0;
        for (int k = 0; k < 3; ++k) scale += m.dx[k] * (m.lam * m.dx[k] + (-m.g[k]));
        scale += 1e-3;
        rho = (m.cost - temp) / scale;
        if (!(rho > 0.0) && !(rho <= 0.0)) rho = -1.0;
    }
    const bool accepted = rho > 0.0;
    if (m.trials < kMaxTrials) {
        double* tr = trace + (int64_t)m.trials * kTraceItems;
        tr[0] = temp; tr[1] = m.lam; tr[2] = accepted ? 1.0 : 0.0; tr[3] = m.ex; tr[4] = m.ey; tr[5] = m.ed;
    }
    if (accepted) {
        const double u = 2.0 * rho - 1.0;
        double alpha = 1.0 - u * u * u;
        if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
        m.lambda *= (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
        m.nu = 2.0;
        m.before = m.cost;
        m.x = m.ex; m.y = m.ey; m.d = m.ed;
        for (int k = 0; k < 6; ++k) m.H[k] = TH[k];
        for (int k = 0; k < 3; ++k) m.g[k] = Tg[k];
        m.cost = Tcost;
    } else {
        m.lambda *= m.nu;
        m.nu *= 2.0;
    }
    ++m.q; ++m.trials;
    const bool lam_ok = finite(m.lambda);
    if (!accepted && rho < 0.0 && m.q < kTrialsPerIteration && lam_ok) return;     // the next trial of this iteration
    ++m.it;
    if (m.q == kTrialsPerIteration || rho == 0.0 || !lam_ok) { m.done = 1; m.term = VISFS_SCAN_REFINE_NO_PROGRESS; }
    else if (P.ftol > 0.0 && m.before - m.cost <= P.ftol * m.before) { m.done = 1; m.term = VISFS_SCAN_REFINE_TOLERANCE; }
    else if (m.it >= P.max_it) { m.done = 1; m.term = VISFS_SCAN_REFINE_ITERATIONS; }
    m.q = 0;
}

__host__ __device__ inline void lm_advance(Lm& m, const Prm& P, const double sums[kSums], double* __restrict__ trace) {
    // the priors join the reduced sums: translation towards the target, rotation towards the initial yaw
    double H[6], g[3], cost;
    for (int k = 0; k < 6; ++k) H[k] = sums[k];
    for (int k = 0; k < 3; ++k) g[k] = sums[6 + k];
    const double e0 = P.wt * (m.ex - m.tx), e1 = P.wt * (m.ey - m.ty), e2 = P.wr * m.ed;
    H[0] += P.wt * P.wt; H[3] += P.wt * P.wt; H[5] += P.wr * P.wr;
    g[0] += P.wt * e0; g[1] += P.wt * e1; g[2] += P.wr * e2;
    cost = ((sums[9] + e0 * e0) + e1 * e1) + e2 * e2;
    if (m.phase == 0) {
        m.phase = 1;
        m.x = m.ex; m.y = m.ey; m.d = m.ed;
        for (int k = 0; k < 6; ++k) m.H[k] = H[k];
        for (int k = 0; k < 3; ++k) m.g[k] = g[k];
        m.cost = m.cost0 = m.before = cost;
        double top = H[0];
        if (H[3] > top) top = H[3];
        if (H[5] > top) top = H[5];
        m.lambda = 1e-5 * top; m.nu = 2.0;
        if (!finite(cost)) { m.done = 1; m.term = VISFS_SCAN_REFINE_NO_PROGRESS; }
    } else lm_decide(m, P, true, H, g, cost, trace);
    while (!m.done) {
        m.lam = m.lambda;
        bool ok = solve3(m.H, m.g, m.lam, m.dx);
        if (ok) {
            m.ex = m.x + m.dx[0]; m.ey = m.y + m.dx[1]; m.ed = m.d + m.dx[2];
            ok = finite(m.ex) && finite(m.ey) && m.ed <= VISFS_SCAN_REFINE_MAX_ROTATION && m.ed >= -VISFS_SCAN_REFINE_MAX_ROTATION;
        } else { m.dx[0] = m.dx[1] = m.dx[2] = 0.0; m.ex = m.x; m.ey = m.y; m.ed = m.d; }
        if (ok) return;                                                    // to be evaluated
        lm_decide(m, P, false, H, g, cost, trace);
    }
}

// The start of one job: false when there is nothing to refine (a skipped member; `status` says whether it overflowed).
__host__ __device__ inline bool lm_start(const Job& J, const Prm& P, Lm& m) {
    m.phase = 0; m.q = 0; m.it = 0; m.trials = 0; m.term = 0; m.done = 0; m.run = 1; m.status = VISFS_BA_OK;
    m.lambda = 0.0; m.nu = 2.0; m.cost = m.cost0 = m.before = 0.0; m.lam = 0.0;
    m.dx[0] = m.dx[1] = m.dx[2] = 0.0;
    if (!J.from_match) {
        m.ex = J.x0; m.ey = J.y0; m.yaw0 = J.yaw0; m.c0 = J.c0; m.s0 = J.s0; m.tx = J.tx; m.ty = J.ty;
    } else {
        const scanfast::Ctrl c = *J.ctrl;
        const int32_t L = 2 * J.nl + 1;
        m.ex = J.gx; m.ey = J.gy; m.yaw0 = J.gyaw; m.c0 = 1.0; m.s0 = 0.0; m.tx = J.gx; m.ty = J.gy;
        if (c.overflow) { m.run = 0; m.status = VISFS_BA_ERR_UNSUPPORTED; }
        else if (c.best_index < 0 || (int64_t)c.best_index >= (int64_t)J.S * L * L) { m.run = 0; m.status = VISFS_BA_ERR_DEVICE; }
        else {
            const int32_t k = c.best_index / (L * L), xo = (c.best_index / L) % L - J.nl, yo = c.best_index % L - J.nl;
            m.ex = J.gx + (double)(-yo) * J.res;                           // scan::fill_result
            m.ey = J.gy + (double)(-xo) * J.res;
            m.yaw0 = J.gyaw + (double)(k - J.na) * J.step;
            m.c0 = J.rot[2 * k]; m.s0 = J.rot[2 * k + 1];
            if (!(scan::candidate_score(c.best_sum, P.n, 1.0) >= J.min_score)) m.run = 0;
        }
    }
    m.ed = 0.0;
    m.x = m.ex; m.y = m.ey; m.d = 0.0;
    for (int k = 0; k < 6; ++k) m.H[k] = 0.0;
    for (int k = 0; k < 3; ++k) m.g[k] = 0.0;
    return m.run != 0;
}

__host__ __device__ inline void lm_result(const Lm& m, visfs_scan_refine_result& r) {
    r.status = m.status; r.refined = m.run; r.iterations = m.it; r.trials = m.trials; r.termination = m.term; r.reserved = 0;
    r.x = m.x; r.y = m.y; r.yaw = m.yaw0 + m.d;
    r.initial_cost = m.cost0; r.final_cost = m.cost;
    r.information[0] = m.H[0]; r.information[1] = m.H[1]; r.information[2] = m.H[2];
    r.information[3] = m.H[1]; r.information[4] = m.H[3]; r.information[5] = m.H[4];
    r.information[6] = m.H[2]; r.information[7] = m.H[4]; r.information[8] = m.H[5];
}

// ---------------------------------------------------------------- host side (defined in ba_scan_refine.hip)

// The argument checks of a call in the order the entry points make them (the pointers and n >= 0 already checked).
int check_call(const visfs_scan_refine_params& p, const double initial[3], const double target[2], int32_t n, const double* xyz, const char** why);
Prm make_prm(const visfs_scan_refine_params& p, int32_t n);
// the job of a refinement on level 0 of a stack from a given start
Job stack_job(const visfs_scan_stack* st, const double initial[3], const double target[2]);
// the record of a call that refined nothing: the start back
void not_refined(int32_t status, double x, double y, double yaw, visfs_scan_refine_result* out);
// The one-core twin: the kernel's schedule on host memory.  pts [n][2]; trace: room for kMaxTrials * kTraceItems doubles.
void host_refine(const Job& J, const Prm& P, const double* pts, visfs_scan_refine_result* out, double* trace);
// k_scan_refine on `stream`: jobs[m], pts [n][2], out[m] and trace[m][kMaxTrials][kTraceItems] in device memory.  Returns the
// launch's hipError_t as an int.
int launch_refine(hipStream_t stream, int32_t m, const Job* d_jobs, const Prm& P, const double* d_pts, visfs_scan_refine_result* d_out, double* d_trace);

// the refinement's buffers on a stack (visfs_scan_stack::refine) or a sub-maps object
struct State;
void state_free(State* s);

}  // namespace scanrefine
