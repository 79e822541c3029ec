// ba_pnp.hpp — the arithmetic of the PnP-RANSAC pose guess (include/visfs_pnp.h), shared by the HIP kernels of ba_pnp.hip and the
// one-core host twin: the counter-hash sampler, the P3P solver (Grunert's quartic, Ferrari's resolvent with a fixed number of
// bisections and Newton steps), the reprojection error, the Levenberg-Marquardt refit and the refinement loop of solvePnPRansac
// (corelib/src/MultiviewGeometry.cpp:241-313).  DESIGN.md section 9e states every step.
//
// Everything is + - * / sqrt in a fixed order with contraction off, so the device and the twin produce the same bits.  The control
// flow of the refit and of the refinement loop is written once, over a policy that supplies the reductions: on the device every
// thread of the workgroup runs it with the same values, on the host one thread does.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#pragma clang fp contract(off)

#include "ba_math.hpp"

namespace pnp {

using visfs_ba::Mat3;
using visfs_ba::Quat;
using visfs_ba::Rt;
using visfs_ba::Vec3;

constexpr int kMaxPoints = 4096;       // rows of a call
constexpr int kMaxHypotheses = 4096;
constexpr int kMaxRefine = 32;         // refinement passes recorded for visfs_pnp_download
constexpr int kSlots = 256;            // leaves of the summation tree (part of the definition, not of the launch shape)
constexpr int kRefitIterations = 20;
constexpr int kCubicBisections = 80;
constexpr int kQuarticPolishSteps = 8;
constexpr double kCollinearSin2 = 1e-8;    // a sample whose world triad has sin^2(angle at the first point) below this is invalid
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-9, kLambdaMax = 1e12, kStepStop = 1e-10;

struct Cam { double fx, fy, cx, cy; };
struct Row { float X, Y, Z, u, v; };       // one correspondence: the 3-D word of the frame before, its pixel in this frame

// What the refine stage leaves behind (one block of the copy out; the inlier list follows it).
struct Result {
    int32_t winner;            // hypothesis index, -1: no valid hypothesis
    int32_t winner_count;
    int32_t n_passes;
    int32_t n_inliers;
    double refit0[7];          // the refit on the winner's inliers (step 5), t then q
    double tq[7];              // the model after the refinement loop
};

// ---- step 2: the sampler ----------------------------------------------------------------------------------------------------------
BA_HD uint64_t mix64(uint64_t z) {     // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
BA_HD void sample4(uint64_t seed, int32_t h, int32_t m, int32_t s[4]) {
    int32_t a = 0, b = 0, c = 0;       // the rows taken so far, ascending
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t r = mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(4 * (int64_t)h + k + 1));
        int32_t j = (int32_t)(r % (uint64_t)(m - k));
        if (k > 0 && j >= a) ++j;
        if (k > 1 && j >= b) ++j;
        if (k > 2 && j >= c) ++j;
        s[k] = j;
        if (k == 0) a = j;
        else if (k == 1) { if (j < a) { b = a; a = j; } else b = j; }
        else if (k == 2) { if (j < a) { c = b; b = a; a = j; } else if (j < b) { c = b; b = j; } else c = j; }
    }
}

// ---- small vectors ----------------------------------------------------------------------------------------------------------------
BA_HD Vec3 vsub(const Vec3& a, const Vec3& b) { return Vec3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
BA_HD double vdot(const Vec3& a, const Vec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
BA_HD Vec3 vcross(const Vec3& a, const Vec3& b) { return Vec3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
BA_HD Vec3 vscale(const Vec3& a, double s) { return Vec3{ a.x * s, a.y * s, a.z * s }; }
BA_HD Vec3 bearing(const Cam& K, float u, float v) {
    const double x = ((double)u - K.cx) / K.fx, y = ((double)v - K.cy) / K.fy;
    const double n = sqrt(x * x + y * y + 1.0);
    return Vec3{ x / n, y / n, 1.0 / n };
}

// ---- step 4: the reprojection error of one row (cv::projectPoints without distortion, then computeReprojErrors' float norm) ------
BA_HD void project(const Rt& T, const Cam& K, const Row& r, double& pu, double& pv) {
    const Vec3 pc = visfs_ba::mat_vec(T.R, Vec3{ (double)r.X, (double)r.Y, (double)r.Z });
    const double x = pc.x + T.t.x, y = pc.y + T.t.y, z = pc.z + T.t.z;
    const double iz = z != 0.0 ? 1.0 / z : 1.0;
    pu = K.fx * (x * iz) + K.cx;
    pv = K.fy * (y * iz) + K.cy;
}
BA_HD float reproj_error(const Rt& T, const Cam& K, const Row& r) {
    double pu, pv;
    project(T, K, r, pu, pv);
    const double dx = (double)r.u - pu, dy = (double)r.v - pv;
    return (float)sqrt(dx * dx + dy * dy);
}

// ---- step 3: P3P ------------------------------------------------------------------------------------------------------------------
// An orthonormal frame on a triad: e1 along a->b, e3 normal to the plane, e2 = e3 x e1.  sin2: sin^2 of the angle at a.
BA_HD void triad_frame(const Vec3& a, const Vec3& b, const Vec3& c, Vec3& e1, Vec3& e2, Vec3& e3, double& sin2) {
    const Vec3 d1 = vsub(b, a), d2 = vsub(c, a);
    const double n1 = sqrt(vdot(d1, d1));
    e1 = vscale(d1, 1.0 / n1);
    const Vec3 x = vcross(e1, d2);
    const double x2 = vdot(x, x);
    sin2 = x2 / vdot(d2, d2);
    e3 = vscale(x, 1.0 / sqrt(x2));
    e2 = vcross(e3, e1);
}

// The best of the up-to-four P3P poses of rows r0..r2, judged on r3.  Returns false when no solution has three positive depths.
BA_HD bool p3p_solve(const Cam& K, const Row& r0, const Row& r1, const Row& r2, const Row& r3, Rt& best) {
    const Vec3 P1{ (double)r0.X, (double)r0.Y, (double)r0.Z }, P2{ (double)r1.X, (double)r1.Y, (double)r1.Z }, P3{ (double)r2.X, (double)r2.Y, (double)r2.Z };
    const Vec3 j1 = bearing(K, r0.u, r0.v), j2 = bearing(K, r1.u, r1.v), j3 = bearing(K, r2.u, r2.v);
    double best_err = __builtin_huge_val();
    bool found = false;
    Vec3 e1, e2, e3;
    double sin2;
    triad_frame(P1, P2, P3, e1, e2, e3, sin2);
    if (!(sin2 >= kCollinearSin2)) return false;
    // Grunert: s2 = u s1, s3 = v s1 with the law of cosines on the three sides.
    const Vec3 d23 = vsub(P2, P3), d13 = vsub(P1, P3), d12 = vsub(P1, P2);
    const double a2 = vdot(d23, d23), b2 = vdot(d13, d13), c2 = vdot(d12, d12);
    const double ca = vdot(j2, j3), cb = vdot(j1, j3), cg = vdot(j1, j2);
    // u = N(v) / D(v): N = n2 v^2 + n1 v + n0, D = d1 v + d0
    const double k = a2 - c2;
    const double n2 = k - b2, n1 = -2.0 * k * cb, n0 = k + b2;
    const double d1 = -2.0 * b2 * ca, d0 = 2.0 * b2 * cg;
    // b2 (D^2 + N^2 - 2 cg N D) - c2 (v^2 - 2 cb v + 1) D^2 = 0
    const double D2 = d1 * d1, D1 = 2.0 * d1 * d0, D0 = d0 * d0;
    const double N4 = n2 * n2, N3 = 2.0 * n2 * n1, N2 = 2.0 * n2 * n0 + n1 * n1, N1 = 2.0 * n1 * n0, N0 = n0 * n0;
    const double M3 = n2 * d1, M2 = n2 * d0 + n1 * d1, M1 = n1 * d0 + n0 * d1, M0 = n0 * d0;
    const double Q4 = D2, Q3 = D1 - 2.0 * cb * D2, Q2 = D0 - 2.0 * cb * D1 + D2, Q1 = D1 - 2.0 * cb * D0, Q0 = D0;
    const double c4 = b2 * N4 - c2 * Q4;
    const double c3 = b2 * (N3 - 2.0 * cg * M3) - c2 * Q3;
    const double c2q = b2 * (D2 + N2 - 2.0 * cg * M2) - c2 * Q2;
    const double c1 = b2 * (D1 + N1 - 2.0 * cg * M1) - c2 * Q1;
    const double c0 = b2 * (D0 + N0 - 2.0 * cg * M0) - c2 * Q0;
    // Ferrari on the monic quartic x^4 + A x^3 + B x^2 + C x + E
    const double A = c3 / c4, B = c2q / c4, C = c1 / c4, E = c0 / c4;
    const double A2 = A * A;
    const double p = B - 0.375 * A2;
    const double q = C - 0.5 * A * B + 0.125 * A2 * A;
    const double r = E - 0.25 * A * C + 0.0625 * A2 * B - (3.0 / 256.0) * A2 * A2;
    // the resolvent f(m) = m^3 + p m^2 + (p^2/4 - r) m - q^2/8: f(0) <= 0 and f is positive at the Cauchy bound, so a positive root is
    // bracketed; a fixed number of bisections takes it to the last bit (Newton from the bound stalls when a complex pair lies to the
    // right of the real root)
    const double k1 = 0.25 * p * p - r, k0 = -0.125 * q * q;
    double bound = fabs(p);
    if (fabs(k1) > bound) bound = fabs(k1);
    if (fabs(k0) > bound) bound = fabs(k0);
    double lo = 0.0, hi = 1.0 + bound;
    for (int it = 0; it < kCubicBisections; ++it) {
        const double mid = 0.5 * (lo + hi);
        const double f = ((mid + p) * mid + k1) * mid + k0;
        if (f > 0.0) hi = mid; else lo = mid;
    }
    const double mm = hi;
    const double s = sqrt(2.0 * mm);
    const double hq = q / (2.0 * s), base = 0.5 * p + mm;
    const double disc_a = s * s - 4.0 * (base + hq), disc_b = s * s - 4.0 * (base - hq);
    const double ra = sqrt(disc_a), rb = sqrt(disc_b);          // NaN for a complex pair: every test below fails on it
    const double y[4] = { 0.5 * (s + ra), 0.5 * (s - ra), 0.5 * (-s + rb), 0.5 * (-s - rb) };
    const Vec3 u1 = j1, u2 = j2, u3 = j3;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double v = y[i] - 0.25 * A;
        for (int it = 0; it < kQuarticPolishSteps; ++it) {
            const double f = (((v + A) * v + B) * v + C) * v + E;
            const double df = ((4.0 * v + 3.0 * A) * v + 2.0 * B) * v + C;
            v = v - f / df;
        }
        const double u = ((n2 * v + n1) * v + n0) / (d1 * v + d0);
        const double s1 = sqrt(b2 / ((v - 2.0 * cb) * v + 1.0));
        const double s2 = u * s1, s3 = v * s1;
        if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
        Vec3 f1, f2, f3;
        double fs2;
        const Vec3 X1 = vscale(u1, s1);
        triad_frame(X1, vscale(u2, s2), vscale(u3, s3), f1, f2, f3, fs2);
        Rt T;                                                    // R e_k = f_k
        T.R.m00 = f1.x * e1.x + f2.x * e2.x + f3.x * e3.x; T.R.m01 = f1.x * e1.y + f2.x * e2.y + f3.x * e3.y; T.R.m02 = f1.x * e1.z + f2.x * e2.z + f3.x * e3.z;
        T.R.m10 = f1.y * e1.x + f2.y * e2.x + f3.y * e3.x; T.R.m11 = f1.y * e1.y + f2.y * e2.y + f3.y * e3.y; T.R.m12 = f1.y * e1.z + f2.y * e2.z + f3.y * e3.z;
        T.R.m20 = f1.z * e1.x + f2.z * e2.x + f3.z * e3.x; T.R.m21 = f1.z * e1.y + f2.z * e2.y + f3.z * e3.y; T.R.m22 = f1.z * e1.z + f2.z * e2.z + f3.z * e3.z;
        const Vec3 RP = visfs_ba::mat_vec(T.R, P1);
        T.t = vsub(X1, RP);
        double pu, pv;
        project(T, K, r3, pu, pv);
        const double dx = (double)r3.u - pu, dy = (double)r3.v - pv;
        const double err = sqrt(dx * dx + dy * dy);
        if (err < best_err) { best_err = err; best = T; found = true; }
    }
    return found;
}

BA_HD void rt_to_tq(const Rt& T, double tq[7]) {
    const Quat q = visfs_ba::quat_positify(visfs_ba::R_to_quat(T.R));
    tq[0] = T.t.x; tq[1] = T.t.y; tq[2] = T.t.z; tq[3] = q.x; tq[4] = q.y; tq[5] = q.z; tq[6] = q.w;
}

// ---- step 5: one row of the normal equations -------------------------------------------------------------------------------------
// e = observed - projected (2), J = d projected / d (dt, dtheta) under pose_oplus (left-multiplied rotation): acc[0..20] += the upper
// triangle of J^T J row by row, acc[21..26] += J^T e, acc[27] += e^T e.
BA_HD void normal_row(const Rt& T, const Cam& K, const Row& r, double acc[28]) {
    const Vec3 rx = visfs_ba::mat_vec(T.R, Vec3{ (double)r.X, (double)r.Y, (double)r.Z });
    const double x = rx.x + T.t.x, y = rx.y + T.t.y, z = rx.z + T.t.z;
    const double iz = z != 0.0 ? 1.0 / z : 1.0;
    const double ex = (double)r.u - (K.fx * (x * iz) + K.cx), ey = (double)r.v - (K.fy * (y * iz) + K.cy);
    const double a = K.fx * iz, b = K.fy * iz, c = -(K.fx * x) * (iz * iz), d = -(K.fy * y) * (iz * iz);
    // d pc / d dtheta = -[R X]x
    const double Ju[6] = { a, 0.0, c, c * rx.y, a * rx.z - c * rx.x, -a * rx.y };
    const double Jv[6] = { 0.0, b, d, d * rx.y - b * rx.z, -d * rx.x, b * rx.x };
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { acc[q] += Ju[i] * Ju[j] + Jv[i] * Jv[j]; ++q; }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += Ju[i] * ex + Jv[i] * ey;
    acc[27] += ex * ex + ey * ey;
}
BA_HD double cost_row(const Rt& T, const Cam& K, const Row& r) {
    double pu, pv;
    project(T, K, r, pu, pv);
    const double ex = (double)r.u - pu, ey = (double)r.v - pv;
    return ex * ex + ey * ey;
}

// (H + lambda diag H) d = g by Cholesky; false on a pivot that is not positive.
BA_HD bool damped_solve(const double acc[28], double lambda, double d[6]) {
    double L[6][6];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { L[j][i] = (i == j) ? acc[q] + lambda * acc[q] : acc[q]; ++q; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.0)) ok = false;
        const double dj = sqrt(s);
        L[j][j] = dj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / dj;
        }
    }
    if (!ok) return false;
    double yv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = acc[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= L[i][k] * yv[k];
        yv[i] = t / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double t = yv[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t -= L[k][i] * d[k];
        d[i] = t / L[i][i];
    }
    return true;
}

BA_HD Rt tq_to_rt(const double tq[7]) { return visfs_ba::pose_to_Rt(tq); }

// The refit: Levenberg-Marquardt on the pixel residual over list[0..n) from tq, in place.  P::sums(T, list, n, acc, full) fills acc
// (28 sums, or only acc[27] when !full) by the fixed tree and hands every caller the same values.
template <class P>
BA_HD void refit(P& pol, const Cam& K, int list, int n, double tq[7]) {
    double acc[28];
    pol.sums(tq_to_rt(tq), K, list, n, acc, false);
    double cost = acc[27], lambda = kLambda0;
    for (int it = 0; it < kRefitIterations; ++it) {
        pol.sums(tq_to_rt(tq), K, list, n, acc, true);
        double d[6];
        if (!damped_solve(acc, lambda, d)) {
            lambda *= 10.0;
            if (lambda > kLambdaMax) break;
            continue;
        }
        double cand[7];
        visfs_ba::pose_oplus(tq, d, cand);
        pol.sums(tq_to_rt(cand), K, list, n, acc, false);
        double step = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) if (fabs(d[i]) > step) step = fabs(d[i]);
        if (acc[27] < cost) {
#pragma unroll
            for (int i = 0; i < 7; ++i) tq[i] = cand[i];
            cost = acc[27];
            lambda = lambda * 0.1 > kLambdaMin ? lambda * 0.1 : kLambdaMin;
        } else {
            lambda *= 10.0;
            if (lambda > kLambdaMax) break;
        }
        if (step < kStepStop) break;
    }
}

// The convergence polish of a refit that a refine-only call adds: the refit above accepts a step only when the
// cost falls and stops at a step below kStepStop, which leaves the pose up to about 1e-10 from the least-squares optimum (near it a
// step changes the cost by less than a double resolves).  From there undamped Gauss-Newton steps are taken while they stay inside
// kPolishBasin, where such a step cannot move the pose by more than the basin; a refit that ended further out is left as it is.
constexpr int kPolishSteps = 3;
constexpr double kPolishBasin = 1e-6, kPolishStop = 1e-14;
template <class P>
BA_HD void polish(P& pol, const Cam& K, int list, int n, double tq[7]) {
    double acc[28];
    for (int it = 0; it < kPolishSteps; ++it) {
        pol.sums(tq_to_rt(tq), K, list, n, acc, true);
        double d[6];
        if (!damped_solve(acc, 0.0, d)) break;
        double step = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) if (fabs(d[i]) > step) step = fabs(d[i]);
        if (!(step < kPolishBasin)) break;
        double cand[7];
        visfs_ba::pose_oplus(tq, d, cand);
#pragma unroll
        for (int i = 0; i < 7; ++i) tq[i] = cand[i];
        if (step < kPolishStop) break;
    }
}

// ---- steps 5 and 6: from the winner to the returned model and list ---------------------------------------------------------------
// The policy keeps two row lists (0 and 1) and the float errors of the last selection:
//   select(T, K, thr, list) -> count : list := rows with error <= thr, ascending; the errors in the same order
//   spread(n, mean, var)             : uMean and uVariance of those errors (Math.h:58-67, :104-114)
//   same(n)                          : the first n entries of the two lists are equal
//   record(pass, tq, thr, list, n)   : test hook
//   finish(list, n)                  : the returned list
//   Polish: every refit is followed by polish() (the refine-only call of section 9x; the pose guess of section 9e runs without it)
template <class P, bool Polish = false>
BA_HD void refine_all(P& pol, const Cam& K, bool have_winner, const Rt& W, int min_inliers, int refine_iterations, float thr0, float sigma,
                      Result& res) {
    res.n_passes = 0; res.n_inliers = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) { res.refit0[i] = 0.0; res.tq[i] = 0.0; }
    if (!have_winner) { pol.finish(0, 0); return; }
    const int n0 = pol.select(W, K, thr0, 0);
    if (n0 < min_inliers || refine_iterations <= 0) { pol.finish(0, 0); return; }     // _inliers is never assigned (:241-245)
    double tq[7];
    rt_to_tq(W, tq);
    refit(pol, K, 0, n0, tq);
    if constexpr (Polish) polish(pol, K, 0, n0, tq);
#pragma unroll
    for (int i = 0; i < 7; ++i) res.refit0[i] = tq[i];
    int prev = 0, nprev = n0, cur = 1, ncur = 0;
    int hist = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;      // inliersSizes: its length and its last four entries, h1 the newest
    int it = 0;
    bool changed = false;
    float thr = thr0;
    for (;;) {
        refit(pol, K, prev, nprev, tq);
        if constexpr (Polish) polish(pol, K, prev, nprev, tq);
        h4 = h3; h3 = h2; h2 = h1; h1 = nprev; ++hist;
        ncur = pol.select(tq_to_rt(tq), K, thr, cur);
        if (res.n_passes < kMaxRefine) pol.record(res.n_passes, tq, thr, cur, ncur);
        ++res.n_passes;
        if (ncur < min_inliers) {
            ++it;
            if (it >= refine_iterations) break;
        } else {
            float mean, var;
            pol.spread(ncur, mean, var);
            const float st = sigma * (float)sqrt((double)var);
            thr = thr0 < st ? thr0 : st;                 // std::min(inlierThreshold, ...)
            changed = false;
            { const int t = prev; prev = cur; cur = t; }
            { const int t = nprev; nprev = ncur; ncur = t; }
            if (ncur != nprev) {
                if (hist >= min_inliers && h1 == h3 && h2 == h4) break;      // the history LENGTH against _minInliersCount (:282)
                changed = true;
            } else {
                changed = !pol.same(nprev);
            }
        }
        if (!(changed && ++it < refine_iterations)) break;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) res.tq[i] = tq[i];
    res.n_inliers = ncur;
    pol.finish(cur, ncur);                               // std::swap(_inliers, newInliers) (:310)
}

// ---- the pose guess inside a tracker call (include/visfs_tracker_pnp.h) ----------------------------------
// A member of the call: where its rows and its state stand in device memory.  k_pnp_ransac_g and k_pnp_refine_g read the record at
// blockIdx.z; the rows kernel of ba_tracker.hip has left the rows, their number and the zeroed winner key.
struct PnpRec {
    const int32_t* m;                          // rows with a finite 3-D point
    const Row* rows;
    unsigned long long* key;                   // (count << 32) | (0xFFFFFFFF - h) of the best hypothesis so far; 0: none
    int32_t* samples; int32_t* vc; double* models;     // per hypothesis, as RansacArgs has them
    Result* res; int32_t* inliers;             // in the output block of the member
    double* pass_tq; float* pass_thr; int32_t* pass_cnt; int32_t* pass_lists;
    Cam K;
    int32_t cap;                               // row stride of pass_lists
    int32_t skip;                              // the member takes no part in this call
};

// A member of a refine-only call (include/visfs_place_verify.h): k_pnp_refine_from_g runs the refinement loop
// on the member's rows from the model `start` holds.  *ran == 0: nothing runs for the member and its result stays what its rows
// kernel wrote; the same holds with fewer rows than min_inliers.
struct RefineFromRec {
    const int32_t* m;
    const Row* rows;
    const int32_t* ran;
    const Result* start;                       // its tq is the start model
    Result* res; int32_t* inliers;
    double* pass_tq; float* pass_thr; int32_t* pass_cnt; int32_t* pass_lists;
    Cam K;
    int32_t cap, pad;
};

// what every member of a call shares; min_inliers is already raised to 4
struct PnpShape { int32_t iterations, min_inliers, refine_iterations; float thr, sigma; uint64_t seed; };

}  // namespace pnp
