// ba_fund.hpp — the arithmetic of the fundamental-matrix cull (include/visfs_fund.h), shared by the HIP kernels of ba_fund.hip and the
// one-core host twin: the seven-row counter-hash sampler, the seven-point solver (a 7x9 null space by Gauss-Jordan elimination with
// full pivoting, the cubic det(f1 + x f2) by explicit polynomial products, one root by bisection, two from the deflated quadratic,
// Newton polish), the canonical form and order of the models, and the symmetric epipolar error.  DESIGN.md section 9f states every
// step.
//
// Everything is + - * / sqrt in a fixed order with contraction off, so the device and the twin produce the same bits.  Every index
// that depends on the data is resolved by compare-and-select over fully unrolled loops: the 7x9 matrix stays in registers.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#pragma clang fp contract(off)

#include "ba_pnp.hpp"      // mix64, the counter hash of section 9e step 2

namespace fund {

constexpr int kMaxPoints = 4096;
constexpr int kMaxHypotheses = 4096;
constexpr int kMinRows = 7;
constexpr int kBisections = 100;
constexpr int kPolishSteps = 4;
constexpr double kPivotFraction = 1e-9;    // a pivot below this fraction of the first (the largest entry of A) makes the sample invalid
constexpr double kLeadFraction = 1e-10;    // so does a leading coefficient below this fraction of the cubic's largest coefficient
constexpr double kNormMax = 1e300;         // a model whose squared norm is not in (0, kNormMax) is dropped: a root that is not finite

struct Row { float x1, y1, x2, y2; };      // one correspondence on the raw pixels: from, to
struct Hartley { double cx, cy, s; };      // x^ = (x - cx) s; as a matrix [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]

// ---- step 3: n distinct rows of m by the counter hash ------------------------------------------------------------------------------
template <int N>
BA_HD void sample_rows(uint64_t seed, int32_t h, int32_t m, int32_t s[N]) {
    int32_t taken[N];                      // the rows taken so far, ascending
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const uint64_t r = pnp::mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(N * (int64_t)h + k + 1));
        int32_t j = (int32_t)(r % (uint64_t)(m - k));
#pragma unroll
        for (int i = 0; i < N; ++i) if (i < k && j >= taken[i]) ++j;
        s[k] = j;
        int32_t carry = j;                 // insert j, keeping the order
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i >= k) continue;
            const int32_t t = taken[i];
            const bool sw = carry < t;
            taken[i] = sw ? carry : t;
            carry = sw ? t : carry;
        }
        taken[k] = carry;
    }
}

// ---- step 2: conditioned coordinates and the denormalisation F = T2^T F^ T1 --------------------------------------------------------
BA_HD double cond(double v, double c, double s) { return (v - c) * s; }
BA_HD void denormalise(const double Fh[9], const Hartley& T1, const Hartley& T2, double F[9]) {
    const double tx1 = -(T1.s * T1.cx), ty1 = -(T1.s * T1.cy), tx2 = -(T2.s * T2.cx), ty2 = -(T2.s * T2.cy);
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        M[3 * i] = Fh[3 * i] * T1.s;
        M[3 * i + 1] = Fh[3 * i + 1] * T1.s;
        M[3 * i + 2] = (Fh[3 * i] * tx1 + Fh[3 * i + 1] * ty1) + Fh[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        F[j] = T2.s * M[j];
        F[3 + j] = T2.s * M[3 + j];
        F[6 + j] = (tx2 * M[j] + ty2 * M[3 + j]) + M[6 + j];
    }
}

// The Hartley transform of one image (section 9f step 2) in pieces that the host and the rows kernel of the resident tracker
// (section 9j) share: every sum is one serial chain of rounded double additions in row order, so where a chain runs changes no bit.
// The terms of a chain do not depend on it and may be made by anybody.
template <class T>
BA_HD double serial_sum(const T* v, int m, int stride) {
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < m; ++i) s += (double)v[(size_t)i * stride];
    return s;
}
BA_HD double centre_distance(double x, double y, double cx, double cy) {
    const double dx = x - cx, dy = y - cy;
    return sqrt(dx * dx + dy * dy);
}
BA_HD Hartley hartley_of(double cx, double cy, double sd, double m) {
    Hartley T;
    T.cx = cx; T.cy = cy;
    const double mean = sd / m;
    T.s = mean > 0.0 ? 1.4142135623730951 / mean : 1.0;
    return T;
}
// one image of m rows (to: the second); term[m]: room for the distances
BA_HD Hartley hartley(const Row* rows, int m, bool to, double* term) {
    const float *x = to ? &rows->x2 : &rows->x1, *y = to ? &rows->y2 : &rows->y1;
    const double cx = serial_sum(x, m, 4) / (double)m, cy = serial_sum(y, m, 4) / (double)m;
    for (int i = 0; i < m; ++i) term[i] = centre_distance((double)x[4 * (size_t)i], (double)y[4 * (size_t)i], cx, cy);
    return hartley_of(cx, cy, serial_sum(term, m, 1), (double)m);
}
BA_HD void hartley_matrix(const Hartley& T, double* o) {
    o[0] = T.s; o[1] = 0.0; o[2] = -(T.s * T.cx); o[3] = 0.0; o[4] = T.s; o[5] = -(T.s * T.cy); o[6] = 0.0; o[7] = 0.0; o[8] = 1.0;
}

// ---- step 5: FMEstimatorCallback::computeError; the row is an inlier iff both halves, narrowed to float, are within thr2 ----------
BA_HD bool inlier(const double F[9], const Row& r, float thr2) {
    const double x1 = (double)r.x1, y1 = (double)r.y1, x2 = (double)r.x2, y2 = (double)r.y2;
    double a = (F[0] * x1 + F[1] * y1) + F[2];
    double b = (F[3] * x1 + F[4] * y1) + F[5];
    double c = (F[6] * x1 + F[7] * y1) + F[8];
    const double d2 = (x2 * a + y2 * b) + c;
    const double e2 = (d2 * d2) / (a * a + b * b);
    a = (F[0] * x2 + F[3] * y2) + F[6];
    b = (F[1] * x2 + F[4] * y2) + F[7];
    c = (F[2] * x2 + F[5] * y2) + F[8];
    const double d1 = (x1 * a + y1 * b) + c;
    const double e1 = (d1 * d1) / (a * a + b * b);
    return (float)e1 <= thr2 && (float)e2 <= thr2;     // (float)max(e1, e2) <= thr2, and false on a NaN
}

// ---- step 4: the seven-point solver -------------------------------------------------------------------------------------------------
BA_HD double pick9(const double v[9], int idx) {
    double r = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) r = (c == idx) ? v[c] : r;
    return r;
}

// (p1 x + p0)(q1 x + q0) and (a2 x^2 + a1 x + a0)(q1 x + q0), accumulated with a sign
struct Lin { double c1, c0; };
struct Quad { double c2, c1, c0; };
BA_HD Quad lin_mul(const Lin& p, const Lin& q) { return Quad{ p.c1 * q.c1, p.c1 * q.c0 + p.c0 * q.c1, p.c0 * q.c0 }; }
BA_HD Quad quad_sub(const Quad& a, const Quad& b) { return Quad{ a.c2 - b.c2, a.c1 - b.c1, a.c0 - b.c0 }; }
BA_HD void cubic_add(double c[4], const Lin& p, const Quad& q, double sign) {
    c[3] += sign * (p.c1 * q.c2);
    c[2] += sign * (p.c1 * q.c1 + p.c0 * q.c2);
    c[1] += sign * (p.c1 * q.c0 + p.c0 * q.c1);
    c[0] += sign * (p.c0 * q.c0);
}

// The models of seven conditioned correspondences: Fh[k][9] (row-major), k < the returned count (0 .. 3), ordered by ascending
// Fh[k][8]; the rest of Fh is zero.
BA_HD int seven_point(const double x1[7], const double y1[7], const double x2[7], const double y2[7], double Fh[3][9]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) Fh[k][i] = 0.0;
    double A[7][9];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        A[r][0] = x2[r] * x1[r]; A[r][1] = x2[r] * y1[r]; A[r][2] = x2[r];
        A[r][3] = y2[r] * x1[r]; A[r][4] = y2[r] * y1[r]; A[r][5] = y2[r];
        A[r][6] = x1[r]; A[r][7] = y1[r]; A[r][8] = 1.0;
    }
    // Gauss-Jordan with full pivoting: step p takes the largest |entry| of rows p.. over the columns not used yet (the first in
    // row-major order among equals), brings its row to p and clears its column in every other row.
    int pivcol[7];
    unsigned used = 0;
    double first = 0.0;
    bool ok = true;
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        double best = -1.0;
        int br = p, bc = 0;
#pragma unroll
        for (int r = 0; r < 7; ++r)
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                if (r < p) continue;
                const double v = fabs(A[r][c]);
                const bool take = !((used >> c) & 1u) && v > best;
                best = take ? v : best; br = take ? r : br; bc = take ? c : bc;
            }
        if (p == 0) first = best;
        if (!(best >= kPivotFraction * first) || !(first > 0.0) || !(best < kNormMax)) ok = false;
        used |= 1u << bc;
        pivcol[p] = bc;
#pragma unroll
        for (int r = 0; r < 7; ++r) {              // swap rows p and br
            if (r <= p) continue;
            const bool sw = r == br;
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double u = A[p][c], w = A[r][c];
                A[p][c] = sw ? w : u; A[r][c] = sw ? u : w;
            }
        }
        const double piv = pick9(A[p], bc);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            if (r == p) continue;
            const double f = pick9(A[r], bc) / piv;
#pragma unroll
            for (int c = 0; c < 9; ++c) A[r][c] = (c == bc) ? 0.0 : A[r][c] - f * A[p][c];
        }
    }
    if (!ok) return 0;
    // the two free columns, ascending; null vector j has 1 in free column j, 0 in the other, -A[p][free] / pivot_p in pivot column p
    int f1c = -1, f2c = -1;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const bool fr = !((used >> c) & 1u);
        const bool isfirst = fr && f1c < 0;
        f2c = (fr && !isfirst) ? c : f2c;
        f1c = isfirst ? c : f1c;
    }
    double n1[9], n2[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { n1[c] = (c == f1c) ? 1.0 : 0.0; n2[c] = (c == f2c) ? 1.0 : 0.0; }
#pragma unroll
    for (int p = 0; p < 7; ++p) {
        const double piv = pick9(A[p], pivcol[p]);
        const double v1 = -(pick9(A[p], f1c) / piv), v2 = -(pick9(A[p], f2c) / piv);
#pragma unroll
        for (int c = 0; c < 9; ++c) { n1[c] = (c == pivcol[p]) ? v1 : n1[c]; n2[c] = (c == pivcol[p]) ? v2 : n2[c]; }
    }
    // det(n1 + x n2) = c3 x^3 + c2 x^2 + c1 x + c0, expanded along the first row
    Lin P[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) P[i] = Lin{ n2[i], n1[i] };
    double c[4] = { 0.0, 0.0, 0.0, 0.0 };
    cubic_add(c, P[0], quad_sub(lin_mul(P[4], P[8]), lin_mul(P[5], P[7])), 1.0);
    cubic_add(c, P[1], quad_sub(lin_mul(P[3], P[8]), lin_mul(P[5], P[6])), -1.0);
    cubic_add(c, P[2], quad_sub(lin_mul(P[3], P[7]), lin_mul(P[4], P[6])), 1.0);
    double big = fabs(c[0]);
#pragma unroll
    for (int i = 1; i < 4; ++i) big = fabs(c[i]) > big ? fabs(c[i]) : big;
    if (!(fabs(c[3]) >= kLeadFraction * big) || !(big > 0.0) || !(big < kNormMax)) return 0;
    const double b2 = c[2] / c[3], b1 = c[1] / c[3], b0 = c[0] / c[3];
    // one real root of the monic cubic between -+ the Cauchy bound, where its signs differ
    double bound = fabs(b2);
    bound = fabs(b1) > bound ? fabs(b1) : bound;
    bound = fabs(b0) > bound ? fabs(b0) : bound;
    double lo = -(1.0 + bound), hi = 1.0 + bound;
    for (int it = 0; it < kBisections; ++it) {
        const double mid = 0.5 * (lo + hi);
        const double f = ((mid + b2) * mid + b1) * mid + b0;
        if (f > 0.0) hi = mid; else lo = mid;
    }
    double root[3];
    root[0] = hi;
    // the deflated quadratic x^2 + p x + q
    const double pq = b2 + root[0], qq = b1 + pq * root[0];
    const double disc = pq * pq - 4.0 * qq;
    const int nroots = disc >= 0.0 ? 3 : 1;
    const double sq = sqrt(disc >= 0.0 ? disc : 0.0);
    root[1] = 0.5 * (-pq - sq);
    root[2] = 0.5 * (-pq + sq);
    int n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double x = root[k];
        for (int it = 0; it < kPolishSteps; ++it) {
            const double f = ((x + b2) * x + b1) * x + b0;
            const double df = (3.0 * x + 2.0 * b2) * x + b1;
            x = x - f / df;
        }
        double G[9], norm2 = 0.0, amax = -1.0, sign = 1.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            G[i] = n1[i] + x * n2[i];
            norm2 += G[i] * G[i];
            const double a = fabs(G[i]);
            if (a > amax) { amax = a; sign = G[i] < 0.0 ? -1.0 : 1.0; }
        }
        const bool keep = k < nroots && norm2 > 0.0 && norm2 < kNormMax;
        const double inv = sign / sqrt(keep ? norm2 : 1.0);
        if (keep) {
            // insert by ascending F^[2][2] among the n models held (n <= 2 here; the slots behind them are zero)
            const double key = G[8] * inv;
            const int pos = ((n > 0 && Fh[0][8] <= key) ? 1 : 0) + ((n > 1 && Fh[1][8] <= key) ? 1 : 0);
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double v = G[i] * inv;
                const double m0 = Fh[0][i], m1 = Fh[1][i];
                Fh[2][i] = pos == 2 ? v : m1;
                Fh[1][i] = pos == 1 ? v : (pos == 0 ? m0 : m1);
                Fh[0][i] = pos == 0 ? v : m0;
            }
            ++n;
        }
    }
    return n;
}

// ---- the control flow of a call, written once over a policy -------------------------------------------------------------------------
// What the copy in carries in front of the rows (the winner key is zeroed by that copy) and what the copy out carries in front of the
// mask and the status.
struct Header {
    unsigned long long key;    // (count << 32) | (0xFFFFFFFF - (3 h + k)) of the best model so far; 0: none
    unsigned long long pad;
    Hartley T1, T2;
};
struct Result {
    int32_t winner_h, winner_k, count, pad;
    double F[9];
};
struct Call {
    Hartley T1, T2;
    int32_t m, iterations;
    uint64_t seed;
    float thr2;
};

BA_HD unsigned long long winner_key(int32_t count, int32_t h, int k) {
    return ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(3 * h + k));
}

// The models of the sample s: P::row(i) hands every caller the same row.
template <class P>
BA_HD int solve_sample(P& pol, const Call& c, const int32_t s[7], double Fh[3][9]) {
    double x1[7], y1[7], x2[7], y2[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const Row r = pol.row(s[k]);
        x1[k] = cond((double)r.x1, c.T1.cx, c.T1.s); y1[k] = cond((double)r.y1, c.T1.cy, c.T1.s);
        x2[k] = cond((double)r.x2, c.T2.cx, c.T2.s); y2[k] = cond((double)r.y2, c.T2.cy, c.T2.s);
    }
    return seven_point(x1, y1, x2, y2, Fh);
}

// Hypothesis h: sample, solve, score every model in one pass over the rows, record, propose.
//   P::count(F, n, counts) : counts[k] = inliers of F[k] over the m rows for k < n, 0 behind; every caller gets the same values
//   P::record(h, s, n, Fh, counts) : the test hook stores and the proposals to the winner key
template <class P>
BA_HD void hypothesis(P& pol, const Call& c, int32_t h) {
    int32_t s[7];
    sample_rows<7>(c.seed, h, c.m, s);
    double Fh[3][9], F[3][9];
    const int n = solve_sample(pol, c, s, Fh);
#pragma unroll
    for (int k = 0; k < 3; ++k) denormalise(Fh[k], c.T1, c.T2, F[k]);
    int32_t counts[3];
    pol.count(F, n, counts);
    pol.record(h, s, n, Fh, counts);
}

// The winner from the key: Result without the mask; F is zero without a winner.
BA_HD Result winner_of(unsigned long long key, const double* models, const Call& c) {
    Result res;
    res.pad = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) res.F[i] = 0.0;
    if (key == 0) { res.winner_h = -1; res.winner_k = -1; res.count = 0; return res; }
    const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    res.winner_h = (int32_t)(idx / 3u); res.winner_k = (int32_t)(idx % 3u); res.count = (int32_t)(key >> 32);
    double Fh[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Fh[i] = models[9 * (size_t)idx + i];
    denormalise(Fh, c.T1, c.T2, res.F);
    return res;
}

// ---- the cull inside the resident tracker (include/visfs_tracker.h, section 9j) ------------------------------------------------------
// Where the cull of one tracker works, in device memory or, for the host twin, in host memory.  The rows kernel of ba_tracker.hip fills
// m, head, rows, keep, st and the pass-through of mask and status; the search and the mask of ba_fund.hip read a table of these at
// member blockIdx.z.
struct CullRec {
    int32_t* m;                                // rows that entered
    Header* head;                              // the winner key and the two transforms
    Row* rows; int32_t* keep; uint8_t* st;     // [m]: the rows that entered, their from-row numbers, their Lucas-Kanade status
    int32_t* samples; int32_t* nc; double* models;     // per hypothesis, as RansacArgs has them
    Result* res;
    uint8_t* mask; uint8_t* status;            // per from-row: the winner's mask, the status after the AND
    int32_t skip, pad;                         // the member takes no part in this call
};

// what every member of a call shares
struct CullShape { int32_t iterations; float thr2; uint64_t seed; };

BA_HD float cull_thr2(float pixel_error) {
    const float thr = pixel_error > 0.0f ? pixel_error : 3.0f;
    return (float)((double)thr * (double)thr);
}


}  // namespace fund
