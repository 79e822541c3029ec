// ba_cov.hpp — marginal covariances of the optimised window: the block arithmetic of the banded factorisation and of the
// selected inversion (Takahashi), shared by the kernels (ba_cov.hip) and the host hook visfs_ba_hook_band_selinv.
//
// Band layout (the one of DeviceGraph::band_L): a symmetric block-banded matrix of n block rows and block half-bandwidth B is
// stored as [n][B + 1][36], block (I, I - d) of the LOWER band at [I][d], 6x6 row-major; slots with I - d < 0 are unused.
//
// Factor:  S = L L^T, L block lower with L_kk = C_k (the lower Cholesky factor of the pivot block, stored in full with zeros above
//          the diagonal) and L_ik = W_ik = G_ik C_k^-T below it (G: the block after the updates of the columns left of k).
// Inverse: with N_ik = W_ik C_k^-1 (so S = (I + N) C C^T (I + N)^T), for k = n - 1 .. 0
//          Sigma_jk = - sum_{i = k+1}^{k+B} Sigma_ji N_ik        (k < j <= k + B)
//          Sigma_kk = C_k^-T C_k^-1 - sum_{i = k+1}^{k+B} Sigma_ik^T N_ik
//          Every Sigma_ji it reads lies in the band (|j - i| < B), so the band of Sigma is computed without ever forming the rest.
//
// Every function below handles the work items [t0, t0 + dt, ...) of one step: the kernels pass (threadIdx.x, blockDim.x), the host
// passes (0, 1) — the same items, each summed in the same fixed order, so the device and the host hook compute the same arithmetic.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define COV_HD __host__ __device__
#else
#define COV_HD
#endif

namespace visfs_ba {
namespace cov {

COV_HD inline double* blk(double* band, int W, int I, int d) { return band + ((size_t)I * W + d) * 36; }
COV_HD inline const double* blk(const double* band, int W, int I, int d) { return band + ((size_t)I * W + d) * 36; }

// Lower Cholesky factor of the SPD 6x6 block a (row-major; only the lower triangle is read), in place, zeros above the diagonal.
// false: a pivot is not positive or not finite.
COV_HD inline bool chol6(double a[36]) {
    bool ok = true;
    for (int j = 0; j < 6; ++j) {
        double p = a[6 * j + j];
        for (int m = 0; m < j; ++m) p -= a[6 * j + m] * a[6 * j + m];
        ok = ok && (p > 0.0) && (p <= 1.7976931348623157e308);
        const double c = sqrt(p);
        a[6 * j + j] = c;
        for (int i = j + 1; i < 6; ++i) {
            double v = a[6 * i + j];
            for (int m = 0; m < j; ++m) v -= a[6 * i + m] * a[6 * j + m];
            a[6 * i + j] = v / c;
        }
        for (int i = 0; i < j; ++i) a[6 * i + j] = 0.0;
    }
    return ok;
}
// w C^T = g (a row of W = G C^-T): w_j = (g_j - sum_{m < j} w_m C_jm) / C_jj
COV_HD inline void row_fwd(const double* C, const double g[6], double w[6]) {
    for (int j = 0; j < 6; ++j) {
        double v = g[j];
        for (int m = 0; m < j; ++m) v -= w[m] * C[6 * j + m];
        w[j] = v / C[6 * j + j];
    }
}
// x C = z (a row of N = W C^-1): x_j = (z_j - sum_{m > j} x_m C_mj) / C_jj
COV_HD inline void row_bwd(const double* C, const double z[6], double x[6]) {
    for (int j = 5; j >= 0; --j) {
        double v = z[j];
        for (int m = 5; m > j; --m) v -= x[m] * C[6 * m + j];
        x[j] = v / C[6 * j + j];
    }
}
// entry (r, c) of the symmetric band matrix's block (a, b), |a - b| <= B
COV_HD inline double sym_at(const double* band, int W, int a, int b, int r, int c) {
    return a >= b ? blk(band, W, a, a - b)[6 * r + c] : blk(band, W, b, b - a)[6 * c + r];
}
// (m, j), 1 <= j <= m, of the p-th block of a trailing update listed by rows
COV_HD inline void pair_of(int p, int& m, int& j) {
    m = 1;
    while (m * (m + 1) / 2 <= p) ++m;
    j = p - (m - 1) * m / 2 + 1;
}

// ---- factorisation, step k (nb = min(B, n - 1 - k) blocks below the pivot)
// (1) the pivot: C_k replaces block (k, k).  One work item.
COV_HD inline bool factor_pivot(double* F, int W, int k) { return chol6(blk(F, W, k, 0)); }
// (2) W_{k+m,k} = G_{k+m,k} C_k^-T, a work item per scalar row (6 nb items)
COV_HD inline void factor_rows(double* F, int W, int k, int nb, int t0, int dt) {
    const double* C = blk(F, W, k, 0);
    for (int t = t0; t < 6 * nb; t += dt) {
        const int m = t / 6 + 1, r = t - 6 * (m - 1);
        double* row = blk(F, W, k + m, m) + 6 * r;
        double g[6], w[6];
        for (int c = 0; c < 6; ++c) g[c] = row[c];
        row_fwd(C, g, w);
        for (int c = 0; c < 6; ++c) row[c] = w[c];
    }
}
// (3) A_{k+m,k+j} -= W_{k+m,k} W_{k+j,k}^T for 1 <= j <= m <= nb, a work item per entry (36 nb (nb + 1) / 2 items)
COV_HD inline void factor_update(double* F, int W, int k, int nb, int t0, int dt) {
    const int n_items = 36 * (nb * (nb + 1) / 2);
    for (int t = t0; t < n_items; t += dt) {
        const int p = t / 36, q = t - 36 * p, r = q / 6, c = q - 6 * r;
        int m, j;
        pair_of(p, m, j);
        const double* Wm = blk(F, W, k + m, m) + 6 * r;
        const double* Wj = blk(F, W, k + j, j) + 6 * c;
        double s = 0.0;
        for (int e = 0; e < 6; ++e) s += Wm[e] * Wj[e];
        blk(F, W, k + m, m - j)[q] -= s;
    }
}

// ---- selected inversion, step k.  N: [B][36] scratch (N_{k+i,k} at i - 1), Ci: [36] scratch (C_k^-1, row-major).
// (1) N_{k+i,k} = W_{k+i,k} C_k^-1, a work item per scalar row (6 nb), and the columns of C_k^-1 (6 more items)
COV_HD inline void selinv_prep(const double* F, int W, int k, int nb, double* N, double* Ci, int t0, int dt) {
    const double* C = blk(F, W, k, 0);
    for (int t = t0; t < 6 * nb + 6; t += dt) {
        if (t < 6 * nb) {
            const int i = t / 6 + 1, r = t - 6 * (i - 1);
            const double* row = blk(F, W, k + i, i) + 6 * r;
            double z[6], x[6];
            for (int c = 0; c < 6; ++c) z[c] = row[c];
            row_bwd(C, z, x);
            for (int c = 0; c < 6; ++c) N[36 * (i - 1) + 6 * r + c] = x[c];
        } else {
            // column c of C^-1: forward substitution of C y = e_c
            const int c = t - 6 * nb;
            double y[6];
            for (int j = 0; j < 6; ++j) {
                double v = j == c ? 1.0 : 0.0;
                for (int m = 0; m < j; ++m) v -= C[6 * j + m] * y[m];
                y[j] = v / C[6 * j + j];
            }
            for (int j = 0; j < 6; ++j) Ci[6 * j + c] = y[j];
        }
    }
}
// (2) Sigma_{k+jj,k} = - sum_i Sigma_{k+jj,k+i} N_{k+i,k}, a work item per entry (36 nb)
COV_HD inline void selinv_off(double* Sg, int W, int k, int nb, const double* N, int t0, int dt) {
    for (int t = t0; t < 36 * nb; t += dt) {
        const int jj = t / 36 + 1, q = t - 36 * (jj - 1), r = q / 6, c = q - 6 * r;
        double s = 0.0;
        for (int i = 1; i <= nb; ++i) {
            const double* Ni = N + 36 * (i - 1);
            for (int e = 0; e < 6; ++e) s += sym_at(Sg, W, k + jj, k + i, r, e) * Ni[6 * e + c];
        }
        blk(Sg, W, k + jj, jj)[q] = -s;
    }
}
// (3) Sigma_kk = C_k^-T C_k^-1 - sum_i Sigma_{k+i,k}^T N_{k+i,k}, a work item per entry of the upper triangle (21), mirrored
COV_HD inline void selinv_diag(double* Sg, int W, int k, int nb, const double* N, const double* Ci, int t0, int dt) {
    for (int t = t0; t < 21; t += dt) {
        int r = 0, rem = t;
        while (rem >= 6 - r) { rem -= 6 - r; ++r; }
        const int c = r + rem;
        double d = 0.0;
        for (int e = 0; e < 6; ++e) d += Ci[6 * e + r] * Ci[6 * e + c];
        double s = 0.0;
        for (int i = 1; i <= nb; ++i) {
            const double* Si = blk(Sg, W, k + i, i);
            const double* Ni = N + 36 * (i - 1);
            for (int e = 0; e < 6; ++e) s += Si[6 * e + r] * Ni[6 * e + c];
        }
        double* D = blk(Sg, W, k, 0);
        D[6 * r + c] = d - s;
        D[6 * c + r] = d - s;
    }
}

// Inverse of the SPD 3x3 block h = (xx xy xz yy yz zz) through its Cholesky factor; false when it is not positive definite.
COV_HD inline bool inv3_spd(const double h[6], double out[9]) {
    const double l00s = h[0];
    if (!(l00s > 0.0)) return false;
    const double l00 = sqrt(l00s), l10 = h[1] / l00, l20 = h[2] / l00;
    const double l11s = h[3] - l10 * l10;
    if (!(l11s > 0.0)) return false;
    const double l11 = sqrt(l11s), l21 = (h[4] - l20 * l10) / l11;
    const double l22s = h[5] - l20 * l20 - l21 * l21;
    if (!(l22s > 0.0)) return false;
    const double l22 = sqrt(l22s);
    // Y = L^-1 (lower), inverse = Y^T Y
    const double y00 = 1.0 / l00, y11 = 1.0 / l11, y22 = 1.0 / l22;
    const double y10 = -l10 * y00 / l11;
    const double y21 = -l21 * y11 / l22;
    const double y20 = -(l20 * y00 + l21 * y10) / l22;
    out[0] = y00 * y00 + y10 * y10 + y20 * y20;
    out[1] = y10 * y11 + y20 * y21;
    out[2] = y20 * y22;
    out[4] = y11 * y11 + y21 * y21;
    out[5] = y21 * y22;
    out[8] = y22 * y22;
    out[3] = out[1]; out[6] = out[2]; out[7] = out[5];
    return true;
}

}  // namespace cov
}  // namespace visfs_ba
