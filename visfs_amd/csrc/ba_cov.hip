// ba_cov.hip — marginal covariances of the optimised window on gfx950 (visfs_ba_graph_covariance).
//
// The covariance is the inverse of the Gauss-Newton Hessian of the g2o branch at the resident estimate (active edges, no lambda, the
// fixed poses fix the gauge).  The host re-linearises with the production kernels (k_linearize ... k_schur_finalize at lambda = 0),
// which leaves S, H_ll and the H_pl tiles in HBM; then three launches:
//   k_band_factor   one workgroup: the block-banded Cholesky factor of S (unscaled: the C_k and W_ik of ba_cov.hpp) to HBM;
//   k_band_selinv   one workgroup: the band of Sigma = S^-1 by the block Takahashi recurrence, last block row first;
//   k_point_cov     a thread per landmark (only when point covariances are asked for): Sigma_ll = D^-1 + sum E_i^T Sigma_ij E_j.
// fp64 throughout, no atomics, every sum in a fixed order: the results are bitwise reproducible run to run.  Rare calls, off the
// per-frame path: the kernels are written for clarity, the factor and Sigma live in HBM (L2-resident at these sizes).
#include <hip/hip_runtime.h>

#include "ba_cov.hpp"
#include "ba_kernels.hpp"

namespace visfs_ba {

constexpr int COV_T = 256;

// fail[0] = 1: a pivot of the factorisation is not positive (or not finite); the later steps are skipped.
__global__ __launch_bounds__(COV_T) void k_band_factor(const DeviceGraph g, double* __restrict__ F, int* __restrict__ fail) {
    const int Npf = g.Npf, B = g.band_B, W = B + 1, tid = threadIdx.x;
    __shared__ int bad;
    // the lower band of S: block (I, I - d) is the transpose of the stored upper block (I - d, I) (DeviceGraph::band_code)
    for (size_t t = tid; t < (size_t)Npf * W * 36; t += COV_T) {
        const int slot = (int)(t / 36), q = (int)(t - 36 * (size_t)slot), I = slot / W, d = slot - W * I, r = q / 6, c = q - 6 * r;
        const int b = I - d >= 0 ? g.band_code[slot] : -1;
        F[t] = b >= 0 ? g.S[36 * (size_t)b + 6 * c + r] : 0.0;
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < Npf; ++k) {
        const int nb = min(B, Npf - 1 - k);
        if (tid == 0 && !cov::factor_pivot(F, W, k)) bad = 1;
        __syncthreads();
        if (bad) break;
        cov::factor_rows(F, W, k, nb, tid, COV_T);
        __syncthreads();
        cov::factor_update(F, W, k, nb, tid, COV_T);
        __syncthreads();
    }
    if (tid == 0) fail[0] = bad;
}

__global__ __launch_bounds__(COV_T) void k_band_selinv(const int Npf, const int B, const double* __restrict__ F, double* __restrict__ Sg,
                                                       const int* __restrict__ fail) {
    if (fail[0]) return;
    const int W = B + 1, tid = threadIdx.x;
    extern __shared__ double cov_lds[];
    double* N = cov_lds;                  // [B][36]
    double* Ci = cov_lds + 36 * B;        // [36]
    for (int k = Npf - 1; k >= 0; --k) {
        const int nb = min(B, Npf - 1 - k);
        cov::selinv_prep(F, W, k, nb, N, Ci, tid, COV_T);
        __syncthreads();
        cov::selinv_off(Sg, W, k, nb, N, tid, COV_T);
        __syncthreads();
        cov::selinv_diag(Sg, W, k, nb, N, Ci, tid, COV_T);
        __syncthreads();
    }
}

// Landmark l: fixed -> zeros; free without an active edge -> NaN; else D^-1 + sum_{a, b} E_a^T Sigma_{p(a) p(b)} E_b with E = W D^-1 over
// its active observations of free poses, a-major then b, in observation order.  out: [Nl][9] row-major.
__global__ __launch_bounds__(COV_T) void k_point_cov(const DeviceGraph g, const double* __restrict__ Sg, double* __restrict__ out,
                                                     const int* __restrict__ fail) {
    const int l = blockIdx.x * COV_T + threadIdx.x;
    if (l >= g.Nl || fail[0]) return;                          // (a failed factorisation left no Sigma band to read)
    double* o = out + 9 * (size_t)l;
    if (g.pt_fixed[l]) { for (int q = 0; q < 9; ++q) o[q] = 0.0; return; }
    const int k0 = g.lm_ptr[l], k1 = g.lm_ptr[l + 1];
    int n_active = 0;
    for (int k = k0; k < k1; ++k) n_active += (g.obs_level[k] == 0 && g.obs_ok[k]) ? 1 : 0;
    const LinBuf L = lin_of(g, g.st->lin_sel & 1);
    double h[6], Di[9];
    for (int q = 0; q < 6; ++q) h[q] = L.Hll[6 * (size_t)l + q];
    if (n_active == 0 || !cov::inv3_spd(h, Di)) { for (int q = 0; q < 9; ++q) o[q] = __builtin_nan(""); return; }
    const int W = g.band_B + 1;
    double acc[9];
    for (int q = 0; q < 9; ++q) acc[q] = Di[q];
    for (int a = k0; a < k1; ++a) {
        const int pa = g.pose_free[g.obs_pose[a]];
        if (pa < 0 || g.obs_level[a] != 0) continue;
        double Ea[18];                                         // E_a = W_a D^-1, 6x3
        const double* Wa = g.W + 18 * (size_t)a;
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 3; ++c) Ea[3 * r + c] = Wa[3 * r] * Di[c] + Wa[3 * r + 1] * Di[3 + c] + Wa[3 * r + 2] * Di[6 + c];
        double V[18];                                          // V = sum_b Sigma_{pa pb} E_b
        for (int q = 0; q < 18; ++q) V[q] = 0.0;
        for (int b = k0; b < k1; ++b) {
            const int pb = g.pose_free[g.obs_pose[b]];
            if (pb < 0 || g.obs_level[b] != 0) continue;
            double Eb[18];
            const double* Wb = g.W + 18 * (size_t)b;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 3; ++c) Eb[3 * r + c] = Wb[3 * r] * Di[c] + Wb[3 * r + 1] * Di[3 + c] + Wb[3 * r + 2] * Di[6 + c];
            for (int r = 0; r < 6; ++r)
                for (int e = 0; e < 6; ++e) {
                    const double s = cov::sym_at(Sg, W, pa, pb, r, e);
                    for (int c = 0; c < 3; ++c) V[3 * r + c] += s * Eb[3 * e + c];
                }
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double s = 0.0;
                for (int e = 0; e < 6; ++e) s += Ea[3 * e + r] * V[3 * e + c];
                acc[3 * r + c] += s;
            }
    }
    for (int r = 0; r < 3; ++r)                                // symmetric by construction up to rounding: the mean of the two halves
        for (int c = r; c < 3; ++c) { const double v = 0.5 * (acc[3 * r + c] + acc[3 * c + r]); o[3 * r + c] = v; o[3 * c + r] = v; }
}

void launch_band_factor(const DeviceGraph& g, double* F, int* fail, hipStream_t s) {
    hipLaunchKernelGGL(k_band_factor, dim3(1), dim3(COV_T), 0, s, g, F, fail);
}
void launch_band_selinv(const DeviceGraph& g, const double* F, double* Sg, const int* fail, hipStream_t s) {
    hipLaunchKernelGGL(k_band_selinv, dim3(1), dim3(COV_T), (size_t)(36 * g.band_B + 36) * sizeof(double), s, g.Npf, g.band_B, F, Sg, fail);
}
void launch_point_cov(const DeviceGraph& g, const double* Sg, double* out, const int* fail, hipStream_t s) {
    if (g.Nl > 0) hipLaunchKernelGGL(k_point_cov, dim3((g.Nl + COV_T - 1) / COV_T), dim3(COV_T), 0, s, g, Sg, out, fail);
}

}  // namespace visfs_ba
