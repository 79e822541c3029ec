// Monte-Carlo localisation on a likelihood field (include/visfs_mcl.h): the definition of every step, which
// the kernels of ba_mcl.hip and the one-core twin both call, and the host parts (the table, the motion plan, finalize).
//
// The device and the twin agree byte for byte: every double below is formed by + - * / sqrt round in one order, without
// contraction; every quantity that work items share is an integer (the field, the beam sums Q, the resampling counts), or a
// floating sum whose order is the adjacent-pair tree of the definition.  exp, atan2 and log run on the host only.
#pragma once
#pragma clang fp contract(off)

#include "ba_scan_refine.hpp"      // sincos_poly; first, as its head asks
#include "ba_pnp.hpp"              // mix64

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/visfs_mcl.h"

namespace mcl {

constexpr int kThreads = 256;                 // work items of every workgroup; the partial sums below are of 256 particles
constexpr int kSums = 9;                      // w, w^2, wx, wy, w cos, w sin, wxx, wxy, wyy
constexpr int kMaxBlocks = VISFS_MCL_MAX_PARTICLES / kThreads;
constexpr int32_t kCellClamp = 1 << 30;
constexpr double kTwo40 = 1099511627776.0;
constexpr double kTwo32 = 4294967296.0;
constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
constexpr double kPi = 0x1.921fb54442d18p+1;          // the doubles nearest pi and 2 pi
constexpr double kTwoPi = 0x1.921fb54442d18p+2;
constexpr double kTwoOverPi = 0x1.45f306dc9c883p-1;
constexpr double kP1 = 0x1.921fb54400000p+0;          // pi / 2 in three pieces: 33 bits, 33 bits, the rest
constexpr double kP2 = 0x1.0b4611a600000p-34;
constexpr double kP3 = 0x1.3198a2e037073p-69;

// ---------------------------------------------------------------- angles

// sin and cos of a, |a| <= 16: k = round(a 2/pi), a three-constant Cody-Waite remainder (k P1 and k P2 are exact for |k| < 2^20),
// the polynomial of section 9o on it, the quadrant by sign and swap.
__host__ __device__ inline void sincos_any(double a, double& s, double& c) {
    const double k = ::round(a * kTwoOverPi);
    const double r = ((a - k * kP1) - k * kP2) - k * kP3;
    double sr, cr;
    scanrefine::sincos_poly(r, sr, cr);
    const int32_t q = (int32_t)k & 3;
    if (q == 0) { s = sr; c = cr; }
    else if (q == 1) { s = cr; c = -sr; }
    else if (q == 2) { s = -sr; c = -cr; }
    else { s = -cr; c = sr; }
}

// into (-pi, pi] by one step of 2 pi
__host__ __device__ inline double wrap(double yaw) {
    if (yaw > kPi) return yaw - kTwoPi;
    if (yaw <= -kPi) return yaw + kTwoPi;
    return yaw;
}

// ---------------------------------------------------------------- random numbers

__host__ __device__ inline uint64_t key(uint64_t seed, uint64_t update, uint64_t particle, uint64_t draw) {
    uint64_t h = pnp::mix64(seed + kGold * (update + 1));
    h = pnp::mix64(h + kGold * (particle + 1));
    return pnp::mix64(h + kGold * (draw + 1));
}

// A standard normal as the sum of twelve uniforms: the twelve 32-bit halves of six outputs, exact up to the conversion.
__host__ __device__ inline double normal(uint64_t h) {
    uint64_t s = 0;
    for (uint64_t m = 1; m <= 6; ++m) {
        const uint64_t r = pnp::mix64(h + kGold * m);
        s += (r >> 32) + (r & 0xFFFFFFFFull);
    }
    return (double)((int64_t)s - 6 * (int64_t)0xFFFFFFFFll) / kTwo32;
}

// ---------------------------------------------------------------- the field

__host__ __device__ inline bool occupied(uint16_t v, int32_t v_occ) {
    const int32_t u = v & 32767;
    return u >= 1 && u <= v_occ;
}

// The distance along row y from x to the nearest obstacle of the row, R + 1 when none lies within R.
__host__ __device__ inline uint16_t row_dist(const uint16_t* __restrict__ cells, int32_t nx, int32_t x, int32_t y, int32_t v_occ, int32_t R) {
    const uint16_t* row = cells + (int64_t)y * nx;
    for (int32_t d = 0; d <= R; ++d) {
        if (x - d >= 0 && occupied(row[x - d], v_occ)) return (uint16_t)d;
        if (x + d < nx && occupied(row[x + d], v_occ)) return (uint16_t)d;
    }
    return (uint16_t)(R + 1);
}

// min(T, min over |dy| <= R of dy^2 + g^2) down column x; (R + 1)^2 >= T, so a row without an obstacle never wins.
__host__ __device__ inline uint16_t col_min(const uint16_t* __restrict__ g, int32_t nx, int32_t ny, int32_t x, int32_t y, int32_t R, int32_t T) {
    int32_t best = T;
    for (int32_t d = 0; d <= R; ++d) {
        const int32_t d2 = d * d;
        if (d2 >= best) break;
        if (y - d >= 0) {
            const int32_t a = g[(int64_t)(y - d) * nx + x], v = d2 + a * a;
            if (v < best) best = v;
        }
        if (d > 0 && y + d < ny) {
            const int32_t a = g[(int64_t)(y + d) * nx + x], v = d2 + a * a;
            if (v < best) best = v;
        }
    }
    return (uint16_t)best;
}

// What a weight reads of a field.
struct FieldView {
    const uint16_t* t = nullptr;
    const int64_t* q = nullptr;
    double res = 0.0, max_x = 0.0, max_y = 0.0;
    int32_t nx = 0, ny = 0, T = 0;
};

// submap::cell_index's rounding, saturating; a NaN lands outside
__host__ __device__ inline int32_t round_cell(double v) {
    const double r = ::round(v);
    if (!(r < (double)kCellClamp)) return kCellClamp;
    if (!(r > -(double)kCellClamp)) return -kCellClamp;
    return (int32_t)r;
}

// q[t] at the endpoint of beam (px, py) seen from (x, y) with (c, s) = cos, sin of the yaw.
__host__ __device__ inline int64_t beam_q(const FieldView& F, double x, double y, double c, double s, double px, double py) {
    const double ex = x + (c * px - s * py);
    const double ey = y + (s * px + c * py);
    const int32_t ix = round_cell((F.max_y - ey) / F.res - 0.5);
    const int32_t iy = round_cell((F.max_x - ex) / F.res - 0.5);
    int32_t t = F.T;
    if (ix >= 0 && iy >= 0 && ix < F.nx && iy < F.ny) t = F.t[(int64_t)iy * F.nx + ix];
    return F.q[t];
}

// ---------------------------------------------------------------- the motion

struct Motion { double rot1, trans, rot2, s_r1, s_t, s_r2; };

// What one update uploads ahead of its beams ([n][2] doubles).
struct Hdr {
    Motion M;
    double ratio_n;                           // n_eff_ratio * N
    double inv_n;                             // 1 / N
    uint64_t seed, update;
    int32_t N, n, P, gate;                    // P: N rounded up to a power of two; gate: the counter is a multiple of the interval
    int32_t lanes, pad;
};

// What one update downloads.
struct Rec {
    double sums[kSums];
    double best_w;                            // before normalising
    double best_pose[3];
    uint64_t K, r0;
    int32_t best, resampled;
};

struct InitHdr { double mean[3], sigma[3]; double inv_n; uint64_t seed; int32_t N, pad; };

__host__ __device__ inline void init_particle(const InitHdr& I, int32_t j, double& x, double& y, double& yaw) {
    const double g0 = normal(key(I.seed, 0, (uint64_t)j, 0)), g1 = normal(key(I.seed, 0, (uint64_t)j, 1)), g2 = normal(key(I.seed, 0, (uint64_t)j, 2));
    x = I.mean[0] + I.sigma[0] * g0;
    y = I.mean[1] + I.sigma[1] * g1;
    yaw = wrap(I.mean[2] + I.sigma[2] * g2);
}

// sample_motion_model_odometry for particle j: the noise is subtracted; a zero step leaves the bytes alone.
__host__ __device__ inline void move_particle(const Hdr& H, int32_t j, double& x, double& y, double& yaw) {
    const double g0 = normal(key(H.seed, H.update, (uint64_t)j, 0)), g1 = normal(key(H.seed, H.update, (uint64_t)j, 1)),
                 g2 = normal(key(H.seed, H.update, (uint64_t)j, 2));
    const double r1 = H.M.rot1 - H.M.s_r1 * g0;
    const double th = H.M.trans - H.M.s_t * g1;
    const double r2 = H.M.rot2 - H.M.s_r2 * g2;
    if (th != 0.0) {
        double s, c;
        sincos_any(yaw + r1, s, c);
        x = x + th * c;
        y = y + th * s;
    }
    const double dyaw = r1 + r2;
    if (dyaw != 0.0) yaw = wrap(yaw + dyaw);
}

__host__ __device__ inline double weight_factor(int64_t Q) { return 1.0 + (double)Q / kTwo40; }

// The nine terms particle (w, x, y, cos, sin) adds to the sums.
__host__ __device__ inline void sum_terms(double w, double x, double y, double c, double s, double t[kSums]) {
    const double wx = w * x, wy = w * y;
    t[0] = w; t[1] = w * w; t[2] = wx; t[3] = wy; t[4] = w * c; t[5] = w * s; t[6] = wx * x; t[7] = wx * y; t[8] = wy * y;
}

__host__ __device__ inline bool gate_open(int32_t gate, double W, double S2, double ratio_n) { return gate != 0 && (W * W) / S2 < ratio_n; }

__host__ __device__ inline uint64_t count_of(double w) { return (uint64_t)::floor(w * kTwo40); }

// ---------------------------------------------------------------- host only

inline int32_t pow2_at_least(int32_t n) { int32_t p = 1; while (p < n) p *= 2; return p; }

// The adjacent-pair tree over a (its size a power of two).
inline double tree_sum(std::vector<double>& a) {
    for (size_t n = a.size(); n > 1; n /= 2)
        for (size_t i = 0; i < n / 2; ++i) a[i] = a[2 * i] + a[2 * i + 1];
    return a[0];
}

inline bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

// v_occ, R, T and the table; VISFS_BA_OK or the refusal with `why`.
inline int field_plan(const visfs_mcl_field_params& p, double res, const std::vector<double>& cost, int32_t& v_occ, int32_t& R, int32_t& T,
                      std::vector<int64_t>& q, const char** why) {
    if (!finite_pos(p.occupied_probability) || !finite_pos(p.max_dist) || !finite_pos(p.z_hit) || !finite_pos(p.z_rand) ||
        !finite_pos(p.sigma_hit) || !finite_pos(p.range_max) || p.occupied_probability > 1.0) {
        *why = "every field parameter must be finite and positive, occupied_probability at most 1"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    const double d = p.max_dist / res;
    if (!(d < (double)(VISFS_MCL_MAX_RADIUS + 1))) { *why = "max_dist spans more than 255 cells"; return VISFS_BA_ERR_UNSUPPORTED; }
    const double t = std::ceil(d * d);
    if (!(t <= 65535.0)) { *why = "(max_dist / resolution)^2 exceeds 65535"; return VISFS_BA_ERR_UNSUPPORTED; }
    R = (int32_t)std::floor(d); T = (int32_t)t;
    v_occ = 0;
    for (int32_t v = 1; v < 32768; ++v) if (1.0 - cost[(size_t)v] >= p.occupied_probability) v_occ = v;
    q.assign((size_t)T + 1, 0);
    const double two_s2 = 2.0 * (p.sigma_hit * p.sigma_hit), floor_ = p.z_rand / p.range_max;
    for (int32_t i = 0; i <= T; ++i) {
        const double z = i < T ? res * std::sqrt((double)i) : p.max_dist;
        const double pz = p.z_hit * std::exp(-(z * z) / two_s2) + floor_;
        const double v = (pz * pz * pz) * kTwo40;
        if (!(v <= 281474976710656.0)) { *why = "pz^3 2^40 exceeds 2^48: the beam sums would not fit"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        q[(size_t)i] = (int64_t)std::llround(v);
    }
    return VISFS_BA_OK;
}

// rot1, trans, rot2 and their deviations from (dx, dy, dyaw); VISFS_BA_OK or the refusal.
inline int motion_plan(const visfs_mcl_params& p, const double d[3], Motion& M, const char** why) {
    const double a[4] = { p.alpha1, p.alpha2, p.alpha3, p.alpha4 };
    for (double v : a) if (!(std::isfinite(v) && v >= 0.0)) { *why = "the alphas must be finite and not negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (!std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2]) || std::fabs(d[0]) > 1e6 || std::fabs(d[1]) > 1e6) {
        *why = "the odometry delta is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    M.trans = std::sqrt(d[0] * d[0] + d[1] * d[1]);
    M.rot1 = M.trans < 0.01 ? 0.0 : std::atan2(d[1], d[0]);
    if (!(std::fabs(d[2]) <= kTwoPi)) { *why = "the yaw delta exceeds 2 pi"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    M.rot2 = d[2] - M.rot1;                   // not wrapped: rot1 + rot2 stays the yaw delta, also when driving backwards
    // AMCL's diff model: the noise grows with the rotation away from straight ahead or straight back, whichever is nearer
    const double w2 = std::fabs(wrap(M.rot2));
    const double n1 = std::fmin(std::fabs(M.rot1), kPi - std::fabs(M.rot1)), n2 = std::fmin(w2, kPi - w2);
    M.s_r1 = std::sqrt(a[0] * (n1 * n1) + a[1] * (M.trans * M.trans));
    M.s_t = std::sqrt((a[2] * (M.trans * M.trans) + a[3] * (n1 * n1)) + a[3] * (n2 * n2));
    M.s_r2 = std::sqrt(a[0] * (n2 * n2) + a[1] * (M.trans * M.trans));
    // |g| <= 6, so the noisy yaw step stays within 2 pi and a yaw in (-pi, pi] needs one wrap at the most
    if (!(std::fabs(M.rot1 + M.rot2) + 6.0 * (M.s_r1 + M.s_r2) <= kTwoPi)) {
        *why = "|rot1 + rot2| + 6 (sigma_rot1 + sigma_rot2) exceeds 2 pi: the yaw could need more than one wrap"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    return VISFS_BA_OK;
}

// The host's end of an update, shared by the device path and the twin: mean, covariance and n_eff from the nine sums.
inline void finalize(const Rec& r, int32_t n_beams, int64_t update, visfs_mcl_result& out) {
    const double* S = r.sums;
    const double W = S[0];
    out = visfs_mcl_result();
    out.status = VISFS_BA_OK;
    out.resampled = r.resampled; out.best = r.best; out.n_beams = n_beams; out.update = update;
    const double mx = S[2] / W, my = S[3] / W, mc = S[4] / W, ms = S[5] / W;
    out.mean[0] = mx; out.mean[1] = my; out.mean[2] = std::atan2(S[5], S[4]);
    out.covariance[0] = S[6] / W - mx * mx;
    out.covariance[1] = out.covariance[3] = S[7] / W - mx * my;
    out.covariance[4] = S[8] / W - my * my;
    const double len = std::sqrt(mc * mc + ms * ms);
    out.covariance[8] = len < 1.0 ? (len > 0.0 ? -2.0 * std::log(len) : HUGE_VAL) : 0.0;
    out.n_eff = (W * W) / S[1];
    out.W = W;
    for (int i = 0; i < 3; ++i) out.best_pose[i] = r.best_pose[i];
    out.best_weight = r.best_w / W;
}

}  // namespace mcl
