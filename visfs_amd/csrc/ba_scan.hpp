// Correlative scan matching on the laser sub-maps (include/visfs_scan_match.h): what the kernels of
// ba_scan.hip and the one-core host twin share, the search set-up (host doubles), and Estimator::laserPretreatment.
//
// Unlike the insertion path (ba_submap.hpp: "the device sees integers"), the rotation and discretisation of a point runs on the
// device: S * n of them per call would otherwise be formed on the host and uploaded.  It is one __host__ __device__ function,
// built without contraction, of + - * / and a rounding, which the twin calls as well; every transcendental (acos, cos, sin, exp,
// hypot) is evaluated on the host and reaches the device as a table.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ba_submap_access.hpp"
#include "../../include/visfs_scan_match.h"

#pragma clang fp contract(off)

namespace scan {

constexpr int kThreads = 256;                 // work items of one workgroup of k_scan_score: candidates x point slices
constexpr int kChunk = 1024;                  // points whose cells one workgroup stages in LDS at a time
constexpr int32_t kMaxValue = 32767;          // value of the maximal correspondence cost = the minimal probability
constexpr int32_t kCellClamp = 1 << 30;       // a discretised index saturates here (far outside any grid either way)
constexpr double kKappa = 0.8 / 32766.0;      // probability per value step: (kMaxProbability - kMinProbability) / 32766

// ---------------------------------------------------------------- shared by the kernels and the twin

// lround(v) for |v| < 2^30, saturating beyond (a guess far away must not overflow the index arithmetic)
__host__ __device__ inline int32_t round_index(double v) {
    const double r = ::round(v);
    if (r >= (double)kCellClamp) return kCellClamp;
    if (r <= -(double)kCellClamp) return -kCellClamp;
    return (int32_t)r;
}

// Point (px, py) of the scan rotated by (c, s) = (cos a_k, sin a_k) about the guess (gx, gy), and its cell:
// MapLimits::getCellIndex (submap::cell_index) on the limits in force.
__host__ __device__ inline void discretise(double c, double s, double px, double py, double gx, double gy, double res, double max_x,
                                           double max_y, int32_t& ix, int32_t& iy) {
    const double X = (c * px - s * py) + gx;
    const double Y = (s * px + c * py) + gy;
    ix = round_index((max_y - Y) / res - 0.5);
    iy = round_index((max_x - X) / res - 0.5);
}

using submap::GridView;

// 32767 - eff(v): what one point adds to a candidate's sum.  Unknown (0) and outside read as the minimal probability: nothing.
__host__ __device__ inline int32_t cell_gain(const GridView& g, int32_t x, int32_t y) {
    x -= g.ox; y -= g.oy;
    if (x < 0 || y < 0 || x >= g.nx || y >= g.ny) return 0;
    const int32_t v = g.cells[(int64_t)y * g.nx + x];
    return v == 0 ? 0 : kMaxValue - (v & kMaxValue);
}

__host__ __device__ inline int32_t iabs(int32_t v) { return v < 0 ? -v : v; }

// index of candidate (k, xo, yo)'s weight in the table [na + 1][nl + 1][nl + 1] over (|k - na|, |xo|, |yo|)
__host__ __device__ inline int32_t weight_index(int32_t na, int32_t nl, int32_t k, int32_t xo, int32_t yo) {
    return (iabs(k - na) * (nl + 1) + iabs(xo)) * (nl + 1) + iabs(yo);
}

// mean probability of the n cells times the candidate's weight, in this order
__host__ __device__ inline double candidate_score(int32_t Q, int32_t n, double w) {
    return (0.1 + ((double)Q * kKappa) / (double)n) * w;
}

// max_element's order: the larger score, and among equal scores the earlier candidate
__host__ __device__ inline bool better(double sa, int32_t ia, double sb, int32_t ib) { return sa > sb || (sa == sb && ia < ib); }

// ---------------------------------------------------------------- the search of one call (host doubles)
struct Plan {
    submap::Limits L;                         // the limits in force at the call
    double gx = 0.0, gy = 0.0, gyaw = 0.0;
    int32_t n = 0, na = 0, nl = 0, S = 0, Lw = 0;
    double step = 0.0;
    std::vector<double> pts;                  // [n][2]
    std::vector<double> rot;                  // [S][2]: cos a_k, sin a_k
    std::vector<double> weight;               // [na + 1][nl + 1][nl + 1]
    int64_t candidates() const { return (int64_t)S * Lw * Lw; }
};

// Returns VISFS_BA_OK, VISFS_BA_ERR_UNSUPPORTED when the search exceeds a limit, or VISFS_BA_ERR_BAD_ARGUMENT when the weights make a
// candidate's weight NaN (`why` says which).  Arguments already checked finite.
// The two halves of a plan that the branch-and-bound matcher (ba_scan_fast.hip) forms in the same way: the search's angular step and
// its half-widths as doubles (the caller holds them to its own limits before they become integers) ...
inline bool plan_search(double res, double linear_window, double angular_window, int32_t n, const double* xyz, double& step, double& fa,
                        double& fl) {
    double max_range = 3.0 * res;
    for (int32_t i = 0; i < n; ++i) {
        const double px = xyz[3 * i], py = xyz[3 * i + 1];
        const double r = std::sqrt(px * px + py * py);
        if (r > max_range) max_range = r;
    }
    if (!std::isfinite(max_range)) return false;
    step = (1.0 - 1e-3) * std::acos(1.0 - (res * res) / (2.0 * (max_range * max_range)));
    fa = std::ceil(angular_window / step); fl = std::ceil(linear_window / res);
    return true;
}

// ... and, once P.n, P.na, P.S, P.gyaw and P.step stand, the points' x, y and the rotation table
inline void plan_tables(const double* xyz, Plan& P) {
    P.pts.resize(2 * (size_t)P.n);
    for (int32_t i = 0; i < P.n; ++i) { P.pts[2 * i] = xyz[3 * i]; P.pts[2 * i + 1] = xyz[3 * i + 1]; }
    P.rot.resize(2 * (size_t)P.S);
    for (int32_t k = 0; k < P.S; ++k) {
        const double a = P.gyaw + (double)(k - P.na) * P.step;
        P.rot[2 * k] = std::cos(a); P.rot[2 * k + 1] = std::sin(a);
    }
}

inline int make_plan(const submap::Limits& L, const visfs_scan_match_params& p, const double g[3], int32_t n, const double* xyz, Plan& P,
                     const char** why) {
    P.L = L; P.gx = g[0]; P.gy = g[1]; P.gyaw = g[2]; P.n = n;
    const double res = L.res;
    double step, fa, fl;
    if (!plan_search(res, p.linear_search_window, p.angular_search_window, n, xyz, step, fa, fl)) { *why = "the scan's range overflows"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (!(fl <= (double)VISFS_SCAN_MATCH_MAX_LINEAR)) { *why = "the linear window spans more than 32 cells"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (!(2.0 * fa + 1.0 <= (double)VISFS_SCAN_MATCH_MAX_SCANS)) { *why = "the angular window holds more than 1025 rotations"; return VISFS_BA_ERR_UNSUPPORTED; }
    P.step = step; P.na = (int32_t)fa; P.nl = (int32_t)fl; P.S = 2 * P.na + 1; P.Lw = 2 * P.nl + 1;
    if (P.candidates() > (int64_t)VISFS_SCAN_MATCH_MAX_CANDIDATES) { *why = "more than 2^21 candidates"; return VISFS_BA_ERR_UNSUPPORTED; }
    plan_tables(xyz, P);
    const int32_t m = P.nl + 1;
    P.weight.resize((size_t)(P.na + 1) * m * m);
    for (int32_t ka = 0; ka <= P.na; ++ka)
        for (int32_t ax = 0; ax <= P.nl; ++ax)
            for (int32_t ay = 0; ay <= P.nl; ++ay) {
                const double cx = (double)ay * res, cy = (double)ax * res;        // |-yo res|, |-xo res|
                const double t = std::hypot(cx, cy) * p.translation_delta_cost_weight + ((double)ka * step) * p.rotation_delta_cost_weight;
                const double w = std::exp(-(t * t));
                if (!std::isfinite(w)) { *why = "the cost weights overflow"; return VISFS_BA_ERR_BAD_ARGUMENT; }      // no NaN score
                P.weight[((size_t)ka * m + ax) * m + ay] = w;
            }
    return VISFS_BA_OK;
}

// the result record from the winner's (candidate index, score, Q)
inline void fill_result(const Plan& P, int32_t idx, double score, int32_t Q, visfs_scan_match_result& r) {
    const int32_t L = P.Lw;
    const int32_t k = idx / (L * L), xo = (idx / L) % L - P.nl, yo = idx % L - P.nl;
    r.matched = 1;
    r.x = P.gx + (double)(-yo) * P.L.res;         // the cell x index runs along -y
    r.y = P.gy + (double)(-xo) * P.L.res;
    r.yaw = P.gyaw + (double)(k - P.na) * P.step;
    r.score = score; r.sum = Q;
    r.scan_index = k; r.x_offset = xo; r.y_offset = yo;
    r.num_scans = P.S; r.num_linear = P.nl; r.angular_step = P.step;
}

// ---------------------------------------------------------------- Estimator::laserPretreatment (Estimator.cpp:116-157)

// Isometry3d * Vector3d, all three rows, in submap::transform_xy's order
inline void transform_xyz(const double T[12], const double p[3], double o[3]) {
    for (int r = 0; r < 3; ++r) o[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
}

// 600 points at ten flops each: a loop on the host, no launch.
inline void pretreat(const visfs_scan_pretreat_params& p, const double T[12], const double origin[3], int32_t n, const double* xyz,
                     double* ret, double* mis, visfs_range_data* rd, int32_t* n_out) {
    int32_t nrd = 0;
    size_t nr = 0, nm = 0;
    double o[3];
    transform_xyz(T, origin, o);                                                   // every subdivision starts from the cloud's origin
    for (int32_t i = 0; i < p.num_subdivisions; ++i) {
        const size_t a = (size_t)n * (size_t)i / (size_t)p.num_subdivisions, b = (size_t)n * (size_t)(i + 1) / (size_t)p.num_subdivisions;
        if (a == b) continue;
        visfs_range_data& d = rd[nrd++];
        for (int c = 0; c < 3; ++c) d.origin[c] = o[c];
        d.returns = ret + 3 * nr; d.misses = mis + 3 * nm;
        d.n_returns = 0; d.n_misses = 0;
        for (size_t j = a; j < b; ++j) {
            double q[3];
            transform_xyz(T, xyz + 3 * j, q);
            const double dx = q[0] - o[0], dy = q[1] - o[1], dz = q[2] - o[2];
            const double range = std::sqrt((dx * dx + dy * dy) + dz * dz);         // Vector3d::norm
            if (!(range >= p.min_range)) continue;
            if (range <= p.max_range) {
                for (int c = 0; c < 3; ++c) ret[3 * nr + c] = q[c];
                ++nr; ++d.n_returns;
            } else {
                const double f = p.missing_ray_length / range;
                mis[3 * nm] = o[0] + f * dx; mis[3 * nm + 1] = o[1] + f * dy; mis[3 * nm + 2] = o[2] + f * dz;
                ++nm; ++d.n_misses;
            }
        }
    }
    *n_out = nrd;
}

}  // namespace scan
