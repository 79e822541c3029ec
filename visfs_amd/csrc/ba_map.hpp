// A global occupancy map composed from frozen sub-maps (include/visfs_map.h): the definition of a composed
// cell, which k_map_compose and the one-core twin of ba_map.hip both call, and the host plan of a compose (limits, culling boxes).
//
// As in ba_scan.hpp, the cosine and sine of every tile's yaw are formed on the host; the device evaluates + - * / and a rounding,
// in one __host__ __device__ function built without contraction.  The log-odds table is integers built once on the host, so the
// sum over the tiles has no order.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ba_scan.hpp"
#include "../../include/visfs_map.h"

#pragma clang fp contract(off)

namespace gmap {

constexpr int kBlockX = 64, kBlockY = 4;      // output cells of one workgroup: a wavefront per row of 64
constexpr int kThreads = kBlockX * kBlockY;
constexpr int kValues = 32768;
constexpr int kBoxMargin = 2;                 // output cells a tile's box is widened by on every side

// One tile as a compose reads it: the rotation, the translation, the frozen limits, the cells [ny][nx] (markers stripped, in the
// memory of the map's flavour) and its box in output cells (inclusive; bx0 > bx1: the tile misses the grid).
struct TileRec {
    double c, s, x, y;
    double res, max_x, max_y;
    const uint16_t* cells;
    int32_t nx, ny;
    int32_t bx0, by0, bx1, by1;
};

// Tile cell (x, y) of its limits from the sub-map's allocation: the update marker stripped; outside the allocation unknown.
__host__ __device__ inline uint16_t frozen_cell(const submap::GridView& g, int32_t x, int32_t y) {
    x -= g.ox; y -= g.oy;
    if (x < 0 || y < 0 || x >= g.nx || y >= g.ny) return 0;
    return (uint16_t)(g.cells[(int64_t)y * g.nx + x] & 32767);
}

// The value of tile `t` at the map point (X, Y): 0 when the point lies outside the tile or in an unknown cell.
__host__ __device__ inline int32_t tile_sample(const TileRec& t, double X, double Y) {
    const double dx = X - t.x, dy = Y - t.y;
    const double px = t.c * dx + t.s * dy, py = t.c * dy - t.s * dx;
    const int32_t jx = scan::round_index((t.max_y - py) / t.res - 0.5);
    const int32_t jy = scan::round_index((t.max_x - px) / t.res - 0.5);
    if (jx < 0 || jy < 0 || jx >= t.nx || jy >= t.ny) return 0;
    return (int32_t)(t.cells[(int64_t)jy * t.nx + jx] & 32767);
}

// The v in 1 .. 32767 whose L[v] is nearest to S (L strictly decreasing, L[32767] <= S <= L[1]); of two equally near, the smaller.
__host__ __device__ inline int32_t odds_inverse(const int32_t* __restrict__ L, int32_t S) {
    int32_t lo = 1, hi = kValues - 1;         // the smallest v with L[v] <= S
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (L[mid] <= S) hi = mid; else lo = mid + 1;
    }
    if (lo > 1 && L[lo - 1] - S <= S - L[lo]) return lo - 1;
    return lo;
}

// Output cell (ix, iy) of the grid (max_x, max_y, res) from the tiles in increasing index.  (bx, by) is the first cell of the
// block of kBlockX x kBlockY cells the cell lies in: a tile whose box misses the block is skipped, which drops no cell the sample
// would accept (make_plan).  On the device the test reads scalars only: it is uniform over the workgroup.
__host__ __device__ inline void compose_cell(const TileRec* __restrict__ tiles, int32_t nt, const int32_t* __restrict__ L, int32_t combine,
                                             double max_x, double max_y, double res, int32_t bx, int32_t by, int32_t ix, int32_t iy,
                                             uint16_t& value, uint8_t& count) {
    const double X = max_x - ((double)iy + 0.5) * res;
    const double Y = max_y - ((double)ix + 0.5) * res;
    int32_t n = 0, sum = 0, latest = 0, least = kValues;
    for (int32_t k = 0; k < nt; ++k) {
        const TileRec& t = tiles[k];
        if (t.bx0 > bx + (kBlockX - 1) || t.bx1 < bx || t.by0 > by + (kBlockY - 1) || t.by1 < by) continue;
        const int32_t v = tile_sample(t, X, Y);
        if (v == 0) continue;
        ++n;
        latest = v;
        if (v < least) least = v;
        if (combine == VISFS_MAP_ODDS) sum += L[v];
    }
    count = (uint8_t)(n > 255 ? 255 : n);
    if (n == 0) { value = 0; return; }
    if (n == 1 || combine == VISFS_MAP_LATEST) { value = (uint16_t)latest; return; }      // one tile: its value, in every mode
    if (combine == VISFS_MAP_OCCUPIED) { value = (uint16_t)least; return; }
    const int32_t top = L[1], bottom = L[kValues - 1];
    const int32_t S = sum > top ? top : (sum < bottom ? bottom : sum);
    value = (uint16_t)odds_inverse(L, S);
}

// ---------------------------------------------------------------- the host plan (host doubles, no launch)

struct PlanTile {
    submap::Limits L;
    double pose[3] = { 0.0, 0.0, 0.0 };
};

struct Plan {
    submap::Limits G;                         // the composed grid
    std::vector<TileRec> recs;                // per tile; `cells` left null
    submap::Box known;                        // the union of the boxes
    int32_t drawn = 0;
};

inline bool limits_ok(double res, double max_x, double max_y, int32_t nx, int32_t ny) {
    return std::isfinite(res) && res > 0.0 && std::isfinite(max_x) && std::isfinite(max_y) && nx >= 1 && ny >= 1;
}

// The four corners of a tile's extent in the map frame, in the order of the definition.
inline void tile_corners(const PlanTile& t, double c, double s, double gx[4], double gy[4]) {
    const double x0 = t.L.max_x, x1 = t.L.max_x - (double)t.L.ny * t.L.res;
    const double y0 = t.L.max_y, y1 = t.L.max_y - (double)t.L.nx * t.L.res;
    const double px[4] = { x0, x1, x0, x1 }, py[4] = { y0, y0, y1, y1 };
    for (int i = 0; i < 4; ++i) {
        gx[i] = (c * px[i] - s * py[i]) + t.pose[0];
        gy[i] = (s * px[i] + c * py[i]) + t.pose[1];
    }
}

// One axis of a box: the fractional output indices [mn, mx] widened by kBoxMargin cells and cut to [0, n - 1]; false: empty.
inline bool box_axis(double mn, double mx, int32_t n, int32_t& lo, int32_t& hi) {
    double a = std::floor(mn) - (double)kBoxMargin, b = std::ceil(mx) + (double)kBoxMargin;
    if (!(a >= 0.0)) a = 0.0;                 // a NaN widens, it never drops
    if (!(b <= (double)(n - 1))) b = (double)(n - 1);
    if (a > b) return false;
    lo = (int32_t)a; hi = (int32_t)b;
    return true;
}

// Returns VISFS_BA_OK, or the refusal with `why`.  The tiles' limits and poses are already checked finite.
inline int make_plan(const visfs_map_params& p, const std::vector<PlanTile>& tiles, Plan& P, const char** why) {
    if (p.combine != VISFS_MAP_ODDS && p.combine != VISFS_MAP_LATEST && p.combine != VISFS_MAP_OCCUPIED) { *why = "unknown combine"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    const size_t n = tiles.size();
    P = Plan();
    P.recs.resize(n);
    std::vector<double> gx(4 * n), gy(4 * n);
    for (size_t k = 0; k < n; ++k) {
        TileRec& r = P.recs[k];
        const PlanTile& t = tiles[k];
        r.c = std::cos(t.pose[2]); r.s = std::sin(t.pose[2]); r.x = t.pose[0]; r.y = t.pose[1];
        r.res = t.L.res; r.max_x = t.L.max_x; r.max_y = t.L.max_y; r.nx = t.L.nx; r.ny = t.L.ny; r.cells = nullptr;
        tile_corners(t, r.c, r.s, &gx[4 * k], &gy[4 * k]);
    }
    submap::Limits& G = P.G;
    if (p.explicit_limits == 1) {
        const visfs_submap_info& l = p.limits;
        if (!limits_ok(l.resolution, l.max_x, l.max_y, l.num_x_cells, l.num_y_cells)) {
            *why = "the limits need a positive resolution, a finite corner and at least one cell per axis"; return VISFS_BA_ERR_BAD_ARGUMENT;
        }
        G.res = l.resolution; G.max_x = l.max_x; G.max_y = l.max_y; G.nx = l.num_x_cells; G.ny = l.num_y_cells;
    } else if (p.explicit_limits == 0) {
        if (!(std::isfinite(p.resolution) && p.resolution > 0.0)) { *why = "the resolution must be finite and positive"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        if (n == 0) { *why = "no tile to take the limits from"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        double lo_x = gx[0], hi_x = gx[0], lo_y = gy[0], hi_y = gy[0];
        for (size_t i = 1; i < 4 * n; ++i) {
            if (gx[i] < lo_x) lo_x = gx[i];
            if (gx[i] > hi_x) hi_x = gx[i];
            if (gy[i] < lo_y) lo_y = gy[i];
            if (gy[i] > hi_y) hi_y = gy[i];
        }
        const double res = p.resolution;
        const double cx = std::ceil(hi_x / res), fx = std::floor(lo_x / res), cy = std::ceil(hi_y / res), fy = std::floor(lo_y / res);
        const double ny = cx - fx, nx = cy - fy;
        G.res = res; G.max_x = cx * res; G.max_y = cy * res;
        if (!(ny <= (double)VISFS_MAP_MAX_CELLS) || !(nx <= (double)VISFS_MAP_MAX_CELLS) || !std::isfinite(G.max_x) || !std::isfinite(G.max_y)) {
            *why = "the composed grid exceeds 2^26 cells"; return VISFS_BA_ERR_UNSUPPORTED;
        }
        G.nx = (int32_t)nx; G.ny = (int32_t)ny;
        if (G.nx < 1 || G.ny < 1) { *why = "the tiles span less than one cell"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    } else { *why = "explicit_limits must be 0 or 1"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if ((int64_t)G.nx * G.ny > (int64_t)VISFS_MAP_MAX_CELLS) { *why = "the composed grid exceeds 2^26 cells"; return VISFS_BA_ERR_UNSUPPORTED; }
    for (size_t k = 0; k < n; ++k) {
        TileRec& r = P.recs[k];
        double mn_x = 0.0, mx_x = 0.0, mn_y = 0.0, mx_y = 0.0;
        for (int i = 0; i < 4; ++i) {
            const double fx = (G.max_y - gy[4 * k + i]) / G.res - 0.5;          // the output x index runs along -y
            const double fy = (G.max_x - gx[4 * k + i]) / G.res - 0.5;
            if (i == 0) { mn_x = mx_x = fx; mn_y = mx_y = fy; continue; }
            if (!(fx >= mn_x)) mn_x = fx;
            if (!(fx <= mx_x)) mx_x = fx;
            if (!(fy >= mn_y)) mn_y = fy;
            if (!(fy <= mx_y)) mx_y = fy;
        }
        if (box_axis(mn_x, mx_x, G.nx, r.bx0, r.bx1) && box_axis(mn_y, mx_y, G.ny, r.by0, r.by1)) {
            ++P.drawn;
            P.known.extend(r.bx0, r.by0); P.known.extend(r.bx1, r.by1);
        } else { r.bx0 = r.by0 = 1; r.bx1 = r.by1 = 0; }
    }
    return VISFS_BA_OK;
}

inline void fill_info(const Plan& P, visfs_submap_info& l) {
    l = visfs_submap_info();
    l.resolution = P.G.res; l.max_x = P.G.max_x; l.max_y = P.G.max_y; l.num_x_cells = P.G.nx; l.num_y_cells = P.G.ny;
    l.known_min_x = P.known.min_x; l.known_min_y = P.known.min_y; l.known_max_x = P.known.max_x; l.known_max_y = P.known.max_y;
}

}  // namespace gmap
