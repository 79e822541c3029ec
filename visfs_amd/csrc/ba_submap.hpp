// Laser sub-maps (ActiveSubmaps2D + ProbabilityGrid, Submap2D.cpp / ProbabilityGridRangeDataInserter2D.cpp / RayToPixelMask.cpp):
// the per-item functions the kernels of ba_submap.hip and the host restatement (visfs_submaps_create_host, the hooks) share.
//
// Every double of an insertion (point transform, superscaled cell index, growth, the crop's value -> probability -> value round trip)
// is formed on the host, once, by the functions below; the device sees integers and the tables built from them.  So there is no
// product a device compiler could fuse, and the host restatement and the device path read the same integers by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/visfs_submap.h"

struct visfs_ba_handle;
struct visfs_ba_window;
struct visfs_ba_result;

namespace submap {

constexpr int kSubpixelScale = 1000;          // ProbabilityGridRangeDataInserter2D.cpp:13
constexpr uint16_t kUpdateMarker = 1u << 15;  // ProbabilityValues.h
constexpr int kValueCount = 32768;
constexpr int kInitialSubmapSize = 100;       // Submap2D.cpp (createGrid)
constexpr int kCellsPerItem = 8;              // cells of one ray column one work item walks at most
constexpr int kMaxBatch = 32;                 // insertions per batch: one bit each in the per-cell marks

constexpr double kMinProbability = 0.1;
constexpr double kMaxProbability = 1.0 - kMinProbability;
constexpr double kMinCorrespondenceCost = 1.0 - kMaxProbability;
constexpr double kMaxCorrespondenceCost = 1.0 - kMinProbability;

// MapLimits (MapLimits.h:43-85): resolution, max corner, cell counts
struct Limits {
    double res = 0.0, max_x = 0.0, max_y = 0.0;
    int32_t nx = 0, ny = 0;
};

inline Limits limits_of(const visfs_submap_info& l) {
    Limits L;
    L.res = l.resolution; L.max_x = l.max_x; L.max_y = l.max_y; L.nx = l.num_x_cells; L.ny = l.num_y_cells;
    return L;
}

// AlignedBox2i of the known cells; empty as Eigen's default box (min > max)
struct Box {
    int32_t min_x = 1, min_y = 1, max_x = 0, max_y = 0;
    bool empty() const { return min_x > max_x || min_y > max_y; }
    void extend(int32_t x, int32_t y) {
        if (empty()) { min_x = max_x = x; min_y = max_y = y; return; }
        if (x < min_x) min_x = x;
        if (x > max_x) max_x = x;
        if (y < min_y) min_y = y;
        if (y > max_y) max_y = y;
    }
    void extend(const Box& b) { if (!b.empty()) { extend(b.min_x, b.min_y); extend(b.max_x, b.max_y); } }
};

// ---------------------------------------------------------------- host doubles

// Isometry3d * Vector3d: linear() * p + translation(), summed column by column.  Twr row-major 3x4.  Only x, y are used (head<2>).
inline void transform_xy(const double T[12], const double p[3], double& x, double& y) {
    x = ((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[3];
    y = ((T[4] * p[0] + T[5] * p[1]) + T[6] * p[2]) + T[7];
}

// MapLimits::getCellIndex: the x index comes from y and the y index from x
inline void cell_index(double res, double max_x, double max_y, double px, double py, int32_t& ix, int32_t& iy) {
    ix = (int32_t)std::lround((max_y - py) / res - 0.5);
    iy = (int32_t)std::lround((max_x - px) / res - 0.5);
}
inline bool contains(const Limits& L, int32_t ix, int32_t iy) { return ix >= 0 && iy >= 0 && ix < L.nx && iy < L.ny; }

// The superscaled limits (ProbabilityGridRangeDataInserter2D.cpp:28-36): resolution / kSubpixelScale, same max.  getCellIndex does
// not read the cell counts, so only the resolution changes.
inline void superscaled_index(const Limits& L, double px, double py, int32_t& ix, int32_t& iy) {
    const double sres = L.res / kSubpixelScale;
    cell_index(sres, L.max_x, L.max_y, px, py, ix, iy);
}

// One step of Grid2D::growLimits (Grid2d.cpp:34-65): doubles the grid around its centre; (xoff, yoff) is where the old cell (0, 0)
// lands.  Returns false when `p` is already inside.
inline bool grow_step(Limits& L, double px, double py, int32_t& xoff, int32_t& yoff) {
    int32_t ix, iy;
    cell_index(L.res, L.max_x, L.max_y, px, py, ix, iy);
    if (contains(L, ix, iy)) return false;
    xoff = L.nx / 2; yoff = L.ny / 2;
    L.max_x = L.max_x + L.res * (double)yoff;                // max + resolution * Vector2d(yOffset, xOffset)
    L.max_y = L.max_y + L.res * (double)xoff;
    L.nx = 2 * L.nx; L.ny = 2 * L.ny;
    return true;
}

// ---------------------------------------------------------------- shared integer work items (host and device)

__host__ __device__ inline int64_t floor_div(int64_t a, int64_t d) {        // d > 0
    int64_t q = a / d;
    if ((a % d) != 0 && a < 0) --q;
    return q;
}
__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t d) { return -floor_div(-a, d); }

// A ray of rayToPixelMask (RayToPixelMask.cpp) in superscaled cells, its endpoints ordered by x as the reference orders them.
struct Ray { int32_t bx, by, ex, ey; };

__host__ __device__ inline Ray ray_make(int32_t bx, int32_t by, int32_t ex, int32_t ey) {
    if (bx > ex) return Ray{ ex, ey, bx, by };
    return Ray{ bx, by, ex, ey };
}
__host__ __device__ inline int32_t ray_columns(const Ray& r, int S = kSubpixelScale) { return r.ex / S - r.bx / S + 1; }

// Cells one column may hold, at most (sizes the work items of a column): exact for the vertical case; otherwise the smaller of two
// upper bounds: a column's share of the y travel, |dy| / dx cells, plus the two partial cells at its ends, and the rows between the
// ray's own end cells (a steep ray that crosses one column border has a huge |dy| / dx and a few tens of rows).
__host__ __device__ inline int32_t ray_max_span(const Ray& r, int S = kSubpixelScale) {
    const int32_t a = r.by / S, b = r.ey / S;
    const int64_t rows = (int64_t)(a > b ? a - b : b - a) + 1;
    if (r.bx / S == r.ex / S) return (int32_t)rows;
    const int64_t dx = (int64_t)r.ex - r.bx, dy = (int64_t)r.ey - r.by;
    const int64_t ady = dy < 0 ? -dy : dy;
    const int64_t slope = ady / dx + 2;
    return (int32_t)(slope < rows ? slope : rows);
}

// Column j (0 .. ray_columns - 1) of the ray: its x and the first and last y in the reference's stepping order (step +1 or -1).
// Closed form of the stepping loop: the loop's running sub-pixel value `subY`, never reduced, is G(c) at the right border of column c
// (c < endX) and G(endX) at the end point; the loop leaves column c on y0 + floor(G(c) / den) when dy > 0 and y0 + ceil(G(c) / den) - 1
// otherwise, and reaches y0 + ceil(G(c) / den) - 1, resp. y0 + floor(G(c) / den), inside it.  Both ends inclusive.
// S: the sub-pixel scale (kSubpixelScale in the inserter; the reference's unit tests also use other scales).
__host__ __device__ inline void ray_column(const Ray& r, int32_t j, int32_t& x, int32_t& y_first, int32_t& y_last, int32_t& step,
                                           int S = kSubpixelScale) {
    const int32_t x0 = r.bx / S;
    x = x0 + j;
    if (x0 == r.ex / S) {                                   // special case: vertical line
        const int32_t lo = (r.by < r.ey ? r.by : r.ey) / S, hi = (r.by < r.ey ? r.ey : r.by) / S;
        y_first = lo; y_last = hi; step = 1;
        return;
    }
    const int64_t dx = (int64_t)r.ex - r.bx;
    const int64_t dy = (int64_t)r.ey - r.by;
    const int64_t den = 2 * (int64_t)S * dx;
    const int32_t y0 = r.by / S;
    const int32_t endX = r.ex / S;
    const int first_pixel = 2 * S - 2 * (r.bx % S) - 1;
    const int last_pixel = 2 * (r.ex % S) + 1;
    const int64_t G0 = (int64_t)(2 * (r.by % S) + 1) * dx + dy * first_pixel;
    auto G = [&](int32_t c) -> int64_t {                    // c in [x0, endX]
        if (c < endX) return G0 + (int64_t)(c - x0) * (dy * 2 * S);
        return G0 + (int64_t)(endX - 1 - x0) * (dy * 2 * S) + dy * last_pixel;
    };
    const int64_t g = G(x);
    if (dy > 0) {
        const int64_t start = (j == 0) ? 0 : floor_div(G(x - 1), den);
        int64_t end = ceil_div(g, den) - 1;
        if (end < start) end = start;
        y_first = y0 + (int32_t)start; y_last = y0 + (int32_t)end; step = 1;
    } else {
        const int64_t start = (j == 0) ? 0 : ceil_div(G(x - 1), den) - 1;
        int64_t end = floor_div(g, den);
        if (end > start) end = start;
        y_first = y0 + (int32_t)start; y_last = y0 + (int32_t)end; step = -1;
    }
}

// Work items per column of the ray: chunks of kCellsPerItem cells that cover ray_max_span.
__host__ __device__ inline int32_t ray_nchunk(const Ray& r, int S = kSubpixelScale) { return (ray_max_span(r, S) + kCellsPerItem - 1) / kCellsPerItem; }

// Work item `local` (0 .. ray_columns * nchunk - 1) of the ray: column local / nchunk, chunk local % nchunk of it.  Returns the
// number of cells the item holds (0: the chunk lies past the column's end), at (x, y + step * k), k = 0 .. count - 1.
__host__ __device__ inline int32_t ray_item(const Ray& r, int32_t nchunk, int32_t local, int32_t& x, int32_t& y, int32_t& step,
                                            int S = kSubpixelScale) {
    const int32_t j = local / nchunk, q = local - j * nchunk;
    int32_t y0, y1;
    ray_column(r, j, x, y0, y1, step, S);
    const int32_t n = (y1 - y0) * step + 1;
    const int32_t a = q * kCellsPerItem;
    if (a >= n) return 0;
    y = y0 + step * a;
    return (n < a + kCellsPerItem ? n : a + kCellsPerItem) - a;
}

// ---------------------------------------------------------------- device records of one batch

// One record per return (a hit: one work item) and per ray (return or miss: columns x chunks work items), in final-grid coordinates
// through (ox, oy): the cumulative growth of the sub-map between the insertion's limits and the batch's final limits.
struct MarkRec {
    int32_t bx, by, ex, ey;       // hit: (ex, ey) is the return's superscaled index; ray: ordered endpoints (ray_make)
    int32_t base;                 // first work item
    int32_t nchunk;               // ray: work items per column
    int32_t ox, oy;
    uint32_t flags;               // bit 0-4: insertion within the batch, bit 5: sub-map, bit 6: hit
};

}  // namespace submap

// Internal entry points of ba_api.cpp the sub-maps use (the handle's device, stream and window solve).
hipStream_t visfs_internal_stream(visfs_ba_handle* h);
int visfs_internal_device(visfs_ba_handle* h);
void visfs_internal_set_error(visfs_ba_handle* h, const char* msg);
// visfs_ba_solve_window with the grid's cost array read from device memory `d_cost` (w->grid->correspondence_cost is not read)
int visfs_internal_solve_window(visfs_ba_handle* h, const visfs_ba_window* w, visfs_ba_result* r, const float* d_cost);
