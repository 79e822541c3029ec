// Laser sub-maps resident on the GPU (include/visfs_submap.h).
//
// The reference's ActiveSubmaps2D (Submap2D.cpp:39-103) of ProbabilityGrids, with its range data inserter
// (ProbabilityGridRangeDataInserter2D.cpp) and ray casting (RayToPixelMask.cpp), two ways:
//   * HostSubmaps: the sequential restatement, one core (visfs_submaps_create_host; the parity tests compare against it);
//   * DeviceSubmaps: the grids in HBM, insertions in batches of up to 32 between life-cycle events (add / finish / drop):
//       k_submap_grow   a grown (or new) allocation, old cells moved to their new place, marks cleared
//       k_submap_mark   one work item per return (hit bit) and per (ray, column, chunk of <= 8 cells) (miss bits), atomicOr
//       k_submap_apply  one pass over the batch's box, every sub-map in one launch: per cell the batch's insertions in order
//                       (hit bit -> hit table, else miss bit -> miss table), float cost mirror refreshed, marks cleared
//       k_submap_crop   Submap2D::finish: the known box, value -> probability -> value (a table built on the host)
// A cell changes at most once per insertion and a hit wins over a miss: exactly the reference's update markers, in one pass.
#include "ba_submap.hpp"
#include "ba_submap_access.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_submap.h"

#include <algorithm>
#include <cstring>
#include <deque>
#include <new>
#include <string>
#include <vector>

using namespace submap;
using namespace host;

namespace {

// ---------------------------------------------------------------- value tables (ProbabilityValues.{h,cpp}, ValueConversionTables.cpp)
double clamp_ref(double v, double lo, double hi) { if (v > hi) return hi; if (v < lo) return lo; return v; }   // uClamp
uint16_t bounded_to_value(double v, double lo, double hi) { return (uint16_t)(std::lround((clamp_ref(v, lo, hi) - lo) * (32766.0 / (hi - lo))) + 1); }
double value_to_bounded(int v, double unknown, double lo, double hi) {
    if (v == 0) return unknown;
    const double k = (hi - lo) / 32766.0;
    return v * k + (lo - k);
}
double odds(double p) { return p / (1.0 - p); }
double prob_from_odds(double o) { return o / (o + 1.0); }
uint16_t cost_to_value(double c) { return bounded_to_value(c, kMinCorrespondenceCost, kMaxCorrespondenceCost); }
double value_to_cost(int v) { return value_to_bounded(v & (kValueCount - 1), kMaxCorrespondenceCost, kMinCorrespondenceCost, kMaxCorrespondenceCost); }

// computeLookupTableToApplyCorrespondenceCostOdds (every entry carries the update marker)
std::vector<uint16_t> odds_table(double o) {
    std::vector<uint16_t> t(kValueCount);
    t[0] = (uint16_t)(cost_to_value(1.0 - prob_from_odds(o)) + kUpdateMarker);
    for (int v = 1; v < kValueCount; ++v) t[v] = (uint16_t)(cost_to_value(1.0 - prob_from_odds(o * odds(1.0 - value_to_cost(v)))) + kUpdateMarker);
    return t;
}

struct Tables {
    std::vector<uint16_t> hit, miss, crop;
    std::vector<double> cost;                // Grid2D's value -> correspondence cost (getConversionTables(maxCC, minCC, maxCC))
    std::vector<float> cost_f;               // ... as getCorrespondenceCost returns it
    void build(double p_hit, double p_miss) {
        hit = odds_table(odds(p_hit)); miss = odds_table(odds(p_miss));
        cost.resize(kValueCount); cost_f.resize(kValueCount); crop.resize(kValueCount);
        for (int v = 0; v < kValueCount; ++v) { cost[v] = value_to_cost(v); cost_f[v] = (float)cost[v]; }
        // computeCroppedGrid: setProbability(getProbability(cell)) = correspondenceCostToValue(1 - (1 - valueToCorrespondenceCost(v)))
        crop[0] = 0;
        for (int v = 1; v < kValueCount; ++v) crop[v] = cost_to_value(1.0 - (1.0 - cost[v]));
    }
};

// ---------------------------------------------------------------- host restatement (sequential, as the reference runs it)
struct HostGrid {
    Limits L;
    std::vector<uint16_t> cells;
    Box known;
    std::vector<int64_t> upd;
    void init(const Limits& l) { L = l; cells.assign((size_t)L.nx * L.ny, 0); known = Box(); upd.clear(); }
    void grow_limits(double px, double py) {                                                   // Grid2D::growLimits
        int32_t xo, yo;
        Limits old = L;
        while (grow_step(L, px, py, xo, yo)) {
            std::vector<uint16_t> n((size_t)L.nx * L.ny, 0);
            for (int32_t i = 0; i < old.ny; ++i)
                for (int32_t j = 0; j < old.nx; ++j) n[(size_t)(xo + j) + (size_t)(i + yo) * L.nx] = cells[(size_t)j + (size_t)i * old.nx];
            cells.swap(n);
            if (!known.empty()) { known.min_x += xo; known.max_x += xo; known.min_y += yo; known.max_y += yo; }
            old = L;
        }
    }
    void apply(int32_t x, int32_t y, const std::vector<uint16_t>& table) {                     // ProbabilityGrid::applyLookUpTable
        if (!contains(L, x, y)) return;                                                        // (never taken: growth covers every cell)
        const int64_t i = (int64_t)L.nx * y + x;
        uint16_t& c = cells[(size_t)i];
        if (c >= kUpdateMarker) return;
        upd.push_back(i);
        c = table[c];
        known.extend(x, y);
    }
    void finish_update() { while (!upd.empty()) { cells[(size_t)upd.back()] -= kUpdateMarker; upd.pop_back(); } }
};

// ProbabilityGrid::computeCroppedGrid
void host_crop(const HostGrid& g, const std::vector<uint16_t>& crop, HostGrid& out, int32_t& offx, int32_t& offy) {
    int32_t cx = 1, cy = 1;
    offx = offy = 0;
    if (!g.known.empty()) { offx = g.known.min_x; offy = g.known.min_y; cx = g.known.max_x - g.known.min_x + 1; cy = g.known.max_y - g.known.min_y + 1; }
    Limits l;
    l.res = g.L.res;
    l.max_x = g.L.max_x - l.res * (double)offy;                                             // max - resolution * Vector2d(offset.y, offset.x)
    l.max_y = g.L.max_y - l.res * (double)offx;
    l.nx = cx; l.ny = cy;
    out.init(l);
    for (int32_t y = 0; y < cy; ++y)
        for (int32_t x = 0; x < cx; ++x) {
            const int32_t sx = x + offx, sy = y + offy;
            if (!contains(g.L, sx, sy)) continue;
            const uint16_t v = g.cells[(size_t)g.L.nx * sy + sx];
            if (v == 0) continue;                                                              // isKnown
            out.cells[(size_t)cx * y + x] = crop[v];                                           // setProbability(getProbability(...))
            out.known.extend(x, y);
        }
}

// the cells of one ray, in the reference's order, from the per-column work items
template <class F> void ray_cells(const Ray& r, F&& f, int S = kSubpixelScale) {
    const int32_t nc = ray_columns(r, S);
    for (int32_t j = 0; j < nc; ++j) {
        int32_t x, y0, y1, st;
        ray_column(r, j, x, y0, y1, st, S);
        for (int32_t y = y0;; y += st) { f(x, y); if (y == y1) break; }
    }
}

struct XY { double x, y; };
struct Transformed { XY origin; std::vector<XY> ret, miss; double bmin_x, bmin_y, bmax_x, bmax_y; };

// transformRangeData by the origin (Submap2D.cpp:45-48) and growAsNeeded's padded bounding box
void transform_rd(const double T[12], const visfs_range_data& rd, Transformed& t) {
    transform_xy(T, rd.origin, t.origin.x, t.origin.y);
    t.ret.resize(std::max(rd.n_returns, 0)); t.miss.resize(std::max(rd.n_misses, 0));
    double lo_x = t.origin.x, lo_y = t.origin.y, hi_x = t.origin.x, hi_y = t.origin.y;
    auto ext = [&](const XY& p) { lo_x = std::min(lo_x, p.x); lo_y = std::min(lo_y, p.y); hi_x = std::max(hi_x, p.x); hi_y = std::max(hi_y, p.y); };
    for (int i = 0; i < rd.n_returns; ++i) { transform_xy(T, rd.returns + 3 * i, t.ret[i].x, t.ret[i].y); ext(t.ret[i]); }
    for (int i = 0; i < rd.n_misses; ++i) { transform_xy(T, rd.misses + 3 * i, t.miss[i].x, t.miss[i].y); ext(t.miss[i]); }
    constexpr double kPadding = 1e-6;
    t.bmin_x = lo_x - kPadding; t.bmin_y = lo_y - kPadding; t.bmax_x = hi_x + kPadding; t.bmax_y = hi_y + kPadding;
}

Limits initial_limits(double res, const double T[12]) {                                       // ActiveSubmaps2D::createGrid
    Limits l;
    l.res = res;
    l.max_x = T[3] + 0.5 * kInitialSubmapSize * res;
    l.max_y = T[7] + 0.5 * kInitialSubmapSize * res;
    l.nx = l.ny = kInitialSubmapSize;
    return l;
}

constexpr int64_t kMaxCells = (int64_t)1 << 28;                                              // the BA's grid limit (ba_api.cpp)

// Growth that a range data asks of limits `L` (both padded corners), as the number of cells it would end with.
int64_t grown_cells(Limits L, const Transformed& t) {
    int32_t xo, yo;
    while (grow_step(L, t.bmin_x, t.bmin_y, xo, yo)) if ((int64_t)L.nx * L.ny > kMaxCells) return (int64_t)L.nx * L.ny;
    while (grow_step(L, t.bmax_x, t.bmax_y, xo, yo)) if ((int64_t)L.nx * L.ny > kMaxCells) return (int64_t)L.nx * L.ny;
    return (int64_t)L.nx * L.ny;
}

}  // namespace

// ---------------------------------------------------------------- kernels
namespace {

constexpr int SM_T = 256;

__global__ __launch_bounds__(SM_T) void k_submap_grow(const uint16_t* __restrict__ oc, const float* __restrict__ of, int32_t onx, int32_t ony,
                                                      int32_t xo, int32_t yo, uint16_t* __restrict__ nc, float* __restrict__ nf,
                                                      uint32_t* __restrict__ nh, uint32_t* __restrict__ nm, int32_t nx, int64_t n, float unknown) {
    const int64_t i = (int64_t)blockIdx.x * SM_T + threadIdx.x;
    if (i >= n) return;
    const int32_t y = (int32_t)(i / nx), x = (int32_t)(i - (int64_t)y * nx);
    const int32_t sx = x - xo, sy = y - yo;
    uint16_t v = 0;
    float f = unknown;
    if (oc != nullptr && sx >= 0 && sy >= 0 && sx < onx && sy < ony) { const int64_t o = (int64_t)sy * onx + sx; v = oc[o]; f = of[o]; }
    nc[i] = v; nf[i] = f; nh[i] = 0u; nm[i] = 0u;
}

struct MarkArgs {
    uint32_t* hit[2];
    uint32_t* miss[2];
    int32_t nx[2], ny[2];
};

__global__ __launch_bounds__(SM_T) void k_submap_mark(const MarkRec* __restrict__ recs, int32_t nrec, int32_t total, MarkArgs A) {
    const int32_t t = (int32_t)(blockIdx.x * SM_T + threadIdx.x);
    if (t >= total) return;
    int32_t lo = 0, hi = nrec - 1;                                  // the record whose items hold t
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (recs[mid].base <= t) lo = mid; else hi = mid - 1; }
    const MarkRec r = recs[lo];
    const int s = (r.flags >> 5) & 1;
    const uint32_t bit = 1u << (r.flags & 31u);
    const int32_t nx = A.nx[s], ny = A.ny[s];
    if (r.flags & 64u) {
        const int32_t x = r.ex / kSubpixelScale + r.ox, y = r.ey / kSubpixelScale + r.oy;
        if (x >= 0 && y >= 0 && x < nx && y < ny) atomicOr(A.hit[s] + (int64_t)y * nx + x, bit);
        return;
    }
    int32_t x, y0, st;
    const int32_t n = ray_item(Ray{ r.bx, r.by, r.ex, r.ey }, r.nchunk, t - r.base, x, y0, st);
    if (n == 0) return;
    x += r.ox;
    if (x < 0 || x >= nx) return;
    uint32_t* m = A.miss[s];
    for (int32_t k = 0; k < n; ++k) {
        const int32_t y = y0 + st * k + r.oy;
        if (y >= 0 && y < ny) atomicOr(m + (int64_t)y * nx + x, bit);
    }
}

struct ApplyArgs {
    uint16_t* cells[2];
    float* cost[2];
    uint32_t* hit[2];
    uint32_t* miss[2];
    int32_t nx[2];
    int32_t x0[2], y0[2], w[2], h[2];
};

// hit / miss: the tables without the update marker (finishUpdate right after each insertion)
__global__ __launch_bounds__(SM_T) void k_submap_apply(ApplyArgs A, const uint16_t* __restrict__ hitT, const uint16_t* __restrict__ missT,
                                                       const float* __restrict__ costT) {
    const int s = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * SM_T + threadIdx.x;
    if (i >= (int64_t)A.w[s] * A.h[s]) return;
    const int32_t yy = (int32_t)(i / A.w[s]), xx = (int32_t)(i - (int64_t)yy * A.w[s]);
    const int64_t c = (int64_t)(A.y0[s] + yy) * A.nx[s] + (A.x0[s] + xx);
    const uint32_t h = A.hit[s][c], m = A.miss[s][c];
    uint32_t any = h | m;
    if (any == 0u) return;
    uint16_t v = A.cells[s][c];
    while (any) {                                                   // the batch's insertions in order
        const int k = __builtin_ctz(any);
        any &= any - 1u;
        v = ((h >> k) & 1u) ? hitT[v] : missT[v];
    }
    A.cells[s][c] = v;
    A.cost[s][c] = costT[v];
    A.hit[s][c] = 0u;
    A.miss[s][c] = 0u;
}

__global__ __launch_bounds__(SM_T) void k_submap_crop(const uint16_t* __restrict__ oc, int32_t onx, int32_t offx, int32_t offy,
                                                      uint16_t* __restrict__ nc, float* __restrict__ nf, uint32_t* __restrict__ nh,
                                                      uint32_t* __restrict__ nm, int32_t nx, int64_t n,
                                                      const uint16_t* __restrict__ crop, const float* __restrict__ costT) {
    const int64_t i = (int64_t)blockIdx.x * SM_T + threadIdx.x;
    if (i >= n) return;
    const int32_t y = (int32_t)(i / nx), x = (int32_t)(i - (int64_t)y * nx);
    const uint16_t v = crop[oc[(int64_t)(y + offy) * onx + (x + offx)]];
    nc[i] = v; nf[i] = costT[v]; nh[i] = 0u; nm[i] = 0u;
}

}  // namespace

// ---------------------------------------------------------------- the sub-maps object
struct visfs_submaps {
    visfs_submap_params prm{};
    Tables tab;
    std::string err;
    bool device = false;

    // host restatement
    struct HSub { HostGrid g; int count = 0; bool finished = false; };
    std::deque<HSub> hsubs;

    // device
    visfs_ba_handle* h = nullptr;
    int dev = 0;
    hipStream_t stream = nullptr;
    DeviceBuf<char> d_tables;                 // one allocation, the four tables below
    uint16_t *d_hit = nullptr, *d_miss = nullptr, *d_crop = nullptr;
    float* d_cost = nullptr;
    struct DSub {
        Limits L;                 // current (host-simulated) limits
        Limits La;                // limits of the device allocation
        int32_t gx = 0, gy = 0;   // growth from La to L
        Box known;                // in L's coordinates
        int count = 0;
        bool finished = false;
        DeviceBuf<char> mem;      // one allocation, the four arrays below
        uint16_t* cells = nullptr; float* cost = nullptr; uint32_t* hit = nullptr; uint32_t* miss = nullptr;
    };
    std::deque<DSub> dsubs;
    // the batch being staged: records in the coordinates of the limits in force at their insertion (ox, oy = growth at that point)
    std::vector<MarkRec> recs;
    int batch_n = 0;
    PinnedBuf<MarkRec> h_recs;
    DeviceBuf<MarkRec> d_recs;
    bool recs_in_flight = false;

    // the scan matcher's state (ba_scan.hip), freed with the sub-maps
    void* scan_state = nullptr;
    void (*scan_destroy)(void*) = nullptr;
    void* refine_state = nullptr;
    void (*refine_destroy)(void*) = nullptr;

    ~visfs_submaps() {                        // before the members free what they own; the two states went in visfs_submaps_destroy
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {


// one allocation: cells, cost mirror, hit and miss marks
int dsub_alloc(visfs_submaps* s, const Limits& L, DeviceBuf<char>& mem, uint16_t** c, float** f, uint32_t** hm, uint32_t** mm) {
    const size_t n = (size_t)L.nx * L.ny;
    const size_t b2 = up256(n * 2), b4 = up256(n * 4);
    RC_TRY(mem.alloc(s, b2 + 3 * b4));
    *c = reinterpret_cast<uint16_t*>(mem.get());
    *f = reinterpret_cast<float*>(mem.get() + b2);
    *hm = reinterpret_cast<uint32_t*>(mem.get() + b2 + b4);
    *mm = reinterpret_cast<uint32_t*>(mem.get() + b2 + 2 * b4);
    return VISFS_BA_OK;
}

// the allocation follows the limits: a new (grown) allocation with the old cells moved by (gx, gy)
int dsub_realize(visfs_submaps* s, visfs_submaps::DSub& d) {
    if (d.mem && d.La.nx == d.L.nx && d.La.ny == d.L.ny) return VISFS_BA_OK;
    DeviceBuf<char> mem; uint16_t* c; float* f; uint32_t *hm, *mm;
    RC_TRY(dsub_alloc(s, d.L, mem, &c, &f, &hm, &mm));
    const int64_t n = (int64_t)d.L.nx * d.L.ny;
    hipLaunchKernelGGL(k_submap_grow, dim3(blocks_for(n, SM_T)), dim3(SM_T), 0, s->stream, d.cells, d.cost, d.La.nx, d.La.ny, d.gx, d.gy,
                       c, f, hm, mm, d.L.nx, n, s->tab.cost_f[0]);
    HIP_TRY(s, hipGetLastError());
    const int gone = d.mem.release(s);                                  // (waits for the copy above)
    d.mem = std::move(mem); d.cells = c; d.cost = f; d.hit = hm; d.miss = mm;       // whatever the free said: nothing points into the old block
    d.La = d.L; d.gx = d.gy = 0;
    return gone;
}

int flush_batch(visfs_submaps* s) {
    if (s->batch_n == 0) return VISFS_BA_OK;
    const int ns = (int)s->dsubs.size();
    // growth: final-grid offsets of every record, grown allocations
    Box box[2];
    for (MarkRec& r : s->recs) {
        const visfs_submaps::DSub& d = s->dsubs[(r.flags >> 5) & 1];
        r.ox = d.gx - r.ox; r.oy = d.gy - r.oy;
        const int S = kSubpixelScale;
        Box b;
        if (r.flags & 64u) b.extend(r.ex / S, r.ey / S);
        else { b.extend(r.bx / S, r.by / S); b.extend(r.ex / S, r.ey / S); }
        b.min_x += r.ox; b.max_x += r.ox; b.min_y += r.oy; b.max_y += r.oy;
        box[(r.flags >> 5) & 1].extend(b);
    }
    for (int k = 0; k < ns; ++k) {
        visfs_submaps::DSub& d = s->dsubs[k];
        const int32_t gx = d.gx, gy = d.gy;
        int rc = dsub_realize(s, d);
        if (rc != VISFS_BA_OK) return rc;
        (void)gx; (void)gy;
        d.known.extend(box[k]);                                        // (d.known was translated as the limits grew)
        // the box stays inside the grid (growth covers every endpoint); clip it all the same
        Box& b = box[k];
        if (!b.empty()) { b.min_x = std::max(b.min_x, 0); b.min_y = std::max(b.min_y, 0); b.max_x = std::min(b.max_x, d.L.nx - 1); b.max_y = std::min(b.max_y, d.L.ny - 1); }
    }
    // work items
    int64_t total = 0;
    for (MarkRec& r : s->recs) {
        r.base = (int32_t)total;
        if (r.flags & 64u) { r.nchunk = 1; total += 1; continue; }
        const Ray ray{ r.bx, r.by, r.ex, r.ey };
        r.nchunk = ray_nchunk(ray);
        total += (int64_t)ray_columns(ray) * r.nchunk;
    }
    if (total >= ((int64_t)1 << 31)) return fail(s, VISFS_BA_ERR_UNSUPPORTED, "a batch of more than 2^31 work items");
    const size_t nrec = s->recs.size();
    if (nrec > 0) {
        if (s->recs_in_flight) { HIP_TRY(s, hipStreamSynchronize(s->stream)); s->recs_in_flight = false; }
        RC_TRY(s->h_recs.grow(s, nrec, nrec / 2));
        RC_TRY(s->d_recs.grow(s, nrec, nrec / 2));
        std::memcpy(s->h_recs.get(), s->recs.data(), nrec * sizeof(MarkRec));
        HIP_TRY(s, hipMemcpyAsync(s->d_recs.get(), s->h_recs.get(), nrec * sizeof(MarkRec), hipMemcpyHostToDevice, s->stream));
        s->recs_in_flight = true;
        MarkArgs M{};
        for (int k = 0; k < ns; ++k) { M.hit[k] = s->dsubs[k].hit; M.miss[k] = s->dsubs[k].miss; M.nx[k] = s->dsubs[k].L.nx; M.ny[k] = s->dsubs[k].L.ny; }
        if (total > 0) {
            hipLaunchKernelGGL(k_submap_mark, dim3(blocks_for(total, SM_T)), dim3(SM_T), 0, s->stream, s->d_recs.get(), (int32_t)nrec, (int32_t)total, M);
            HIP_TRY(s, hipGetLastError());
        }
        ApplyArgs A{};
        int64_t most = 0;
        for (int k = 0; k < ns; ++k) {
            const visfs_submaps::DSub& d = s->dsubs[k];
            A.cells[k] = d.cells; A.cost[k] = d.cost; A.hit[k] = d.hit; A.miss[k] = d.miss; A.nx[k] = d.L.nx;
            if (box[k].empty()) { A.w[k] = A.h[k] = 0; continue; }
            A.x0[k] = box[k].min_x; A.y0[k] = box[k].min_y; A.w[k] = box[k].max_x - box[k].min_x + 1; A.h[k] = box[k].max_y - box[k].min_y + 1;
            most = std::max(most, (int64_t)A.w[k] * A.h[k]);
        }
        if (most > 0) {
            hipLaunchKernelGGL(k_submap_apply, dim3(blocks_for(most, SM_T), ns), dim3(SM_T), 0, s->stream, A, s->d_hit, s->d_miss, s->d_cost);
            HIP_TRY(s, hipGetLastError());
        }
    }
    s->recs.clear();
    s->batch_n = 0;
    return VISFS_BA_OK;
}

// Submap2D::finish on the device: the grid cropped to its known box through the value -> probability -> value round trip
int device_finish(visfs_submaps* s, visfs_submaps::DSub& d) {
    int32_t offx = 0, offy = 0, cx = 1, cy = 1;
    if (!d.known.empty()) { offx = d.known.min_x; offy = d.known.min_y; cx = d.known.max_x - d.known.min_x + 1; cy = d.known.max_y - d.known.min_y + 1; }
    Limits l;
    l.res = d.L.res;
    l.max_x = d.L.max_x - l.res * (double)offy;
    l.max_y = d.L.max_y - l.res * (double)offx;
    l.nx = cx; l.ny = cy;
    DeviceBuf<char> mem; uint16_t* c; float* f; uint32_t *hm, *mm;
    RC_TRY(dsub_alloc(s, l, mem, &c, &f, &hm, &mm));
    const int64_t n = (int64_t)cx * cy;
    hipLaunchKernelGGL(k_submap_crop, dim3(blocks_for(n, SM_T)), dim3(SM_T), 0, s->stream, d.cells, d.L.nx, offx, offy, c, f, hm, mm, cx, n, s->d_crop, s->d_cost);
    HIP_TRY(s, hipGetLastError());
    const int gone = d.mem.release(s);
    d.mem = std::move(mem); d.cells = c; d.cost = f; d.hit = hm; d.miss = mm;
    d.L = d.La = l; d.gx = d.gy = 0;
    Box b;
    if (!d.known.empty()) { b.extend(0, 0); b.extend(cx - 1, cy - 1); }              // every cell of the old known box's border rows is known
    d.known = b;
    d.finished = true;
    return gone;                                                        // a failed free is reported; the sub-map stands on its new block
}

// stage one range data into the batch: growth (host-simulated), the insertion's records with the limits in force at it
void stage(visfs_submaps* s, const Transformed& t) {
    const int bit = s->batch_n;
    for (size_t k = 0; k < s->dsubs.size(); ++k) {
        visfs_submaps::DSub& d = s->dsubs[k];
        int32_t xo, yo;
        const double px[2] = { t.bmin_x, t.bmax_x }, py[2] = { t.bmin_y, t.bmax_y };
        for (int c = 0; c < 2; ++c)
            while (grow_step(d.L, px[c], py[c], xo, yo)) {
                d.gx += xo; d.gy += yo;
                if (!d.known.empty()) { d.known.min_x += xo; d.known.max_x += xo; d.known.min_y += yo; d.known.max_y += yo; }
            }
        int32_t bx, by;
        superscaled_index(d.L, t.origin.x, t.origin.y, bx, by);
        const uint32_t fl = (uint32_t)bit | ((uint32_t)k << 5);
        for (const XY& p : t.ret) {
            int32_t ex, ey;
            superscaled_index(d.L, p.x, p.y, ex, ey);
            MarkRec hr{}; hr.ex = ex; hr.ey = ey; hr.ox = d.gx; hr.oy = d.gy; hr.flags = fl | 64u;
            s->recs.push_back(hr);
            const Ray r = ray_make(bx, by, ex, ey);
            MarkRec rr{}; rr.bx = r.bx; rr.by = r.by; rr.ex = r.ex; rr.ey = r.ey; rr.ox = d.gx; rr.oy = d.gy; rr.flags = fl;
            s->recs.push_back(rr);
        }
        for (const XY& p : t.miss) {
            int32_t ex, ey;
            superscaled_index(d.L, p.x, p.y, ex, ey);
            const Ray r = ray_make(bx, by, ex, ey);
            MarkRec rr{}; rr.bx = r.bx; rr.by = r.by; rr.ex = r.ex; rr.ey = r.ey; rr.ox = d.gx; rr.oy = d.gy; rr.flags = fl;
            s->recs.push_back(rr);
        }
        ++d.count;
    }
    ++s->batch_n;
}

int device_insert(visfs_submaps* s, const double T[12], const Transformed& t) {
    const int limit = s->prm.num_range_data_limit;
    int rc;
    if (s->dsubs.empty() || s->dsubs.back().count == limit) {                              // addSubmap (the front, finished, dropped)
        if ((rc = flush_batch(s)) != VISFS_BA_OK) return rc;
        if (s->dsubs.size() >= 2) { const int gone = s->dsubs.front().mem.release(s); s->dsubs.pop_front(); RC_TRY(gone); }
        visfs_submaps::DSub d;
        d.L = initial_limits(s->prm.map_resolution, T);
        s->dsubs.push_back(std::move(d));
        if ((rc = dsub_realize(s, s->dsubs.back())) != VISFS_BA_OK) return rc;
    }
    for (const visfs_submaps::DSub& d : s->dsubs)
        if (grown_cells(d.L, t) > kMaxCells) return fail(s, VISFS_BA_ERR_UNSUPPORTED, "a sub-map would grow beyond 2^28 cells");
    if (s->batch_n == kMaxBatch && (rc = flush_batch(s)) != VISFS_BA_OK) return rc;
    stage(s, t);
    if (s->dsubs.front().count == 2 * limit) {
        if ((rc = flush_batch(s)) != VISFS_BA_OK) return rc;
        if ((rc = device_finish(s, s->dsubs.front())) != VISFS_BA_OK) return rc;
    }
    return VISFS_BA_OK;
}

// ProbabilityGridRangeDataInserter2D::insert (castRays with insertFreeSpace = true) + finishUpdate
void host_cast(visfs_submaps* s, HostGrid& g, const Transformed& t) {
    g.grow_limits(t.bmin_x, t.bmin_y);
    g.grow_limits(t.bmax_x, t.bmax_y);
    const int S = kSubpixelScale;
    int32_t bx, by;
    superscaled_index(g.L, t.origin.x, t.origin.y, bx, by);
    std::vector<int32_t> ends(2 * t.ret.size());
    for (size_t i = 0; i < t.ret.size(); ++i) {
        superscaled_index(g.L, t.ret[i].x, t.ret[i].y, ends[2 * i], ends[2 * i + 1]);
        g.apply(ends[2 * i] / S, ends[2 * i + 1] / S, s->tab.hit);
    }
    auto miss = [&](int32_t x, int32_t y) { g.apply(x, y, s->tab.miss); };
    for (size_t i = 0; i < t.ret.size(); ++i) ray_cells(ray_make(bx, by, ends[2 * i], ends[2 * i + 1]), miss);
    for (const XY& p : t.miss) {
        int32_t ex, ey;
        superscaled_index(g.L, p.x, p.y, ex, ey);
        ray_cells(ray_make(bx, by, ex, ey), miss);
    }
    g.finish_update();
}

int host_insert(visfs_submaps* s, const double T[12], const Transformed& t) {                 // ActiveSubmaps2D::insertRangeData
    const int limit = s->prm.num_range_data_limit;
    if (s->hsubs.empty() || s->hsubs.back().count == limit) {
        if (s->hsubs.size() >= 2) s->hsubs.pop_front();
        s->hsubs.emplace_back();
        s->hsubs.back().g.init(initial_limits(s->prm.map_resolution, T));
    }
    for (const visfs_submaps::HSub& d : s->hsubs)
        if (grown_cells(d.g.L, t) > kMaxCells) return fail(s, VISFS_BA_ERR_UNSUPPORTED, "a sub-map would grow beyond 2^28 cells");
    for (visfs_submaps::HSub& d : s->hsubs) { host_cast(s, d.g, t); ++d.count; }
    if (s->hsubs.front().count == 2 * limit) {
        HostGrid c;
        int32_t ox, oy;
        host_crop(s->hsubs.front().g, s->tab.crop, c, ox, oy);
        s->hsubs.front().g = std::move(c);
        s->hsubs.front().finished = true;
    }
    return VISFS_BA_OK;
}

int check_params(const visfs_submap_params* p, std::string& why) {
    if (p->grid_map_type == 1) { why = "LocalMap/GridMapType 1 (TSDF) is not supported (the reference stops on it as well)"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (p->grid_map_type != 0) { why = "unknown LocalMap/GridMapType"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (p->num_range_data_limit < 1) { why = "LocalMap/NumRangeDataLimit must be positive"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (!(p->map_resolution > 0.0) || !std::isfinite(p->map_resolution)) { why = "LocalMap/MapResolution must be positive"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (!(p->hit_probability > 0.0 && p->hit_probability < 1.0) || !(p->miss_probability > 0.0 && p->miss_probability < 1.0)) {
        why = "hit and miss probabilities must lie in (0, 1)"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    return VISFS_BA_OK;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_submap_abi_version(void) { return VISFS_SUBMAP_ABI_VERSION; }

void visfs_submap_default_params(visfs_submap_params* p) {
    if (!p) return;
    p->num_range_data_limit = 50; p->grid_map_type = 0; p->map_resolution = 0.05; p->insert_free_space = 1;
    p->hit_probability = 0.55; p->miss_probability = 0.49;
}

int visfs_submaps_create_host(const visfs_submap_params* p, visfs_submaps** out) {
    if (!p || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        std::string why;
        const int rc = check_params(p, why);
        if (rc != VISFS_BA_OK) return rc;
        visfs_submaps* s = new visfs_submaps();
        s->prm = *p;
        s->tab.build(p->hit_probability, p->miss_probability);
        *out = s;
        return (int)VISFS_BA_OK;
    });
}

int visfs_submaps_create(visfs_ba_handle* h, const visfs_submap_params* p, visfs_submaps** out) {
    if (!h || !p || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        std::string why;
        int rc = check_params(p, why);
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, why.c_str()); return rc; }
        visfs_submaps* s = new visfs_submaps();
        s->prm = *p;
        s->tab.build(p->hit_probability, p->miss_probability);
        s->device = true; s->h = h; s->dev = visfs_internal_device(h); s->stream = visfs_internal_stream(h);
        auto init = [&]() -> int {
            HIP_TRY(s, hipSetDevice(s->dev));
            // the tables, one allocation: hit, miss (without the update marker), crop round trip (uint16), cost (float)
            const size_t b2 = up256((size_t)kValueCount * 2), b4 = up256((size_t)kValueCount * 4);
            RC_TRY(s->d_tables.alloc(s, 3 * b2 + b4));
            char* const mem = s->d_tables.get();
            s->d_hit = reinterpret_cast<uint16_t*>(mem); s->d_miss = reinterpret_cast<uint16_t*>(mem + b2);
            s->d_crop = reinterpret_cast<uint16_t*>(mem + 2 * b2); s->d_cost = reinterpret_cast<float*>(mem + 3 * b2);
            std::vector<uint16_t> hit(kValueCount), miss(kValueCount);
            for (int v = 0; v < kValueCount; ++v) { hit[v] = (uint16_t)(s->tab.hit[v] - kUpdateMarker); miss[v] = (uint16_t)(s->tab.miss[v] - kUpdateMarker); }
            HIP_TRY(s, hipMemcpy(s->d_hit, hit.data(), kValueCount * 2, hipMemcpyHostToDevice));
            HIP_TRY(s, hipMemcpy(s->d_miss, miss.data(), kValueCount * 2, hipMemcpyHostToDevice));
            HIP_TRY(s, hipMemcpy(s->d_crop, s->tab.crop.data(), kValueCount * 2, hipMemcpyHostToDevice));
            HIP_TRY(s, hipMemcpy(s->d_cost, s->tab.cost_f.data(), kValueCount * 4, hipMemcpyHostToDevice));
            return VISFS_BA_OK;
        };
        rc = init();
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, s->err.c_str()); delete s; return rc; }
        *out = s;
        return (int)VISFS_BA_OK;
    });
}

void visfs_submaps_destroy(visfs_submaps* s) {
    if (!s) return;
    if (s->scan_state && s->scan_destroy) {
        if (s->device) { (void)hipSetDevice(s->dev); if (s->stream) (void)hipStreamSynchronize(s->stream); }
        s->scan_destroy(s->scan_state);
        s->scan_state = nullptr;
    }
    if (s->refine_state && s->refine_destroy) {
        if (s->device) { (void)hipSetDevice(s->dev); if (s->stream) (void)hipStreamSynchronize(s->stream); }
        s->refine_destroy(s->refine_state);
        s->refine_state = nullptr;
    }
    delete s;
}

const char* visfs_submaps_last_error(const visfs_submaps* s) { return s ? s->err.c_str() : "null sub-maps"; }

int visfs_submaps_insert(visfs_submaps* s, const double Twr[12], int32_t n, const visfs_range_data* rd) {
    if (!s || !Twr || n < 0 || (n > 0 && !rd)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        for (int i = 0; i < 12; ++i) if (!std::isfinite(Twr[i])) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "Twr is not finite");
        for (int k = 0; k < n; ++k) {
            const visfs_range_data& r = rd[k];
            if (r.n_returns < 0 || r.n_misses < 0 || (r.n_returns > 0 && !r.returns) || (r.n_misses > 0 && !r.misses))
                return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "range data with negative sizes or without coordinates");
            for (int i = 0; i < 3; ++i) if (!std::isfinite(r.origin[i])) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "range data origin is not finite");
            for (int64_t i = 0; i < 3 * (int64_t)r.n_returns; ++i) if (!std::isfinite(r.returns[i])) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "a return is not finite");
            for (int64_t i = 0; i < 3 * (int64_t)r.n_misses; ++i) if (!std::isfinite(r.misses[i])) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "a miss is not finite");
        }
        if (s->device) HIP_TRY(s, hipSetDevice(s->dev));
        Transformed t;
        for (int k = 0; k < n; ++k) {                                  // each range data its own insertion, in order
            transform_rd(Twr, rd[k], t);
            const int rc = s->device ? device_insert(s, Twr, t) : host_insert(s, Twr, t);
            if (rc != VISFS_BA_OK) { if (s->device) (void)flush_batch(s); return rc; }
        }
        return s->device ? flush_batch(s) : (int)VISFS_BA_OK;
    });
}

int visfs_submaps_describe(const visfs_submaps* s, int32_t* n, visfs_submap_info* info) {
    if (!s || !n) return VISFS_BA_ERR_BAD_ARGUMENT;
    auto put = [&](int k, const Limits& L, const Box& b, int count, bool fin) {
        if (!info) return;
        visfs_submap_info& o = info[k];
        o.num_range_data = count; o.finished = fin ? 1 : 0;
        o.resolution = L.res; o.max_x = L.max_x; o.max_y = L.max_y; o.num_x_cells = L.nx; o.num_y_cells = L.ny;
        o.known_min_x = b.min_x; o.known_min_y = b.min_y; o.known_max_x = b.max_x; o.known_max_y = b.max_y;
    };
    if (s->device) { *n = (int32_t)s->dsubs.size(); for (int k = 0; k < *n; ++k) put(k, s->dsubs[k].L, s->dsubs[k].known, s->dsubs[k].count, s->dsubs[k].finished); }
    else { *n = (int32_t)s->hsubs.size(); for (int k = 0; k < *n; ++k) put(k, s->hsubs[k].g.L, s->hsubs[k].g.known, s->hsubs[k].count, s->hsubs[k].finished); }
    return VISFS_BA_OK;
}

int visfs_submaps_download(const visfs_submaps* cs, int32_t index, uint16_t* cells, float* cost) {
    visfs_submaps* s = const_cast<visfs_submaps*>(cs);
    if (!s) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        const int ns = s->device ? (int)s->dsubs.size() : (int)s->hsubs.size();
        if (index < 0 || index >= ns) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        if (!s->device) {
            const HostGrid& g = s->hsubs[index].g;
            if (cells) std::memcpy(cells, g.cells.data(), g.cells.size() * 2);
            if (cost) for (size_t i = 0; i < g.cells.size(); ++i) cost[i] = s->tab.cost_f[g.cells[i]];
            return (int)VISFS_BA_OK;
        }
        const visfs_submaps::DSub& d = s->dsubs[index];
        const size_t n = (size_t)d.L.nx * d.L.ny;
        HIP_TRY(s, hipSetDevice(s->dev));
        if (cells) HIP_TRY(s, hipMemcpyAsync(cells, d.cells, n * 2, hipMemcpyDeviceToHost, s->stream));
        if (cost) HIP_TRY(s, hipMemcpyAsync(cost, d.cost, n * 4, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        s->recs_in_flight = false;
        return (int)VISFS_BA_OK;
    });
}

int visfs_submaps_solve_window(visfs_ba_handle* h, const visfs_submaps* cs, const visfs_ba_window* w, visfs_ba_result* r) {
    visfs_submaps* s = const_cast<visfs_submaps*>(cs);
    if (!h || !s || !w || !r) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!s->device) { visfs_internal_set_error(h, "host sub-maps have no device grid"); return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (s->dev != visfs_internal_device(h)) { visfs_internal_set_error(h, "the sub-maps live on another device"); return VISFS_BA_ERR_BAD_ARGUMENT; }
    visfs_ba_window wl = *w;
    if (s->dsubs.empty()) {                                            // hasMatchingSubmap2D() false: no laser edges
        wl.grid = nullptr;
        return visfs_ba_solve_window(h, &wl, r);
    }
    const visfs_submaps::DSub& d = s->dsubs.front();                  // getMatchingSubmap2D(): front()
    if (s->stream != visfs_internal_stream(h)) {                       // sub-maps of another handle's stream: their insertions first
        if (hipSetDevice(s->dev) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) { visfs_internal_set_error(h, "hipStreamSynchronize failed"); return VISFS_BA_ERR_DEVICE; }
    }
    visfs_ba_grid G;
    G.resolution = d.L.res; G.max_x = d.L.max_x; G.max_y = d.L.max_y; G.num_x_cells = d.L.nx; G.num_y_cells = d.L.ny;
    G.correspondence_cost = d.cost;                                    // (device memory: read by the device-to-device copy only)
    wl.grid = &G;
    return visfs_internal_solve_window(h, &wl, r, d.cost);
}

// ---- host-only hooks
int visfs_submap_hook_ray(const int32_t begin[2], const int32_t end[2], int32_t scale, int32_t cap, int32_t* cells_xy) {
    if (!begin || !end || cap < 0 || (cap > 0 && !cells_xy)) return -VISFS_BA_ERR_BAD_ARGUMENT;
    if (scale < 1 || scale > (1 << 20)) return -VISFS_BA_ERR_BAD_ARGUMENT;
    int32_t n = 0;
    auto put = [&](int32_t x, int32_t y) { if (n < cap) { cells_xy[2 * n] = x; cells_xy[2 * n + 1] = y; } ++n; };
    ray_cells(ray_make(begin[0], begin[1], end[0], end[1]), put, scale);
    return n;
}

int visfs_submap_hook_mark_items(const int32_t begin[2], const int32_t end[2], int32_t scale, int32_t cap, int32_t* cells_xy, int64_t* n_items) {
    if (!begin || !end || !n_items || cap < 0 || (cap > 0 && !cells_xy)) return -VISFS_BA_ERR_BAD_ARGUMENT;
    if (scale < 1 || scale > (1 << 20)) return -VISFS_BA_ERR_BAD_ARGUMENT;
    const Ray r = ray_make(begin[0], begin[1], end[0], end[1]);
    const int32_t nchunk = ray_nchunk(r, scale);                     // as flush_batch sizes the ray's record
    const int64_t total = (int64_t)ray_columns(r, scale) * nchunk;
    *n_items = total;
    if (total >= ((int64_t)1 << 31)) return -VISFS_BA_ERR_UNSUPPORTED;
    int32_t n = 0;
    for (int32_t local = 0; local < (int32_t)total; ++local) {       // k_submap_mark's items of the record, in index order
        int32_t x, y, st;
        const int32_t cnt = ray_item(r, nchunk, local, x, y, st, scale);
        for (int32_t k = 0; k < cnt; ++k) {
            if (n < cap) { cells_xy[2 * n] = x; cells_xy[2 * n + 1] = y + st * k; }
            ++n;
        }
    }
    return n;
}

int visfs_submap_hook_odds_table(double o, uint16_t* table) {
    if (!table || !(o > 0.0)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int { const std::vector<uint16_t> t = odds_table(o); std::memcpy(table, t.data(), kValueCount * 2); return (int)VISFS_BA_OK; });
}

int visfs_submap_hook_value_tables(double* cost, uint16_t* crop) {
    return guarded(nullptr, [&]() -> int {
        Tables t;
        t.build(0.55, 0.49);
        if (cost) std::memcpy(cost, t.cost.data(), kValueCount * 8);
        if (crop) std::memcpy(crop, t.crop.data(), kValueCount * 2);
        return (int)VISFS_BA_OK;
    });
}

int visfs_submap_hook_crop(int32_t nx, int32_t ny, const uint16_t* cells, const int32_t box[4], int64_t cap, int32_t out_dims[4],
                           uint16_t* out_cells, int32_t out_box[4]) {
    if (nx <= 0 || ny <= 0 || !cells || !box || !out_dims || !out_box || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int {
        Tables t;
        t.build(0.55, 0.49);
        HostGrid g;
        Limits L; L.res = 1.0; L.nx = nx; L.ny = ny;
        g.L = L;
        g.cells.assign(cells, cells + (size_t)nx * ny);
        g.known.min_x = box[0]; g.known.min_y = box[1]; g.known.max_x = box[2]; g.known.max_y = box[3];
        HostGrid c;
        int32_t ox, oy;
        host_crop(g, t.crop, c, ox, oy);
        out_dims[0] = ox; out_dims[1] = oy; out_dims[2] = c.L.nx; out_dims[3] = c.L.ny;
        if ((int64_t)c.cells.size() > cap) return (int)VISFS_BA_ERR_BAD_ARGUMENT;
        if (out_cells) std::memcpy(out_cells, c.cells.data(), c.cells.size() * 2);
        out_box[0] = c.known.min_x; out_box[1] = c.known.min_y; out_box[2] = c.known.max_x; out_box[3] = c.known.max_y;
        return (int)VISFS_BA_OK;
    });
}

}  // extern "C"

// ====================================================================== what the scan matcher (ba_scan.hip) reads
int visfs_internal_scan_access(visfs_submaps* s, int32_t index, submap::ScanAccess* a) {
    *a = submap::ScanAccess();
    a->device = s->device; a->dev = s->dev; a->stream = s->stream;
    if (s->device) {
        HIP_TRY(s, hipSetDevice(s->dev));
        const int rc = flush_batch(s);
        if (rc != VISFS_BA_OK) return rc;
        a->count = (int32_t)s->dsubs.size();
        if (index < 0 || index >= a->count) return VISFS_BA_OK;
        const visfs_submaps::DSub& d = s->dsubs[index];
        a->L = d.L;
        a->grid.cells = d.cells; a->grid.nx = d.La.nx; a->grid.ny = d.La.ny; a->grid.ox = d.gx; a->grid.oy = d.gy;
        return VISFS_BA_OK;
    }
    a->count = (int32_t)s->hsubs.size();
    if (index < 0 || index >= a->count) return VISFS_BA_OK;
    const HostGrid& g = s->hsubs[index].g;
    a->L = g.L;
    a->grid.cells = g.cells.data(); a->grid.nx = g.L.nx; a->grid.ny = g.L.ny;
    return VISFS_BA_OK;
}

int visfs_internal_scan_fail(visfs_submaps* s, int rc, const char* why) { return fail(s, rc, why); }

void** visfs_internal_scan_slot(visfs_submaps* s, void (*destroy)(void*)) {
    s->scan_destroy = destroy;
    return &s->scan_state;
}

void** visfs_internal_refine_slot(visfs_submaps* s, void (*destroy)(void*)) {
    s->refine_destroy = destroy;
    return &s->refine_state;
}
