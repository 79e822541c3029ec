// A global occupancy map composed on the GPU from frozen sub-maps (include/visfs_map.h).
//
//   k_map_tile     the device-to-device freeze of visfs_map_add_submap: one work item per tile cell reads the sub-map's allocation
//                  through its GridView (growth offset) and writes the dense [ny][nx] tile with the update marker stripped;
//   k_map_compose  one work item per output cell, a workgroup of 256 laid out 64 along ix by 4 along iy: a wavefront stores 128
//                  contiguous bytes of a row, and its reads of a tile run along one line of it.  A workgroup skips every tile whose
//                  box misses its block (scalars only).  No atomics, no LDS, no workgroup waits for another.
// A compose is one upload (the tile table), one launch and one wait; the grid and the count plane stay on the device until
// visfs_map_download or visfs_scan_stack_create_from_map asks for them.  The one-core twin calls the same compose_cell of ba_map.hpp.
#include "ba_map.hpp"
#include "ba_scan_stack_access.hpp"
#include "ba_map_access.hpp"
#include "ba_host.hpp"

#include <cstring>
#include <new>
#include <string>
#include <vector>

#pragma clang fp contract(off)

using namespace gmap;
using namespace host;
using submap::GridView;
using submap::Limits;

namespace gmap {

__global__ __launch_bounds__(kThreads) void k_map_tile(GridView g, int32_t nx, int64_t total, uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t y = (int32_t)(i / nx), x = (int32_t)(i - (int64_t)y * nx);
    out[i] = frozen_cell(g, x, y);
}

// blocks_x: workgroups along ix; the grid is one-dimensional (a tall grid of one column has more rows of blocks than a grid's y
// dimension may have).
__global__ __launch_bounds__(kThreads) void k_map_compose(const TileRec* __restrict__ tiles, int32_t nt, const int32_t* __restrict__ L, int32_t combine,
                                                          double max_x, double max_y, double res, int32_t nx, int32_t ny, int32_t blocks_x,
                                                          uint16_t* __restrict__ cells, uint8_t* __restrict__ count) {
    const int32_t b = (int32_t)blockIdx.x;
    const int32_t by = (b / blocks_x) * kBlockY, bx = (b - (b / blocks_x) * blocks_x) * kBlockX;
    const int32_t ix = bx + (int32_t)(threadIdx.x & (kBlockX - 1)), iy = by + (int32_t)(threadIdx.x / kBlockX);
    if (ix >= nx || iy >= ny) return;
    uint16_t v;
    uint8_t c;
    compose_cell(tiles, nt, L, combine, max_x, max_y, res, bx, by, ix, iy, v, c);
    const int64_t o = (int64_t)iy * nx + ix;
    cells[o] = v;
    count[o] = c;
}

}  // namespace gmap

struct visfs_map {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    std::string err;
    struct Tile {
        PlanTile p;
        std::vector<uint16_t> h;              // twin
        DeviceBuf<uint16_t> d;                // device
    };
    std::vector<Tile> tiles;
    int64_t tile_bytes = 0;
    std::vector<int32_t> L;                   // the log-odds table
    DeviceBuf<int32_t> d_L;
    // the last composed grid
    bool have = false;
    Limits G;
    std::vector<uint16_t> h_cells;
    std::vector<uint8_t> h_count;
    DeviceBuf<uint16_t> d_cells;
    DeviceBuf<uint8_t> d_count;               // made behind d_cells: its capacity (cells) stands for both
    Staged<TileRec> tab;
    host::Counts counts;

    ~visfs_map() {                            // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

std::vector<int32_t> odds_table() {
    std::vector<double> cost(kValues);
    std::vector<int32_t> L(kValues, 0);
    if (visfs_submap_hook_value_tables(cost.data(), nullptr) != VISFS_BA_OK) throw std::bad_alloc();
    for (int v = 1; v < kValues; ++v) L[v] = (int32_t)std::llround(std::log((1.0 - cost[v]) / cost[v]) * 1048576.0);
    return L;
}

void free_tiles(visfs_map* m) {
    m->tiles.clear();
    m->tile_bytes = 0;
}

bool pose_ok(const double p[3]) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// The checks every new tile passes before anything is allocated or pushed.
int check_tile(visfs_map* m, const Limits& L, const double pose[3]) {
    if (!pose_ok(pose)) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "the pose is not finite");
    if (!limits_ok(L.res, L.max_x, L.max_y, L.nx, L.ny))
        return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "the limits need a positive resolution, a finite corner and at least one cell per axis");
    if (m->tiles.size() >= (size_t)VISFS_MAP_MAX_TILES) return fail(m, VISFS_BA_ERR_UNSUPPORTED, "more than 256 tiles");
    const int64_t bytes = (int64_t)L.nx * L.ny * 2;
    if (bytes > (int64_t)VISFS_MAP_MAX_TILE_BYTES || m->tile_bytes + bytes > (int64_t)VISFS_MAP_MAX_TILE_BYTES)
        return fail(m, VISFS_BA_ERR_UNSUPPORTED, "the tiles together exceed 1 GiB");
    return VISFS_BA_OK;
}

// The new tile's cells from `g` (memory of the map's flavour; `staged`: host cells for a device map).
int push_tile(visfs_map* m, const Limits& L, const double pose[3], const GridView& g, bool staged, int32_t* tile) {
    visfs_map::Tile t;
    t.p.L = L;
    for (int i = 0; i < 3; ++i) t.p.pose[i] = pose[i];
    const int64_t n = (int64_t)L.nx * L.ny;
    if (!m->device) {
        t.h.resize((size_t)n);
        for (int32_t y = 0; y < L.ny; ++y)
            for (int32_t x = 0; x < L.nx; ++x) t.h[(size_t)y * L.nx + x] = frozen_cell(g, x, y);
    } else {
        HIP_TRY(m, hipSetDevice(m->dev));
        RC_TRY(t.d.alloc(m, (size_t)n));
        if (staged) {
            std::vector<uint16_t> tmp((size_t)n);
            for (int32_t y = 0; y < L.ny; ++y)
                for (int32_t x = 0; x < L.nx; ++x) tmp[(size_t)y * L.nx + x] = frozen_cell(g, x, y);
            HIP_TRY(m, hipMemcpyAsync(t.d.get(), tmp.data(), (size_t)n * 2, hipMemcpyHostToDevice, m->stream));
            HIP_TRY(m, hipStreamSynchronize(m->stream));
        } else {
            hipLaunchKernelGGL(k_map_tile, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, m->stream, g, L.nx, n, t.d.get());
            HIP_TRY(m, hipGetLastError());
            HIP_TRY(m, hipStreamSynchronize(m->stream));                     // the sub-map may change or go from here on
        }
    }
    m->tile_bytes += n * 2;
    m->tiles.push_back(std::move(t));
    if (tile) *tile = (int32_t)m->tiles.size() - 1;
    return VISFS_BA_OK;
}

int device_compose(visfs_map* m, const visfs_map_params& p, Plan& P) {
    const Limits& G = P.G;
    const size_t cells = (size_t)G.nx * G.ny, nt = P.recs.size(), recs = nt ? nt : 1;
    HIP_TRY(m, hipSetDevice(m->dev));
    if (m->d_count.cap() < cells) {
        m->have = false;                                                   // the old grid goes with its buffers
        RC_TRY(m->d_cells.release(m));
        RC_TRY(m->d_count.release(m));
        RC_TRY(m->d_cells.alloc(m, cells));
        RC_TRY(m->d_count.alloc(m, cells));
    }
    RC_TRY(m->tab.reserve(m, recs, recs < 16 ? 16 : recs));
    std::memset(m->tab.h.get(), 0, recs * sizeof(TileRec));
    for (size_t k = 0; k < nt; ++k) { m->tab.h[k] = P.recs[k]; m->tab.h[k].cells = m->tiles[k].d.get(); }
    m->have = false;                                                       // the grid is being overwritten from here on
    HIP_TRY(m, hipMemcpyAsync(m->tab.d.get(), m->tab.h.get(), recs * sizeof(TileRec), hipMemcpyHostToDevice, m->stream));
    const int32_t blocks_x = (G.nx + kBlockX - 1) / kBlockX, blocks_y = (G.ny + kBlockY - 1) / kBlockY;
    hipLaunchKernelGGL(k_map_compose, dim3((unsigned)((int64_t)blocks_x * blocks_y)), dim3(kThreads), 0, m->stream, m->tab.d.get(), (int32_t)nt, m->d_L.get(),
                       p.combine, G.max_x, G.max_y, G.res, G.nx, G.ny, blocks_x, m->d_cells.get(), m->d_count.get());
    HIP_TRY(m, hipGetLastError());
    HIP_TRY(m, hipStreamSynchronize(m->stream));
    m->counts = { 1, 1, 1 };
    return VISFS_BA_OK;
}

void host_compose(visfs_map* m, const visfs_map_params& p, Plan& P) {
    const Limits& G = P.G;
    for (size_t k = 0; k < P.recs.size(); ++k) P.recs[k].cells = m->tiles[k].h.data();
    m->h_cells.assign((size_t)G.nx * G.ny, 0);
    m->h_count.assign((size_t)G.nx * G.ny, 0);
    for (int32_t iy = 0; iy < G.ny; ++iy)
        for (int32_t ix = 0; ix < G.nx; ++ix) {
            const size_t o = (size_t)iy * G.nx + ix;
            compose_cell(P.recs.data(), (int32_t)P.recs.size(), m->L.data(), p.combine, G.max_x, G.max_y, G.res, (ix / kBlockX) * kBlockX,
                         (iy / kBlockY) * kBlockY, ix, iy, m->h_cells[o], m->h_count[o]);
        }
    m->counts = {};
}

}  // namespace

int visfs_internal_map_access(visfs_map* m, gmap::MapAccess* a) {
    if (!m || !a) return VISFS_BA_ERR_BAD_ARGUMENT;
    a->device = m->device; a->dev = m->dev; a->stream = m->stream; a->have = m->have; a->L = m->G;
    a->cells = m->device ? m->d_cells.get() : m->h_cells.data();
    return VISFS_BA_OK;
}

// ====================================================================== exported C ABI
extern "C" {

int visfs_map_abi_version(void) { return VISFS_MAP_ABI_VERSION; }

void visfs_map_default_params(visfs_map_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->combine = VISFS_MAP_ODDS;
    p->resolution = 0.05;
    p->explicit_limits = 0;
}

int visfs_map_create(visfs_ba_handle* h, visfs_map** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        visfs_map* m = new visfs_map();
        m->L = odds_table();
        if (h) {
            m->device = true; m->dev = visfs_internal_device(h); m->stream = visfs_internal_stream(h);
            auto run = [&]() -> int {
                HIP_TRY(m, hipSetDevice(m->dev));
                RC_TRY(m->d_L.alloc(m, kValues));
                HIP_TRY(m, hipMemcpyAsync(m->d_L.get(), m->L.data(), kValues * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
                HIP_TRY(m, hipStreamSynchronize(m->stream));
                return VISFS_BA_OK;
            };
            const int rc = run();
            if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, m->err.c_str()); delete m; return rc; }
        }
        *out = m;
        return (int)VISFS_BA_OK;
    });
}

void visfs_map_destroy(visfs_map* m) { delete m; }

const char* visfs_map_last_error(const visfs_map* m) { return m ? m->err.c_str() : "null map"; }

int visfs_map_add_submap(visfs_map* m, visfs_submaps* s, int32_t index, const double pose[3], int32_t* tile) {
    if (!m || !s || !pose) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(m, [&]() -> int {
        submap::ScanAccess acc;
        int rc = visfs_internal_scan_access(s, index, &acc);               // flushes a staged batch
        if (rc != VISFS_BA_OK) return fail(m, rc, std::string("the sub-maps: ") + visfs_submaps_last_error(s));
        if (acc.device != m->device || (m->device && (acc.dev != m->dev || acc.stream != m->stream)))
            return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "the sub-maps are not of the map's flavour, device and stream");
        if (index < 0 || index >= acc.count) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        if ((rc = check_tile(m, acc.L, pose)) != VISFS_BA_OK) return rc;
        return push_tile(m, acc.L, pose, acc.grid, false, tile);
    });
}

int visfs_map_add_grid(visfs_map* m, const visfs_submap_info* lim, const uint16_t* cells, const double pose[3], int32_t* tile) {
    if (!m || !lim || !cells || !pose) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(m, [&]() -> int {
        const Limits L = submap::limits_of(*lim);
        const int rc = check_tile(m, L, pose);
        if (rc != VISFS_BA_OK) return rc;
        GridView g;
        g.cells = cells; g.nx = L.nx; g.ny = L.ny;
        return push_tile(m, L, pose, g, true, tile);
    });
}

int visfs_map_set_poses(visfs_map* m, int32_t first, int32_t count, const double* poses) {
    if (!m || (count > 0 && !poses)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(m, [&]() -> int {
        if (first < 0 || count < 0 || (int64_t)first + count > (int64_t)m->tiles.size()) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "tile index out of range");
        for (int32_t i = 0; i < count; ++i) if (!pose_ok(poses + 3 * (size_t)i)) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "a pose is not finite");
        for (int32_t i = 0; i < count; ++i)
            for (int k = 0; k < 3; ++k) m->tiles[(size_t)first + i].p.pose[k] = poses[3 * (size_t)i + k];
        return (int)VISFS_BA_OK;
    });
}

int visfs_map_clear(visfs_map* m) {
    if (!m) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(m, [&]() -> int {
        if (m->device) { HIP_TRY(m, hipSetDevice(m->dev)); HIP_TRY(m, hipStreamSynchronize(m->stream)); }
        free_tiles(m);
        return (int)VISFS_BA_OK;
    });
}

int visfs_map_describe_tile(const visfs_map* m, int32_t tile, visfs_submap_info* limits, double pose[3]) {
    if (!m) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (tile < 0 || (size_t)tile >= m->tiles.size()) return VISFS_BA_ERR_BAD_ARGUMENT;
    const PlanTile& t = m->tiles[(size_t)tile].p;
    if (limits) {
        std::memset(limits, 0, sizeof *limits);
        limits->resolution = t.L.res; limits->max_x = t.L.max_x; limits->max_y = t.L.max_y; limits->num_x_cells = t.L.nx; limits->num_y_cells = t.L.ny;
        limits->known_min_x = limits->known_min_y = 1;                     // not tracked: empty
    }
    if (pose) for (int k = 0; k < 3; ++k) pose[k] = t.pose[k];
    return VISFS_BA_OK;
}

int visfs_map_compose(visfs_map* m, const visfs_map_params* p, visfs_map_info* info) {
    if (!m || !p) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(m, [&]() -> int {
        std::vector<PlanTile> tiles;
        for (const visfs_map::Tile& t : m->tiles) tiles.push_back(t.p);
        Plan P;
        const char* why = "";
        int rc = make_plan(*p, tiles, P, &why);
        if (rc != VISFS_BA_OK) return fail(m, rc, why);
        if (m->device) { if ((rc = device_compose(m, *p, P)) != VISFS_BA_OK) return rc; }
        else host_compose(m, *p, P);
        m->G = P.G; m->have = true;
        if (info) {
            fill_info(P, info->limits);
            info->tiles = (int32_t)tiles.size(); info->tiles_drawn = P.drawn;
        }
        return (int)VISFS_BA_OK;
    });
}

int visfs_map_download(visfs_map* m, uint16_t* cells, uint8_t* count) {
    if (!m) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(m, [&]() -> int {
        if (!m->have) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "no composed grid: call visfs_map_compose first");
        const size_t n = (size_t)m->G.nx * m->G.ny;
        if (!m->device) {
            if (cells) std::memcpy(cells, m->h_cells.data(), n * 2);
            if (count) std::memcpy(count, m->h_count.data(), n);
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(m, hipSetDevice(m->dev));
        if (cells) HIP_TRY(m, hipMemcpyAsync(cells, m->d_cells.get(), n * 2, hipMemcpyDeviceToHost, m->stream));
        if (count) HIP_TRY(m, hipMemcpyAsync(count, m->d_count.get(), n, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(m, hipStreamSynchronize(m->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_stack_create_from_map(visfs_map* m, int32_t depth, visfs_scan_stack** out) {
    if (!m || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(m, [&]() -> int {
        if (depth < 1 || depth > VISFS_SCAN_FAST_MAX_DEPTH) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "the depth must lie in [1, 16]");
        if (!m->have) return fail(m, VISFS_BA_ERR_BAD_ARGUMENT, "no composed grid: call visfs_map_compose first");
        GridView g;
        g.cells = m->device ? m->d_cells.get() : m->h_cells.data(); g.nx = m->G.nx; g.ny = m->G.ny;
        std::string why;
        const int rc = visfs_internal_stack_from_view(m->device, m->dev, m->stream, m->G, g, depth, out, &why);
        if (rc != VISFS_BA_OK) return fail(m, rc, why);
        return (int)VISFS_BA_OK;
    });
}

int visfs_map_pose_from_anchor(const double a[3], const double b[3], double out[3]) {
    if (!a || !b || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!pose_ok(a) || !pose_ok(b)) return VISFS_BA_ERR_BAD_ARGUMENT;
    const double yaw = b[2] - a[2], c = std::cos(yaw), s = std::sin(yaw);
    out[0] = b[0] - (c * a[0] - s * a[1]);
    out[1] = b[1] - (s * a[0] + c * a[1]);
    out[2] = yaw;
    return VISFS_BA_OK;
}

int visfs_map_hook_odds_table(int32_t table[32768]) {
    if (!table) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int { const std::vector<int32_t> L = odds_table(); std::memcpy(table, L.data(), kValues * sizeof(int32_t)); return (int)VISFS_BA_OK; });
}

int visfs_map_plan(int32_t n, const visfs_submap_info* tile_limits, const double* poses, const visfs_map_params* p, visfs_submap_info* limits,
                   int32_t* boxes, int32_t* tiles_drawn) {
    if (n < 0 || (n > 0 && (!tile_limits || !poses)) || !p) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(nullptr, [&]() -> int {
        if (n > VISFS_MAP_MAX_TILES) return (int)VISFS_BA_ERR_UNSUPPORTED;
        std::vector<PlanTile> tiles((size_t)n);
        for (int32_t k = 0; k < n; ++k) {
            tiles[(size_t)k].L = submap::limits_of(tile_limits[k]);
            const Limits& L = tiles[(size_t)k].L;
            if (!pose_ok(poses + 3 * (size_t)k) || !limits_ok(L.res, L.max_x, L.max_y, L.nx, L.ny)) return (int)VISFS_BA_ERR_BAD_ARGUMENT;
            for (int i = 0; i < 3; ++i) tiles[(size_t)k].pose[i] = poses[3 * (size_t)k + i];
        }
        Plan P;
        const char* why = "";
        const int rc = make_plan(*p, tiles, P, &why);
        if (rc != VISFS_BA_OK) return rc;
        if (limits) fill_info(P, *limits);
        if (boxes)
            for (int32_t k = 0; k < n; ++k) {
                const TileRec& r = P.recs[(size_t)k];
                boxes[4 * k] = r.bx0; boxes[4 * k + 1] = r.by0; boxes[4 * k + 2] = r.bx1; boxes[4 * k + 3] = r.by1;
            }
        if (tiles_drawn) *tiles_drawn = P.drawn;
        return (int)VISFS_BA_OK;
    });
}

int visfs_map_last_counts(const visfs_map* m, int32_t* launches, int32_t* copies, int32_t* waits) {
    return m ? m->counts.read(launches, copies, waits) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

}  // extern "C"
