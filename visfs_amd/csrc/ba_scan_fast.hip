// Branch-and-bound scan matching over frozen grid stacks (include/visfs_scan_fast.h).
//
// A stack is P_0 = scan::cell_gain of one grid and its window-maximum levels P_1 .. P_(depth-1), each stored with its low-side
// extension (ba_scan_fast.hpp).  Building it is one launch per level:
//   k_fast_base    P_0 from the grid's cells (through the GridView's offsets), one work item per cell;
//   k_fast_up      P_h from P_(h-1), one work item per stored cell.
// A match on a device stack is a scan group of one: visfs_scan_stack_match checks the call, makes its search and runs the one launch
// sequence there is (device_run, ba_scan_group.hip) with m = 1 on the stack's own call block: one upload (points, rotation table,
// a member table of one), H + 5 launches on the stack's stream whatever the data, one download (the Ctrl record) and one wait.  What
// is the single call's own is its reading of that record: an overflow or an empty result fails the call under the single call's
// texts and leaves the hook's arenas and the last record as they were.  All sums are int32, so no reduction or append order can
// show in a result.  The one-core twin (host_search) runs the same schedule through the same functions of ba_scan_fast.hpp.  The
// stack object, the search of one call, the call block and the kernels' bodies are in ba_scan_stack.hpp; this file defines the host
// functions declared there, the launch sequence excepted.
#include "ba_scan_stack.hpp"
#include "ba_scan_stack_access.hpp"
#include "ba_host.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <new>
#include <string>
#include <utility>

#pragma clang fp contract(off)

using namespace scanfast;
using namespace host;
using scan::Plan;
using submap::GridView;
using submap::Limits;

namespace scanfast {

__global__ __launch_bounds__(kThreads) void k_fast_base(GridView g, int32_t nx, int64_t total, uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t y = (int32_t)(i / nx), x = (int32_t)(i - (int64_t)y * nx);
    out[i] = (uint16_t)scan::cell_gain(g, x, y);
}

__global__ __launch_bounds__(kThreads) void k_fast_up(LevelView lo, int32_t w, int32_t e_hi, int32_t half, int64_t total, uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int32_t sy = (int32_t)(i / w), sx = (int32_t)(i - (int64_t)sy * w);
    out[i] = level_up(lo, e_hi, half, sx, sy);
}

}  // namespace scanfast

// ---------------------------------------------------------------- the stack object
namespace {



// The levels' sizes and places; VISFS_BA_ERR_UNSUPPORTED beyond 1 GiB.
int stack_layout(visfs_scan_stack* st) {
    size_t items = 0;
    for (int32_t h = 0; h < st->depth; ++h) {
        const int64_t e = ((int64_t)1 << h) - 1, w = st->L.nx + e, ht = st->L.ny + e;
        st->off[h] = items;
        st->lv.v[h].w = (int32_t)w; st->lv.v[h].ht = (int32_t)ht; st->lv.v[h].e = (int32_t)e;
        items += ((size_t)(w * ht) + 127) & ~size_t(127);                  // every level starts on 256 bytes
        if ((int64_t)items * 2 > (int64_t)VISFS_SCAN_FAST_MAX_BYTES) return fail(st, VISFS_BA_ERR_UNSUPPORTED, "the levels together exceed 1 GiB");
    }
    st->bytes = (int64_t)items * 2;
    return VISFS_BA_OK;
}

// `g`: the grid in the memory of the stack's flavour (device: read on the stack's stream)
int stack_build(visfs_scan_stack* st, const GridView& g) {
    int rc = stack_layout(st);
    if (rc != VISFS_BA_OK) return rc;
    const size_t items = (size_t)(st->bytes / 2);
    if (!st->device) {
        st->h_mem.assign(items, 0);
        for (int32_t h = 0; h < st->depth; ++h) st->lv.v[h].p = st->h_mem.data() + st->off[h];
        uint16_t* p0 = st->h_mem.data();
        for (int32_t y = 0; y < st->L.ny; ++y)
            for (int32_t x = 0; x < st->L.nx; ++x) p0[(size_t)y * st->L.nx + x] = (uint16_t)scan::cell_gain(g, x, y);
        for (int32_t h = 1; h < st->depth; ++h) {
            const LevelView& hi = st->lv.v[h];
            uint16_t* o = st->h_mem.data() + st->off[h];
            for (int32_t sy = 0; sy < hi.ht; ++sy)
                for (int32_t sx = 0; sx < hi.w; ++sx) o[(size_t)sy * hi.w + sx] = level_up(st->lv.v[h - 1], hi.e, 1 << (h - 1), sx, sy);
        }
        return VISFS_BA_OK;
    }
    int cus = 0;
    HIP_TRY(&st->err, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, st->dev));
    st->blocks = std::max(1, cus) * 8;
    RC_TRY(st->d_mem.alloc(&st->err, items));
    for (int32_t h = 0; h < st->depth; ++h) st->lv.v[h].p = st->d_mem.get() + st->off[h];
    const int64_t n0 = (int64_t)st->L.nx * st->L.ny;
    hipLaunchKernelGGL(k_fast_base, dim3(blocks_for(n0, kThreads)), dim3(kThreads), 0, st->stream, g, st->L.nx, n0, st->d_mem.get());
    HIP_TRY(&st->err, hipGetLastError());
    for (int32_t h = 1; h < st->depth; ++h) {
        const LevelView& hi = st->lv.v[h];
        const int64_t nh = (int64_t)hi.w * hi.ht;
        hipLaunchKernelGGL(k_fast_up, dim3(blocks_for(nh, kThreads)), dim3(kThreads), 0, st->stream, st->lv.v[h - 1], hi.w, hi.e, 1 << (h - 1), nh,
                           st->d_mem.get() + st->off[h]);
        HIP_TRY(&st->err, hipGetLastError());
    }
    HIP_TRY(&st->err, hipStreamSynchronize(st->stream));                          // the source grid may change or go from here on
    return VISFS_BA_OK;
}

// The stack of a grid in host memory: its device copy goes once the stream has been waited for, however the build ended.
int stack_build_uploaded(visfs_scan_stack* st, GridView g) {
    struct Wait { hipStream_t stream; ~Wait() { (void)hipStreamSynchronize(stream); } };
    const size_t n = (size_t)g.nx * g.ny;
    DeviceBuf<uint16_t> tmp;
    HIP_TRY(&st->err, hipSetDevice(st->dev));
    RC_TRY(tmp.alloc(&st->err, n));
    const Wait before_tmp_goes{ st->stream };
    HIP_TRY(&st->err, hipMemcpyAsync(tmp.get(), g.cells, n * 2, hipMemcpyHostToDevice, st->stream));
    g.cells = tmp.get();
    return stack_build(st, g);
}

}  // namespace

// ---------------------------------------------------------------- the search of one call (shared with ba_scan_group.hip)
namespace scanfast {

int make_search(const visfs_scan_stack* st, const visfs_scan_stack_params& p, const double g[3], int32_t n, const double* xyz, Search& s,
                const char** why) {
    Plan& P = s.P;
    P.L = st->L; P.gx = g[0]; P.gy = g[1]; P.gyaw = g[2]; P.n = n;
    double step, fa, fl;
    if (!scan::plan_search(st->L.res, p.linear_search_window, p.angular_search_window, n, xyz, step, fa, fl)) { *why = "the scan's range overflows"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (!(fl <= (double)VISFS_SCAN_FAST_MAX_LINEAR)) { *why = "the linear window spans more than 512 cells"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (!(2.0 * fa + 1.0 <= (double)VISFS_SCAN_FAST_MAX_SCANS)) { *why = "the angular window holds more than 1025 rotations"; return VISFS_BA_ERR_UNSUPPORTED; }
    P.step = step; P.na = (int32_t)fa; P.nl = (int32_t)fl; P.S = 2 * P.na + 1; P.Lw = 2 * P.nl + 1;
    if ((int64_t)P.S * n > (int64_t)VISFS_SCAN_FAST_MAX_CELLS) { *why = "more than 2^22 cells (rotations times points)"; return VISFS_BA_ERR_UNSUPPORTED; }
    int32_t h = 0;
    while (h < st->depth - 1 && (1 << h) < P.Lw) ++h;
    s.H = h; s.mH = nodes_per_axis(P.Lw, h);
    if ((int64_t)P.S * s.mH * s.mH > (int64_t)VISFS_SCAN_FAST_MAX_TOP_NODES) { *why = "more than 2^22 nodes at the top level: the stack is too shallow for this window"; return VISFS_BA_ERR_UNSUPPORTED; }
    s.cap = p.frontier_capacity;
    scan::plan_tables(xyz, P);
    return VISFS_BA_OK;
}

std::string overflow_text(int32_t level, int32_t cap) {
    return "frontier overflow at level " + std::to_string(level) + ": more than " + std::to_string(cap) + " nodes kept";
}

void finish(const Search& s, const visfs_scan_stack_params& p, int32_t index, int32_t Q, visfs_scan_stack_result* out) {
    const double score = scan::candidate_score(Q, s.P.n, 1.0);
    scan::fill_result(s.P, index, score, Q, out->match);
    out->match.matched = score >= p.min_score ? 1 : 0;
    out->depth_used = s.H + 1;
}

void no_points(const double g[3], visfs_scan_stack_result* out) {
    std::memset(out, 0, sizeof *out);
    out->match.x = g[0]; out->match.y = g[1]; out->match.yaw = g[2];
}

int check_call(const visfs_scan_stack_params& p, const double g[3], int32_t n, const double* xyz, const char** why) {
    if (n > VISFS_SCAN_FAST_MAX_POINTS) { *why = "more than 16384 points"; return VISFS_BA_ERR_UNSUPPORTED; }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(g[i])) { *why = "the guess is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    for (int64_t i = 0; i < 3 * (int64_t)n; ++i) if (!std::isfinite(xyz[i])) { *why = "a point is not finite"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (!std::isfinite(p.linear_search_window) || !std::isfinite(p.angular_search_window) || p.linear_search_window < 0.0 || p.angular_search_window < 0.0) {
        *why = "the search windows must be finite and not negative"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    if (std::isnan(p.min_score)) { *why = "min_score is not a number"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p.frontier_capacity < 4 || p.frontier_capacity > VISFS_SCAN_FAST_MAX_FRONTIER) { *why = "frontier_capacity must lie in [4, 2^26]"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    return VISFS_BA_OK;
}

// the scan's node sum, sequentially
static int32_t host_node_sum(const int32_t* c, int32_t n, const LevelView& v, int32_t xo, int32_t yo) {
    int32_t q = 0;
    for (int32_t i = 0; i < n; ++i) q += level_read(v, c[2 * i] + xo, c[2 * i + 1] + yo);
    return q;
}

int host_search(const Levels& lv, const Search& s, Last& now, std::string& why) {
    const Plan& P = s.P;
    const int32_t n = P.n, nl = P.nl, L = P.Lw, H = s.H, mH = s.mH, per = mH * mH;
    std::vector<int32_t> cells(2 * (size_t)P.S * n);
    for (int32_t k = 0; k < P.S; ++k)
        for (int32_t i = 0; i < n; ++i)
            scan::discretise(P.rot[2 * k], P.rot[2 * k + 1], P.pts[2 * i], P.pts[2 * i + 1], P.gx, P.gy, P.L.res, P.L.max_x, P.L.max_y,
                             cells[2 * ((size_t)k * n + i)], cells[2 * ((size_t)k * n + i) + 1]);
    auto scan_cells = [&](int32_t k) { return cells.data() + 2 * (size_t)k * n; };
    now = Last();
    now.S = P.S; now.L = L; now.n = n; now.H = H; now.mH = mH;
    now.bounds.resize((size_t)s.top());
    for (int32_t id = 0; id < s.top(); ++id) {
        int32_t k, i, j;
        node_decode(mH, id, k, i, j);
        now.bounds[id] = host_node_sum(scan_cells(k), n, lv.v[H], -nl + (i << H), -nl + (j << H));
    }
    int32_t B = 0;
    for (int32_t k = 0; k < P.S; ++k) {                                    // the greedy descents
        int32_t u = -1, id = INT_MAX;
        for (int32_t a = 0; a < per; ++a) if (better(now.bounds[(size_t)k * per + a], a, u, id)) { u = now.bounds[(size_t)k * per + a]; id = a; }
        int32_t i = id / mH, j = id % mH, cur = u;
        for (int32_t h = H; h >= 1; --h) {
            const int32_t m = nodes_per_axis(L, h - 1);
            int32_t bu = -1, bw = 0;
            for (int w = 0; w < 4; ++w) {
                const int32_t ci = 2 * i + (w >> 1), cj = 2 * j + (w & 1);
                if (ci >= m || cj >= m) continue;
                const int32_t U = host_node_sum(scan_cells(k), n, lv.v[h - 1], -nl + (ci << (h - 1)), -nl + (cj << (h - 1)));
                if (U > bu) { bu = U; bw = w; }
            }
            cur = bu; i = 2 * i + (bw >> 1); j = 2 * j + (bw & 1);
        }
        if (cur > B) B = cur;
    }
    now.c.B = B;
    std::vector<int2> F, G;
    now.c.scored[H] = s.top();
    for (int32_t id = 0; id < s.top(); ++id)
        if (now.bounds[id] >= B) { ++now.c.kept[H]; if ((int32_t)F.size() < s.cap) F.push_back(make_int2(id, now.bounds[id])); }
    if (now.c.kept[H] > s.cap) { why = overflow_text(H, s.cap); return VISFS_BA_ERR_UNSUPPORTED; }
    for (int32_t h = H; h >= 1; --h) {
        const int32_t mh = nodes_per_axis(L, h), ml = nodes_per_axis(L, h - 1), half = 1 << (h - 1);
        G.clear();
        for (const int2& e : F) {
            int32_t k, i, j;
            node_decode(mh, e.x, k, i, j);
            for (int a = 0; a < 4; ++a) {
                const int32_t ci = 2 * i + (a >> 1), cj = 2 * j + (a & 1);
                if (ci >= ml || cj >= ml) continue;
                const int32_t U = host_node_sum(scan_cells(k), n, lv.v[h - 1], -nl + ci * half, -nl + cj * half);
                ++now.c.scored[h - 1];
                if (U < B) continue;
                ++now.c.kept[h - 1];
                if ((int32_t)G.size() < s.cap) G.push_back(make_int2(node_id(ml, k, ci, cj), U));
            }
        }
        if (now.c.kept[h - 1] > s.cap) { why = overflow_text(h - 1, s.cap); return VISFS_BA_ERR_UNSUPPORTED; }
        F.swap(G);
    }
    int32_t u = -1, id = INT_MAX;
    for (const int2& e : F) if (better(e.y, e.x, u, id)) { u = e.y; id = e.x; }
    if (id == INT_MAX) { why = "the search returned no candidate"; return VISFS_BA_ERR_DEVICE; }
    now.c.best_index = id; now.c.best_sum = u;
    std::sort(F.begin(), F.end(), [](const int2& a, const int2& b) { return a.x < b.x; });
    now.survivors = (int32_t)F.size();
    now.surv.swap(F);
    now.have = true;
    return VISFS_BA_OK;
}

Last device_last(const Search& s, const Ctrl& c) {
    Last l;
    l.have = true; l.S = s.P.S; l.L = s.P.Lw; l.n = s.P.n; l.H = s.H; l.mH = s.mH; l.survivors = c.kept[0]; l.c = c;
    return l;
}

int match_download(bool device, int dev, hipStream_t stream, const CallBlock& b, int64_t member, const Last& l, std::string& why, int32_t header[8],
                   int32_t scored[16], int32_t kept[16], int64_t bounds_cap, int32_t* bounds, int64_t survivors_cap, int32_t* survivors) {
    std::memset(header, 0, 8 * sizeof(int32_t));
    if (!l.have) return VISFS_BA_OK;
    const int32_t per = l.mH * l.mH;
    const int64_t nb = (int64_t)l.S * per;
    header[0] = l.S; header[1] = l.L; header[2] = l.n; header[3] = l.H; header[4] = per; header[5] = l.survivors; header[6] = l.c.B;
    if (scored) std::memcpy(scored, l.c.scored, sizeof l.c.scored);
    if (kept) std::memcpy(kept, l.c.kept, sizeof l.c.kept);
    if ((bounds && bounds_cap < nb) || (survivors && survivors_cap < l.survivors)) { why = "the hook's arrays are too small"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (!device) {
        if (bounds) std::memcpy(bounds, l.bounds.data(), (size_t)nb * sizeof(int32_t));
        if (survivors) std::memcpy(survivors, l.surv.data(), (size_t)l.survivors * sizeof(int2));
        return VISFS_BA_OK;
    }
    HIP_TRY(&why, hipSetDevice(dev));
    if (bounds) HIP_TRY(&why, hipMemcpyAsync(bounds, b.bnd[1].get() + member * b.top, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (survivors) HIP_TRY(&why, hipMemcpyAsync(survivors, b.fr[2].get() + member * b.cap, (size_t)l.survivors * sizeof(int2), hipMemcpyDeviceToHost, stream));
    HIP_TRY(&why, hipStreamSynchronize(stream));
    if (survivors) {                                                       // the device appends unordered
        int2* sv = reinterpret_cast<int2*>(survivors);
        std::sort(sv, sv + l.survivors, [](const int2& u, const int2& v) { return u.x < v.x; });
    }
    return VISFS_BA_OK;
}

}  // namespace scanfast

namespace {

int host_match(visfs_scan_stack* st, Search& s, const visfs_scan_stack_params& p, visfs_scan_stack_result* out) {
    Last now;
    std::string why;
    const int rc = host_search(st->lv, s, now, why);
    if (rc != VISFS_BA_OK) return fail(st, rc, why);
    finish(s, p, now.c.best_index, now.c.best_sum, out);
    st->last = std::move(now);
    return VISFS_BA_OK;
}

int check_depth(int32_t depth) { return depth >= 1 && depth <= kMaxDepth; }

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_scan_fast_abi_version(void) { return VISFS_SCAN_FAST_ABI_VERSION; }

void visfs_scan_stack_default_params(visfs_scan_stack_params* p) {
    if (!p) return;
    p->linear_search_window = 7.0;
    p->angular_search_window = 30.0 * 3.14159265358979323846 / 180.0;
    p->min_score = 0.0;
    p->frontier_capacity = 1 << 20;
}

int visfs_scan_stack_create(visfs_submaps* s, int32_t index, int32_t depth, visfs_scan_stack** out) {
    if (!s || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(s, [&]() -> int {
        if (!check_depth(depth)) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "the depth must lie in [1, 16]");
        submap::ScanAccess acc;
        int rc = visfs_internal_scan_access(s, index, &acc);
        if (rc != VISFS_BA_OK) return rc;
        if (index < 0 || index >= acc.count) return visfs_internal_scan_fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "sub-map index out of range");
        visfs_scan_stack* st = new visfs_scan_stack();
        st->device = acc.device; st->dev = acc.dev; st->stream = acc.stream;
        st->L = acc.L; st->depth = depth;
        rc = stack_build(st, acc.grid);
        if (rc != VISFS_BA_OK) { (void)visfs_internal_scan_fail(s, rc, st->err.c_str()); delete st; return rc; }
        *out = st;
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_stack_create_from_grid(visfs_ba_handle* h, const visfs_submap_info* lim, const uint16_t* cells, int32_t depth, visfs_scan_stack** out) {
    if (!lim || !cells || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        auto bad = [&](int rc, const char* why) { if (h) visfs_internal_set_error(h, why); return rc; };
        if (!check_depth(depth)) return bad(VISFS_BA_ERR_BAD_ARGUMENT, "the depth must lie in [1, 16]");
        if (!(lim->resolution > 0.0) || !std::isfinite(lim->resolution) || !std::isfinite(lim->max_x) || !std::isfinite(lim->max_y) ||
            lim->num_x_cells < 1 || lim->num_y_cells < 1)
            return bad(VISFS_BA_ERR_BAD_ARGUMENT, "the limits need a positive resolution, a finite corner and at least one cell per axis");
        if ((int64_t)lim->num_x_cells * lim->num_y_cells * 2 > (int64_t)VISFS_SCAN_FAST_MAX_BYTES) return bad(VISFS_BA_ERR_UNSUPPORTED, "the levels together exceed 1 GiB");
        visfs_scan_stack* st = new visfs_scan_stack();
        st->L.res = lim->resolution; st->L.max_x = lim->max_x; st->L.max_y = lim->max_y; st->L.nx = lim->num_x_cells; st->L.ny = lim->num_y_cells;
        st->depth = depth;
        GridView g;
        g.cells = cells; g.nx = st->L.nx; g.ny = st->L.ny;
        int rc;
        if (!h) rc = stack_build(st, g);
        else {
            st->device = true; st->dev = visfs_internal_device(h); st->stream = visfs_internal_stream(h);
            rc = stack_build_uploaded(st, g);
        }
        if (rc != VISFS_BA_OK) { (void)bad(rc, st->err.c_str()); delete st; return rc; }
        *out = st;
        return (int)VISFS_BA_OK;
    });
}

void visfs_scan_stack_destroy(visfs_scan_stack* st) { delete st; }

const char* visfs_scan_stack_last_error(const visfs_scan_stack* st) { return st ? st->err.c_str() : "null stack"; }

int visfs_scan_stack_describe(const visfs_scan_stack* st, visfs_scan_stack_info* info) {
    if (!st || !info) return VISFS_BA_ERR_BAD_ARGUMENT;
    info->resolution = st->L.res; info->max_x = st->L.max_x; info->max_y = st->L.max_y;
    info->num_x_cells = st->L.nx; info->num_y_cells = st->L.ny; info->depth = st->depth; info->device = st->device ? 1 : 0;
    info->bytes = st->bytes;
    return VISFS_BA_OK;
}

int visfs_scan_stack_match(visfs_scan_stack* st, const visfs_scan_stack_params* p, const double g[3], int32_t n, const double* xyz,
                           visfs_scan_stack_result* out) {
    if (!st || !p || !g || !out || n < 0 || (n > 0 && !xyz)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(st, [&]() -> int {
        const char* why = "";
        int rc = check_call(*p, g, n, xyz, &why);
        if (rc != VISFS_BA_OK) return fail(st, rc, why);
        if (n == 0) { no_points(g, out); return (int)VISFS_BA_OK; }        // nothing to match: the guess back
        Search s;
        rc = make_search(st, *p, g, n, xyz, s, &why);
        if (rc != VISFS_BA_OK) return fail(st, rc, why);
        if (!st->device) return host_match(st, s, *p, out);
        int cur = 0;
        rc = device_run(st->blk, st->dev, st->stream, st->blocks, 1, &st, &s, &cur, st->err);
        if (rc != VISFS_BA_OK) return rc;
        const Ctrl& c = st->blk.ctrl_h()[0];
        if (c.overflow) return fail(st, VISFS_BA_ERR_UNSUPPORTED, overflow_text(c.overflow - 1, s.cap));
        if (c.best_index < 0 || (int64_t)c.best_index >= s.P.candidates()) return fail(st, VISFS_BA_ERR_DEVICE, "the search returned no candidate");
        st->blk.hand_over(cur, s);                                         // only now: a failed call leaves the hook's arenas and `last`
        finish(s, *p, c.best_index, c.best_sum, out);
        st->last = device_last(s, c);
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_stack_download_level(visfs_scan_stack* st, int32_t h, int64_t cap, uint16_t* out, int32_t dims[4]) {
    if (!st || !dims || cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(st, [&]() -> int {
        if (h < 0 || h >= st->depth) return fail(st, VISFS_BA_ERR_BAD_ARGUMENT, "the stack has no such level");
        const LevelView& v = st->lv.v[h];
        dims[0] = v.w; dims[1] = v.ht; dims[2] = v.e; dims[3] = 0;
        if (!out) return (int)VISFS_BA_OK;
        const int64_t items = (int64_t)v.w * v.ht;
        if (cap < items) return fail(st, VISFS_BA_ERR_BAD_ARGUMENT, "the hook's array is too small");
        if (!st->device) { std::memcpy(out, v.p, (size_t)items * 2); return (int)VISFS_BA_OK; }
        HIP_TRY(&st->err, hipSetDevice(st->dev));
        HIP_TRY(&st->err, hipMemcpyAsync(out, v.p, (size_t)items * 2, hipMemcpyDeviceToHost, st->stream));
        HIP_TRY(&st->err, hipStreamSynchronize(st->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_stack_match_download(visfs_scan_stack* st, int32_t header[8], int32_t scored[16], int32_t kept[16], int64_t bounds_cap,
                                    int32_t* bounds, int64_t survivors_cap, int32_t* survivors) {
    if (!st || !header || bounds_cap < 0 || survivors_cap < 0) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(st, [&]() -> int {
        return match_download(st->device, st->dev, st->stream, st->blk, 0, st->last, st->err, header, scored, kept, bounds_cap, bounds, survivors_cap,
                              survivors);
    });
}

}  // extern "C"

// ====================================================================== what the global map (ba_map.hip) borrows
int visfs_internal_stack_from_view(bool device, int dev, hipStream_t stream, const Limits& L, const GridView& g, int32_t depth,
                                   visfs_scan_stack** out, std::string* err) {
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        visfs_scan_stack* st = new visfs_scan_stack();
        st->device = device; st->dev = dev; st->stream = stream;
        st->L = L; st->depth = depth;
        auto run = [&]() -> int {
            if (device) HIP_TRY(&st->err, hipSetDevice(dev));
            return stack_build(st, g);
        };
        const int rc = run();
        if (rc != VISFS_BA_OK) { if (err) *err = st->err; delete st; return rc; }
        *out = st;
        return (int)VISFS_BA_OK;
    });
}
