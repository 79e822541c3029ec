// Corner extraction on the resident level-0 images of a visfs_flow object (include/visfs_corners.h).
//
// cv::goodFeaturesToTrack with OpenCV's defaults and the mask of the reference's Tracker::getMask (Tracker.cpp:116-141, :181, :327),
// two ways over the arithmetic of ba_corners.hpp:
//   * host restatement (objects of visfs_flow_create_host): every pixel and every candidate in sequence on one core;
//   * device, four launches on the stream of the owning handle and no host round trip between them:
//       k_corner_response    a 32 x 8 tile with a 2-pixel apron of the uint8 image in LDS -> Sobel -> products -> 3 x 3 box sums ->
//                            the response map; the mask raster (every pixel against the drawn discs) and the masked maximum (wave
//                            reduce, one atomic max per workgroup) ride in the same launch
//       k_corner_candidates  threshold, 3 x 3 maximum test, mask; appends the 64-bit keys through a per-wave ballot count
//       k_corner_sort        rank sort: a candidate's place is the number of greater keys (the keys are unique), counted through
//                            LDS tiles by 64 candidates x 4 slices per workgroup; right for any count up to (w - 2)(h - 2)
//       k_corner_select      one workgroup: the accepted list in LDS, 1024 sorted candidates at a time against it, the survivors
//                            resolved in order by one wavefront, which is exactly the serial walk
// Which discs are drawn depends on the disc list alone; that short serial pass runs on the host before the launches, for both ways.
#include "ba_corners.hpp"
#include "ba_flow_object.hpp"
#include "ba_group.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_corners.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <new>

using namespace flow;
using namespace host;

// ---------------------------------------------------------------- kernels
namespace flow {

constexpr int CR_T = 256;
constexpr int CT_X = 32, CT_Y = 8;             // the response tile: one thread per pixel
constexpr int kSortTile = 1024;                // keys per LDS tile of the rank sort
constexpr int kSortGrid = 2048;                // workgroups of the rank sort (each strides over chunks of 64 candidates)
constexpr int kSelT = 1024;

struct CornerDev {                             // device words of a call, copied out with the corners behind them
    uint32_t count;                            // candidates
    uint32_t max_bits;                         // ordered_bits of the masked maximum, 0: none
    int32_t n_out;
    int32_t pad;
};

__device__ __forceinline__ void corner_response_body(const uint8_t* __restrict__ px, int w, int h, const Disc* __restrict__ discs,
                                                     int n_discs, const int32_t* __restrict__ hw, float* __restrict__ eig,
                                                     uint8_t* __restrict__ mask, CornerDev* st, const int32_t* dev_args) {
    if (dev_args) {                            // a resident caller: { n_discs, max_corners } of this call live in device memory
        if (dev_args[1] <= 0) return;          // nothing is wanted: no candidate is counted and the selection returns none
        n_discs = dev_args[0];
    }
    __shared__ int sI[CT_Y + 4][CT_X + 5];
    __shared__ int sDx[CT_Y + 2][CT_X + 3];
    __shared__ int sDy[CT_Y + 2][CT_X + 3];
    __shared__ uint32_t sMax[CR_T / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * CT_X, y0 = blockIdx.y * CT_Y;
    // the image from -1 to w and -1 to h is all a derivative inside the image reads
    for (int i = tid; i < (CT_Y + 4) * (CT_X + 4); i += CR_T) {
        const int ty = i / (CT_X + 4), tx = i - ty * (CT_X + 4);
        const int gx = x0 - 2 + tx, gy = y0 - 2 + ty;
        int v = 0;
        if (gx >= -1 && gx <= w && gy >= -1 && gy <= h) v = px[(int64_t)reflect101(gy, h) * w + reflect101(gx, w)];
        sI[ty][tx] = v;
    }
    __syncthreads();
    for (int i = tid; i < (CT_Y + 2) * (CT_X + 2); i += CR_T) {
        const int ty = i / (CT_X + 2), tx = i - ty * (CT_X + 2);
        const int gx = x0 - 1 + tx, gy = y0 - 1 + ty;
        int dx = 0, dy = 0;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            dx = (sI[ty][tx + 2] + 2 * sI[ty + 1][tx + 2] + sI[ty + 2][tx + 2]) - (sI[ty][tx] + 2 * sI[ty + 1][tx] + sI[ty + 2][tx]);
            dy = (sI[ty + 2][tx] + 2 * sI[ty + 2][tx + 1] + sI[ty + 2][tx + 2]) - (sI[ty][tx] + 2 * sI[ty][tx + 1] + sI[ty][tx + 2]);
        }
        sDx[ty][tx] = dx;
        sDy[ty][tx] = dy;
    }
    __syncthreads();
    const int lx = tid % CT_X, ly = tid / CT_X;
    const int X = x0 + lx, Y = y0 + ly;
    uint32_t m = 0;
    if (X < w && Y < h) {
        // a neighbour outside the image is the derivative at the reflected pixel, which lies in this tile's range
        int32_t sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const int sy = reflect101(Y + j, h) - (y0 - 1);
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                const int sx = reflect101(X + i, w) - (x0 - 1);
                const int dx = sDx[sy][sx], dy = sDy[sy][sx];
                sxx += dx * dx;
                sxy += dx * dy;
                syy += dy * dy;
            }
        }
        const float e = min_eig_response(sxx, sxy, syy);
        const int64_t at = (int64_t)Y * w + X;
        eig[at] = e;
        const bool free_px = !masked(discs, n_discs, hw, X, Y);
        mask[at] = free_px ? 255 : 0;
        if (free_px) m = ordered_bits(e);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    if ((tid & 63) == 0) sMax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < CR_T / 64; ++k) m = sMax[k] > m ? sMax[k] : m;
        if (m) atomicMax(&st->max_bits, m);
    }
}

__global__ __launch_bounds__(CR_T) void k_corner_response(const uint8_t* __restrict__ px, int w, int h, const Disc* __restrict__ discs,
                                                          int n_discs, const int32_t* __restrict__ hw, float* __restrict__ eig,
                                                          uint8_t* __restrict__ mask, CornerDev* st) {
    corner_response_body(px, w, h, discs, n_discs, hw, eig, mask, st, nullptr);
}

// The batched forms (tracker groups): member blockIdx.z, its arguments read from the group's table.  A member that takes no part in
// the extraction (skip) leaves at once; the words of every other member's call are zeroed by k_corner_reset_g in front.
__global__ __launch_bounds__(64) void k_corner_reset_g(const CornerRec* __restrict__ recs, int n) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n || recs[m].skip) return;
    *recs[m].st = CornerDev{ 0u, 0u, 0, 0 };
}

__global__ __launch_bounds__(CR_T) void k_corner_response_g(const CornerRec* __restrict__ recs, int w, int h) {
    const CornerRec r = recs[blockIdx.z];
    if (r.skip) return;
    corner_response_body(r.px, w, h, r.discs, 0, r.hw, r.eig, r.mask, r.st, r.args);
}

__device__ __forceinline__ void corner_candidates_body(const float* __restrict__ eig, const uint8_t* __restrict__ mask, int w, int h,
                                                       double quality, CornerDev* st, uint64_t* __restrict__ keys,
                                                       const int32_t* dev_args) {
    if (dev_args && dev_args[1] <= 0) return;  // the response map was not made
    const int64_t i = (int64_t)blockIdx.x * CR_T + threadIdx.x;
    const float t = quality_threshold(from_ordered_bits(st->max_bits), quality);
    bool cand = false;
    float v = 0.0f;
    if (i < (int64_t)w * h) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
            v = eig[i];
            if (v > t && v != 0.0f && mask[i] != 0) {
                cand = true;
#pragma unroll
                for (int j = -1; j <= 1; ++j)
#pragma unroll
                    for (int k = -1; k <= 1; ++k) {
                        const float nb = eig[i + (int64_t)j * w + k];
                        const float nt = nb > t ? nb : 0.0f;
                        if (nt > v) cand = false;
                    }
            }
        }
    }
    const unsigned long long b = __ballot(cand);
    if (b == 0) return;
    const int lane = threadIdx.x & 63;
    const int first = __ffsll(b) - 1;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(&st->count, (uint32_t)__popcll(b));
    base = __shfl(base, first, 64);
    if (cand) keys[base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = corner_key(v, (uint32_t)i);
}

__global__ __launch_bounds__(CR_T) void k_corner_candidates(const float* __restrict__ eig, const uint8_t* __restrict__ mask, int w, int h,
                                                            double quality, CornerDev* st, uint64_t* __restrict__ keys) {
    corner_candidates_body(eig, mask, w, h, quality, st, keys, nullptr);
}

__global__ __launch_bounds__(CR_T) void k_corner_candidates_g(const CornerRec* __restrict__ recs, int w, int h, double quality) {
    const CornerRec r = recs[blockIdx.z];
    if (r.skip) return;
    corner_candidates_body(r.eig, r.mask, w, h, quality, r.st, r.keys, r.args);
}

// sorted[number of keys greater than k] = k.  A workgroup takes 64 candidates at a time (one per lane); its four wavefronts each
// count over a quarter of every LDS tile of keys.
__device__ __forceinline__ void corner_sort_body(const uint64_t* __restrict__ keys, const CornerDev* st, uint64_t* __restrict__ sorted) {
    __shared__ uint64_t tile[kSortTile];
    __shared__ uint32_t part[CR_T / 64][64];
    const uint32_t n = st->count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t c0 = blockIdx.x * 64u; c0 < n; c0 += gridDim.x * 64u) {
        const uint32_t mine = c0 + lane;
        const uint64_t k = mine < n ? keys[mine] : ~0ull;
        uint32_t greater = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += kSortTile) {
            __syncthreads();
            for (int q = tid; q < kSortTile; q += CR_T) tile[q] = t0 + q < n ? keys[t0 + q] : 0ull;     // 0 is below every key
            __syncthreads();
            const uint64_t* s = tile + wave * (kSortTile / 4);
#pragma unroll 8
            for (int q = 0; q < kSortTile / 4; ++q) greater += s[q] > k ? 1u : 0u;
        }
        part[wave][lane] = greater;
        __syncthreads();
        if (wave == 0 && mine < n) sorted[part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]] = k;
    }
}

__global__ __launch_bounds__(CR_T) void k_corner_sort(const uint64_t* __restrict__ keys, const CornerDev* st, uint64_t* __restrict__ sorted) {
    corner_sort_body(keys, st, sorted);
}

__global__ __launch_bounds__(CR_T) void k_corner_sort_g(const CornerRec* __restrict__ recs) {
    const CornerRec r = recs[blockIdx.z];
    if (r.skip) return;
    corner_sort_body(r.keys, r.st, r.sorted);
}

__device__ __forceinline__ void corner_select_body(const uint64_t* __restrict__ sorted, CornerDev* st, int w, int32_t gate,
                                                   int32_t max_corners, float* __restrict__ xy, const int32_t* dev_args) {
    if (dev_args) max_corners = dev_args[1] > 0 ? dev_args[1] : 0;
    __shared__ int32_t acc[kMaxCorners];       // accepted, x | y << 16
    __shared__ int32_t surv[kSelT];            // a chunk's survivors of the list as it stood when the chunk began, in order
    __shared__ int32_t wcount[kSelT / 64];
    __shared__ int32_t s_nacc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = st->count;
    int32_t nacc = 0;
    if (gate <= 1) {                           // no two pixels are closer than 1: the first max_corners of the order
        nacc = n < (uint32_t)max_corners ? (int32_t)n : max_corners;
        for (int a = tid; a < nacc; a += kSelT) {
            const uint32_t idx = (uint32_t)sorted[a];
            acc[a] = (int32_t)(idx % (uint32_t)w) | ((int32_t)(idx / (uint32_t)w) << 16);
        }
        __syncthreads();
    } else {
        for (uint32_t base = 0; base < n && nacc < max_corners; base += kSelT) {
            const uint32_t i = base + tid;
            bool alive = i < n;
            int32_t p = 0;
            if (alive) {
                const uint32_t idx = (uint32_t)sorted[i];
                p = (int32_t)(idx % (uint32_t)w) | ((int32_t)(idx / (uint32_t)w) << 16);
                for (int a = 0; a < nacc; ++a)
                    if (too_close(p, acc[a], gate)) { alive = false; break; }
            }
            const unsigned long long b = __ballot(alive);
            if (lane == 0) wcount[wave] = __popcll(b);
            __syncthreads();
            int32_t before = 0, nsurv = 0;
            for (int k = 0; k < kSelT / 64; ++k) {
                if (k < wave) before += wcount[k];
                nsurv += wcount[k];
            }
            if (alive) surv[before + __popcll(b & ((1ull << lane) - 1ull))] = p;
            __syncthreads();
            if (wave == 0) {
                const int32_t chunk_first = nacc;                                  // accepted since the chunk began: acc[chunk_first .. nacc)
                for (int32_t sb = 0; sb < nsurv && nacc < max_corners; sb += 64) {
                    bool live = sb + lane < nsurv;
                    const int32_t q = live ? surv[sb + lane] : 0;
                    if (live)
                        for (int a = chunk_first; a < nacc; ++a)
                            if (too_close(q, acc[a], gate)) { live = false; break; }
                    // the first survivor is accepted; the ones behind it meet it before their turn comes
                    for (;;) {
                        const unsigned long long lb = __ballot(live);
                        if (lb == 0 || nacc >= max_corners) break;
                        const int f = __ffsll(lb) - 1;
                        const int32_t qf = __shfl(q, f, 64);
                        if (lane == f) { acc[nacc] = q; live = false; }
                        ++nacc;
                        if (live && too_close(q, qf, gate)) live = false;
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                if (lane == 0) s_nacc = nacc;
            }
            __syncthreads();
            nacc = s_nacc;
        }
    }
    for (int a = tid; a < nacc; a += kSelT) {
        xy[2 * a] = (float)(acc[a] & 0xffff);
        xy[2 * a + 1] = (float)(acc[a] >> 16);
    }
    if (tid == 0) st->n_out = nacc;
}

__global__ __launch_bounds__(kSelT) void k_corner_select(const uint64_t* __restrict__ sorted, CornerDev* st, int w, int32_t gate,
                                                         int32_t max_corners, float* __restrict__ xy) {
    corner_select_body(sorted, st, w, gate, max_corners, xy, nullptr);
}

__global__ __launch_bounds__(kSelT) void k_corner_select_g(const CornerRec* __restrict__ recs, int w, int32_t gate) {
    const CornerRec r = recs[blockIdx.z];
    if (r.skip) return;
    corner_select_body(r.sorted, r.st, w, gate, 0, r.xy, r.args);
}

// ---------------------------------------------------------------- per-object state
struct CornerState {
    // the last call
    bool valid = false;
    int32_t n_discs = 0, n_candidates = 0;
    float max_val = 0.0f;
    std::vector<uint8_t> drawn;

    // the raster's discs of a call and their half-width tables
    std::vector<Disc> discs;
    std::vector<int32_t> hw;

    // host restatement
    std::vector<float> heig;
    std::vector<uint8_t> hmask;

    // device
    DeviceBuf<float> d_eig;
    DeviceBuf<uint8_t> d_mask;
    DeviceBuf<uint64_t> d_keys;        // appended, then sorted: 2 x (w - 2)(h - 2)
    uint64_t* d_sorted = nullptr;      // the second half of d_keys
    DeviceBuf<char> d_out;             // CornerDev, xy[kMaxCorners][2]
    PinnedBuf<char> h_out;
    Staged<char> disc;                 // Disc[n], hw[]; bytes
};

void corners_release(visfs_flow* f) {
    CornerState* c = f->corners;
    if (!c) return;
    if (f->device) {
        (void)hipSetDevice(f->dev);
        if (f->stream) (void)hipStreamSynchronize(f->stream);
    }
    delete c;                                  // its members free what they own
    f->corners = nullptr;
}

}  // namespace flow

namespace {

constexpr size_t kOutBytes = sizeof(CornerDev) + sizeof(float) * 2 * kMaxCorners;

size_t max_candidates(const visfs_flow* f) { return (size_t)std::max(f->w - 2, 0) * (size_t)std::max(f->h - 2, 0); }

// the first call of an object allocates; a call that fails here leaves the object without corner state
int ensure_state(visfs_flow* f) {
    if (f->corners) return VISFS_BA_OK;
    CornerState* c = new CornerState();
    f->corners = c;
    if (!f->device) return VISFS_BA_OK;
    const size_t n0 = (size_t)f->w * f->h, nc = std::max<size_t>(max_candidates(f), 1);
    const auto alloc = [&]() -> int {
        HIP_TRY(f, hipSetDevice(f->dev));
        RC_TRY(c->d_eig.alloc(f, n0));
        RC_TRY(c->d_mask.alloc(f, n0));
        RC_TRY(c->d_keys.alloc(f, 2 * nc));
        c->d_sorted = c->d_keys.get() + nc;
        RC_TRY(c->d_out.alloc(f, kOutBytes));
        return c->h_out.alloc(f, kOutBytes);
    };
    const int rc = alloc();
    if (rc != VISFS_BA_OK) corners_release(f);
    return rc;
}

int disc_reserve(visfs_flow* f, size_t bytes) {
    CornerState* c = f->corners;
    if (bytes <= c->disc.cap()) return VISFS_BA_OK;
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return c->disc.reserve(f, bytes, std::max<size_t>(2 * bytes, 16384));
}

int check_call(visfs_flow* f, int32_t slot, int32_t image, const visfs_corners_params* p, int32_t n_discs, const visfs_corners_disc* discs,
               int32_t capacity) {
    if (slot < 0 || slot > 1 || image < 0 || image > 1) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "slot or image out of range");
    if (f->w < 3 || f->h < 3) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the image is smaller than 3 x 3");    // one reflection must stay inside
    if (p->max_corners < 1) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "max_corners must be at least 1");
    if (p->max_corners > kMaxCorners) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "max_corners must not exceed 4096");
    if (p->max_corners > capacity) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "capacity is smaller than max_corners");
    if (!std::isfinite(p->quality_level) || !(p->quality_level > 0.0)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "quality_level must be finite and positive");
    if (!std::isfinite(p->min_distance) || !(p->min_distance >= 0.0)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "min_distance must be finite and not negative");
    for (int32_t i = 0; i < n_discs; ++i) {
        if (!std::isfinite(discs[i].x) || !std::isfinite(discs[i].y)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "a disc's centre is not finite");
        if (discs[i].radius < 0) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "a disc's radius is negative");
        if (discs[i].radius > kMaxRadius) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "a disc's radius must not exceed 32768");
    }
    if (f->frames < (slot == VISFS_FLOW_SLOT_CURRENT ? 1 : 2)) return fail(f, VISFS_BA_ERR_NOT_LOADED, "no frame in that slot");
    return VISFS_BA_OK;
}

// Tracker::getMask's draw decisions, in the order given: c->drawn, and the drawn discs that touch the image for the raster
void decide_discs(const visfs_flow* f, CornerState* c, int32_t n_discs, const visfs_corners_disc* discs) {
    c->drawn.assign((size_t)n_discs, 0);
    c->discs.clear();
    c->hw.clear();
    std::map<int32_t, int32_t> table;          // radius -> first entry of its half-widths
    for (int32_t i = 0; i < n_discs; ++i) {
        const int32_t cx = round_centre(discs[i].x), cy = round_centre(discs[i].y), r = discs[i].radius;
        const bool inside = cx >= 0 && cx < f->w && cy >= 0 && cy < f->h;
        if (inside && masked(c->discs.data(), (int)c->discs.size(), c->hw.data(), cx, cy)) continue;
        c->drawn[(size_t)i] = 1;
        if ((int64_t)cx + r < 0 || (int64_t)cx - r >= f->w || (int64_t)cy + r < 0 || (int64_t)cy - r >= f->h) continue;
        auto it = table.find(r);
        if (it == table.end()) {
            it = table.emplace(r, (int32_t)c->hw.size()).first;
            c->hw.resize(c->hw.size() + (size_t)r + 1);
            disc_halfwidth(r, c->hw.data() + it->second);
        }
        c->discs.push_back(Disc{ cx, cy, r, it->second });
    }
}

int32_t pack_xy(uint32_t index, int32_t w) { return (int32_t)(index % (uint32_t)w) | ((int32_t)(index / (uint32_t)w) << 16); }

void host_corners(visfs_flow* f, CornerState* c, const uint8_t* px, const visfs_corners_params& p, const Disc* discs, int n_discs,
                  const int32_t* hw, float* xy, int32_t* n_out) {
    const int w = f->w, h = f->h;
    const size_t n0 = (size_t)w * h;
    std::vector<int32_t> dxs(n0), dys(n0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int dx, dy;
            sobel_cell(px, w, h, x, y, dx, dy);
            dxs[(size_t)y * w + x] = dx; dys[(size_t)y * w + x] = dy;
        }
    c->heig.resize(n0); c->hmask.resize(n0);
    uint32_t max_bits = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int32_t sxx = 0, sxy = 0, syy = 0;
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i) {
                    const size_t at = (size_t)reflect101(y + j, h) * w + reflect101(x + i, w);
                    sxx += dxs[at] * dxs[at]; sxy += dxs[at] * dys[at]; syy += dys[at] * dys[at];
                }
            const float e = min_eig_response(sxx, sxy, syy);
            const bool free_px = !masked(discs, n_discs, hw, x, y);
            c->heig[(size_t)y * w + x] = e;
            c->hmask[(size_t)y * w + x] = free_px ? 255 : 0;
            if (free_px) max_bits = std::max(max_bits, ordered_bits(e));
        }
    c->max_val = from_ordered_bits(max_bits);
    const float t = quality_threshold(c->max_val, p.quality_level);
    std::vector<uint64_t> keys;
    for (int y = 1; y <= h - 2; ++y)
        for (int x = 1; x <= w - 2; ++x) {
            const size_t at = (size_t)y * w + x;
            const float v = c->heig[at];
            if (!(v > t) || v == 0.0f || c->hmask[at] == 0) continue;
            bool top = true;
            for (int j = -1; j <= 1 && top; ++j)
                for (int i = -1; i <= 1; ++i) {
                    const float nb = c->heig[at + (int64_t)j * w + i];
                    if ((nb > t ? nb : 0.0f) > v) { top = false; break; }
                }
            if (top) keys.push_back(corner_key(v, (uint32_t)at));
        }
    c->n_candidates = (int32_t)keys.size();
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    const int32_t gate = distance_gate(p.min_distance);
    std::vector<int32_t> acc;
    for (size_t k = 0; k < keys.size() && (int32_t)acc.size() < p.max_corners; ++k) {
        const int32_t q = pack_xy((uint32_t)keys[k], w);
        bool good = true;
        if (gate > 1)
            for (int32_t a : acc)
                if (too_close(q, a, gate)) { good = false; break; }
        if (good) acc.push_back(q);
    }
    for (size_t a = 0; a < acc.size(); ++a) { xy[2 * a] = (float)(acc[a] & 0xffff); xy[2 * a + 1] = (float)(acc[a] >> 16); }
    *n_out = (int32_t)acc.size();
}

int device_corners(visfs_flow* f, CornerState* c, const uint8_t* px, const visfs_corners_params& p, float* xy, int32_t* n_out) {
    HIP_TRY(f, hipSetDevice(f->dev));
    const int w = f->w, h = f->h;
    const size_t disc_bytes = c->discs.size() * sizeof(Disc), hw_bytes = c->hw.size() * sizeof(int32_t);
    const Disc* d_discs = nullptr;
    const int32_t* d_hw = nullptr;
    if (!c->discs.empty()) {
        const int rc = disc_reserve(f, disc_bytes + hw_bytes);
        if (rc != VISFS_BA_OK) return rc;
        // the pinned block is free: the call that filled it last ended in a synchronise behind its copy
        std::memcpy(c->disc.h.get(), c->discs.data(), disc_bytes);
        std::memcpy(c->disc.h.get() + disc_bytes, c->hw.data(), hw_bytes);
        HIP_TRY(f, hipMemcpyAsync(c->disc.d.get(), c->disc.h.get(), disc_bytes + hw_bytes, hipMemcpyHostToDevice, f->stream));
        d_discs = reinterpret_cast<const Disc*>(c->disc.d.get());
        d_hw = reinterpret_cast<const int32_t*>(c->disc.d.get() + disc_bytes);
    }
    CornerDev* st = reinterpret_cast<CornerDev*>(c->d_out.get());
    float* d_xy = reinterpret_cast<float*>(c->d_out.get() + sizeof(CornerDev));
    HIP_TRY(f, hipMemsetAsync(c->d_out.get(), 0, sizeof(CornerDev), f->stream));
    hipLaunchKernelGGL(k_corner_response, dim3((w + CT_X - 1) / CT_X, (h + CT_Y - 1) / CT_Y), dim3(CR_T), 0, f->stream, px, w, h, d_discs,
                       (int)c->discs.size(), d_hw, c->d_eig.get(), c->d_mask.get(), st);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_corner_candidates, dim3((unsigned)(((size_t)w * h + CR_T - 1) / CR_T)), dim3(CR_T), 0, f->stream, c->d_eig.get(), c->d_mask.get(),
                       w, h, p.quality_level, st, c->d_keys.get());
    HIP_TRY(f, hipGetLastError());
    const size_t chunks = (max_candidates(f) + 63) / 64;
    hipLaunchKernelGGL(k_corner_sort, dim3((unsigned)std::min<size_t>(std::max<size_t>(chunks, 1), kSortGrid)), dim3(CR_T), 0, f->stream,
                       c->d_keys.get(), st, c->d_sorted);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_corner_select, dim3(1), dim3(kSelT), 0, f->stream, c->d_sorted, st, w, distance_gate(p.min_distance), p.max_corners,
                       d_xy);
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipMemcpyAsync(c->h_out.get(), c->d_out.get(), sizeof(CornerDev) + sizeof(float) * 2 * (size_t)p.max_corners, hipMemcpyDeviceToHost,
                             f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    CornerDev out;
    std::memcpy(&out, c->h_out.get(), sizeof(out));
    if (out.n_out < 0 || out.n_out > p.max_corners) return fail(f, VISFS_BA_ERR_DEVICE, "the selection returned an impossible count");
    c->n_candidates = (int32_t)out.count;
    c->max_val = from_ordered_bits(out.max_bits);
    std::memcpy(xy, c->h_out.get() + sizeof(CornerDev), sizeof(float) * 2 * (size_t)out.n_out);
    *n_out = out.n_out;
    return VISFS_BA_OK;
}

}  // namespace

// ---------------------------------------------------------------- the resident caller's entry points (ba_tracker.hip)
namespace flow {

int group_corners_prepare(visfs_flow* f) { return ensure_state(f); }

void group_corners_fill(visfs_flow* f, const uint8_t* px, const Disc* d_discs, const int32_t* d_hw, const int32_t* d_args, bool skip,
                        CornerRec* r, const int32_t** d_n_out, const float** d_xy) {
    CornerState* c = f->corners;
    if (!skip) c->valid = false;               // the download hook reports staged calls only
    CornerDev* st = reinterpret_cast<CornerDev*>(c->d_out.get());
    r->px = px; r->discs = d_discs; r->hw = d_hw; r->args = d_args;
    r->eig = c->d_eig.get(); r->mask = c->d_mask.get(); r->keys = c->d_keys.get(); r->sorted = c->d_sorted;
    r->st = st; r->xy = reinterpret_cast<float*>(c->d_out.get() + sizeof(CornerDev));
    r->skip = skip ? 1 : 0; r->pad = 0;
    *d_n_out = &st->n_out;
    *d_xy = r->xy;
}

int group_corners(visfs_flow* f, double quality_level, double min_distance, int n, const CornerRec* d_recs, GroupCounts* cnt) {
    const int w = f->w, h = f->h;
    const unsigned z = (unsigned)n;
    hipLaunchKernelGGL(k_corner_reset_g, dim3((z + 63) / 64), dim3(64), 0, f->stream, d_recs, n);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_corner_response_g, dim3((w + CT_X - 1) / CT_X, (h + CT_Y - 1) / CT_Y, z), dim3(CR_T), 0, f->stream, d_recs, w, h);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_corner_candidates_g, dim3((unsigned)(((size_t)w * h + CR_T - 1) / CR_T), 1, z), dim3(CR_T), 0, f->stream, d_recs, w, h,
                       quality_level);
    HIP_TRY(f, hipGetLastError());
    const size_t chunks = (max_candidates(f) + 63) / 64;
    hipLaunchKernelGGL(k_corner_sort_g, dim3((unsigned)std::min<size_t>(std::max<size_t>(chunks, 1), kSortGrid), 1, z), dim3(CR_T), 0, f->stream,
                       d_recs);
    HIP_TRY(f, hipGetLastError());
    hipLaunchKernelGGL(k_corner_select_g, dim3(1, 1, z), dim3(kSelT), 0, f->stream, d_recs, w, distance_gate(min_distance));
    HIP_TRY(f, hipGetLastError());
    cnt->launches += 5;
    return VISFS_BA_OK;
}

int corners_host(visfs_flow* f, const uint8_t* px, int32_t max_corners, double quality_level, double min_distance, const Disc* discs,
                 int n_discs, const int32_t* hw, float* xy, int32_t* n_out) {
    *n_out = 0;
    if (max_corners <= 0) return VISFS_BA_OK;
    const int rc = ensure_state(f);
    if (rc != VISFS_BA_OK) return rc;
    f->corners->valid = false;
    visfs_corners_params p;
    p.max_corners = max_corners; p.quality_level = quality_level; p.min_distance = min_distance;
    host_corners(f, f->corners, px, p, discs, n_discs, hw, xy, n_out);
    return VISFS_BA_OK;
}

}  // namespace flow

// ====================================================================== exported C ABI
extern "C" {

int visfs_corners_abi_version(void) { return VISFS_CORNERS_ABI_VERSION; }

void visfs_corners_default_params(visfs_corners_params* p) {
    if (!p) return;
    p->max_corners = 300; p->quality_level = 0.01; p->min_distance = 40.0;
}

int visfs_flow_corners(visfs_flow* f, int32_t slot, int32_t image, const visfs_corners_params* p, int32_t n_discs,
                       const visfs_corners_disc* discs, int32_t capacity, float* xy, int32_t* n_out) {
    if (!f || !p || !xy || !n_out || n_discs < 0 || (n_discs > 0 && !discs)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        *n_out = 0;
        int rc = check_call(f, slot, image, p, n_discs, discs, capacity);
        if (rc != VISFS_BA_OK) return rc;
        rc = ensure_state(f);
        if (rc != VISFS_BA_OK) return rc;
        CornerState* c = f->corners;
        c->valid = false;
        c->n_discs = n_discs;
        decide_discs(f, c, n_discs, discs);
        const int s = slot == VISFS_FLOW_SLOT_CURRENT ? f->cur : 1 - f->cur;
        if (f->device) {
            rc = device_corners(f, c, f->dpx[s][image], *p, xy, n_out);
            if (rc != VISFS_BA_OK) return rc;
        } else {
            host_corners(f, c, f->hpx[s][image].data(), *p, c->discs.data(), (int)c->discs.size(), c->hw.data(), xy, n_out);
        }
        c->valid = true;
        return (int)VISFS_BA_OK;
    });
}

int visfs_flow_corners_download(const visfs_flow* cf, float* eig, uint8_t* mask, uint8_t* disc_drawn, int32_t* n_candidates, float* max_val) {
    visfs_flow* f = const_cast<visfs_flow*>(cf);
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        const CornerState* c = f->corners;
        if (!c || !c->valid) return fail(f, VISFS_BA_ERR_NOT_LOADED, "no corner call to report on");
        const size_t n0 = (size_t)f->w * f->h;
        if (disc_drawn && c->n_discs > 0) std::memcpy(disc_drawn, c->drawn.data(), (size_t)c->n_discs);
        if (n_candidates) *n_candidates = c->n_candidates;
        if (max_val) *max_val = c->max_val;
        if (!f->device) {
            if (eig) std::memcpy(eig, c->heig.data(), n0 * sizeof(float));
            if (mask) std::memcpy(mask, c->hmask.data(), n0);
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(f, hipSetDevice(f->dev));
        if (eig) HIP_TRY(f, hipMemcpyAsync(eig, c->d_eig.get(), n0 * sizeof(float), hipMemcpyDeviceToHost, f->stream));
        if (mask) HIP_TRY(f, hipMemcpyAsync(mask, c->d_mask.get(), n0, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_flow_corners_last_discs(const visfs_flow* f, int32_t* n_discs) {
    if (!f || !n_discs) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->corners || !f->corners->valid) return VISFS_BA_ERR_NOT_LOADED;
    *n_discs = f->corners->n_discs;
    return VISFS_BA_OK;
}

int visfs_corners_hook_halfwidth(int32_t radius, int32_t* hw) {
    if (radius < 0 || !hw) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (radius > kMaxRadius) return VISFS_BA_ERR_UNSUPPORTED;
    disc_halfwidth(radius, hw);
    return VISFS_BA_OK;
}

}  // extern "C"
