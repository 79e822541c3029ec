// The equalised frame push of a visfs_flow object (include/visfs_clahe.h).
//
// cv::CLAHE::apply on both images of a frame, as the reference runs it in front of the tracker (System.cpp:107-111), two ways over
// the arithmetic of ba_clahe.hpp:
//   * host restatement (objects of visfs_flow_create_host): every tile and every pixel in sequence on one core;
//   * device, two launches on the stream of the owning handle between the copies of the raw images and the pyramid launches:
//       k_clahe_lut    one workgroup per tile and image: the tile's histogram through LDS integer atomics into one sub-histogram per
//                      wavefront, merged; then thread i owns bin i: clip, workgroup sum of the excess, redistribution in closed form,
//                      inclusive scan over the 256 bins (wavefront scan, one LDS hand-off across the four wavefronts), one multiply,
//                      one rounding.  Stores the table byte and the final histogram word.
//       k_clahe_apply  four adjacent pixels per thread: one 4-byte load of the raw image, four table gathers and the blend per pixel,
//                      one 4-byte store into level 0 of the new slot.
// All sums are integers, so device and host agree to the byte whatever the order of summation.
#include "ba_clahe.hpp"
#include "ba_flow_object.hpp"
#include "ba_group.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_clahe.h"

#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace clahe;
using namespace host;

// ---------------------------------------------------------------- kernels
namespace clahe {

constexpr int CL_T = 256;          // one thread per bin
constexpr int CL_WAVES = CL_T / 64;
constexpr int CL_UNROLL = 8;       // pixels a thread of k_clahe_lut loads before it counts them
constexpr int CL_PX = 4;           // pixels per thread of k_clahe_apply

struct LutArgs {
    const uint8_t* raw[2];
    uint8_t* lut[2];               // [tiles_y][tiles_x][256]
    int32_t* hist[2];              // [tiles_y][tiles_x][256]
};

__device__ __forceinline__ void clahe_lut_body(const uint8_t* __restrict__ src, uint8_t* lut, int32_t* hist, const Geom& g) {
    __shared__ int32_t sHist[CL_WAVES][kBins];
    __shared__ int32_t sPart[CL_WAVES];
    __shared__ int32_t sScan[CL_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tile = blockIdx.x, ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
#pragma unroll
    for (int k = 0; k < CL_WAVES; ++k) sHist[k][tid] = 0;
    __syncthreads();
    const int area = g.tile_w * g.tile_h;
    const int x0 = tx * g.tile_w, y0 = ty * g.tile_h;
    // thread t takes pixels t, t + 256, ... of the tile in row-major order; its (row, column) advances without a division, and
    // CL_UNROLL independent loads are in flight before the first atomic needs its value
    const int dq = CL_T / g.tile_w, dr = CL_T - dq * g.tile_w;
    int r = tid / g.tile_w, c = tid - r * g.tile_w;
    for (int i = tid; i < area; i += CL_T * CL_UNROLL) {
        int v[CL_UNROLL];
#pragma unroll
        for (int k = 0; k < CL_UNROLL; ++k) {
            v[k] = -1;
            if (i + k * CL_T < area) {
                const int sx = ext_index(x0 + c, g.w), sy = ext_index(y0 + r, g.h);      // inside the image: one reflection at the most
                v[k] = src[(int64_t)sy * g.w + sx];
            }
            c += dr; r += dq;
            if (c >= g.tile_w) { c -= g.tile_w; ++r; }
        }
#pragma unroll
        for (int k = 0; k < CL_UNROLL; ++k)
            if (v[k] >= 0) atomicAdd(&sHist[wave][v[k]], 1);
    }
    __syncthreads();
    int32_t count = 0;
#pragma unroll
    for (int k = 0; k < CL_WAVES; ++k) count += sHist[k][tid];
    if (g.clip > 0) {                                                            // (uniform)
        int32_t excess = count > g.clip ? count - g.clip : 0;
        count -= excess;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) excess += __shfl_xor(excess, o, 64);
        if (lane == 0) sPart[wave] = excess;
        __syncthreads();
        int32_t clipped = 0;
#pragma unroll
        for (int k = 0; k < CL_WAVES; ++k) clipped += sPart[k];
        count = redistribute(count, tid, clipped);
    }
    int32_t cum = count;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(cum, o, 64);
        if (lane >= o) cum += up;
    }
    if (lane == 63) sScan[wave] = cum;
    __syncthreads();
    for (int k = 0; k < wave; ++k) cum += sScan[k];
    const int64_t o = (int64_t)tile * kBins + tid;
    lut[o] = lut_value(cum, g.lut_scale);
    hist[o] = count;
}

__global__ __launch_bounds__(CL_T) void k_clahe_lut(LutArgs A, Geom g) {
    clahe_lut_body(A.raw[blockIdx.y], A.lut[blockIdx.y], A.hist[blockIdx.y], g);
}

// the batched forms (tracker groups): member blockIdx.z, its buffers read from the group's table
__global__ __launch_bounds__(CL_T) void k_clahe_lut_g(const flow::ClaheRec* __restrict__ recs, Geom g) {
    const flow::ClaheRec& r = recs[blockIdx.z];
    clahe_lut_body(r.raw[blockIdx.y], r.lut[blockIdx.y], r.hist[blockIdx.y], g);
}

struct ApplyArgs {
    const uint8_t* raw[2];
    const uint8_t* lut[2];
    uint8_t* dst[2];               // level 0 of the new slot; like raw, the base is 4-byte aligned
};

__device__ __forceinline__ void clahe_apply_body(const uint8_t* __restrict__ src, const uint8_t* __restrict__ lut, uint8_t* __restrict__ dst,
                                                 const Geom& g) {
    const int64_t n0 = (int64_t)g.w * g.h;
    const int64_t i0 = ((int64_t)blockIdx.x * CL_T + threadIdx.x) * CL_PX;
    if (i0 >= n0) return;
    int y = (int)(i0 / g.w), x = (int)(i0 - (int64_t)y * g.w);
    const bool whole = i0 + CL_PX <= n0;
    uint8_t v[CL_PX] = { 0, 0, 0, 0 }, out[CL_PX];
    if (whole) {
        const uint32_t p = *reinterpret_cast<const uint32_t*>(src + i0);
#pragma unroll
        for (int k = 0; k < CL_PX; ++k) v[k] = (uint8_t)(p >> (8 * k));
    } else {
        for (int k = 0; i0 + k < n0; ++k) v[k] = src[i0 + k];
    }
    Axis Y = axis_of(y, g.inv_th, g.tiles_y);
#pragma unroll
    for (int k = 0; k < CL_PX; ++k) {
        out[k] = blend(lut, g.tiles_x, axis_of(x, g.inv_tw, g.tiles_x), Y, v[k]);      // (past the end: a value nobody stores)
        if (++x == g.w) { x = 0; ++y; Y = axis_of(y < g.h ? y : g.h - 1, g.inv_th, g.tiles_y); }
    }
    if (whole) {
        *reinterpret_cast<uint32_t*>(dst + i0) = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
    } else {
        for (int k = 0; i0 + k < n0; ++k) dst[i0 + k] = out[k];
    }
}

__global__ __launch_bounds__(CL_T) void k_clahe_apply(ApplyArgs A, Geom g) {
    clahe_apply_body(A.raw[blockIdx.y], A.lut[blockIdx.y], A.dst[blockIdx.y], g);
}

__global__ __launch_bounds__(CL_T) void k_clahe_apply_g(const flow::ClaheRec* __restrict__ recs, Geom g) {
    const flow::ClaheRec& r = recs[blockIdx.z];
    clahe_apply_body(r.raw[blockIdx.y], r.lut[blockIdx.y], r.dst[blockIdx.y], g);
}

}  // namespace clahe

// ---------------------------------------------------------------- per-object state
namespace flow {

struct ClaheState {
    bool valid = false;            // a push has completed
    Geom g{};                      // of the last push

    // host restatement: [image]
    std::vector<uint8_t> hlut[2];
    std::vector<int32_t> hhist[2];

    // device: sized for kMaxTiles x kMaxTiles at the first call
    DeviceBuf<uint8_t> d_raw;      // both raw images of a frame
    DeviceBuf<uint8_t> d_lut;      // both images' tables
    DeviceBuf<int32_t> d_hist;     // both images' final histograms
    size_t raw_stride = 0;         // bytes from the left image to the right one
};

void clahe_release(visfs_flow* f) {
    ClaheState* c = f->clahe;
    if (!c) return;
    if (f->device) {
        (void)hipSetDevice(f->dev);
        if (f->stream) (void)hipStreamSynchronize(f->stream);
    }
    delete c;
    f->clahe = nullptr;
}

}  // namespace flow

namespace {

using flow::ClaheState;

constexpr size_t kTableCells = (size_t)kMaxTiles * kMaxTiles * kBins;      // of one image

int check_params(const visfs_clahe_params* p, int32_t w, int32_t h, const char** why) {
    if (!std::isfinite(p->clip_limit) || p->clip_limit < 0.0) { *why = "clip_limit must be finite and not negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p->tiles_x < 1 || p->tiles_y < 1) { *why = "a tile count is below 1"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (w < 1 || h < 1) { *why = "image size must be positive"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p->tiles_x > kMaxTiles || p->tiles_y > kMaxTiles) { *why = "a tile count is above 32"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (w <= p->tiles_x || h <= p->tiles_y) { *why = "the image is not larger than the tile count"; return VISFS_BA_ERR_UNSUPPORTED; }
    return VISFS_BA_OK;
}

// the first call of an object allocates; a call that fails here leaves the object without this state
int ensure_state(visfs_flow* f) {
    if (f->clahe) return VISFS_BA_OK;
    ClaheState* c = new ClaheState();
    f->clahe = c;
    if (!f->device) return VISFS_BA_OK;
    const size_t n0 = (size_t)f->w * f->h;
    c->raw_stride = (n0 + 255) & ~size_t(255);
    const auto alloc = [&]() -> int {
        HIP_TRY(f, hipSetDevice(f->dev));
        RC_TRY(c->d_raw.alloc(f, 2 * c->raw_stride));
        RC_TRY(c->d_lut.alloc(f, 2 * kTableCells));
        RC_TRY(c->d_hist.alloc(f, 2 * kTableCells));
        return VISFS_BA_OK;
    };
    const int rc = alloc();
    if (rc != VISFS_BA_OK) flow::clahe_release(f);
    return rc;
}

void host_equalise(const Geom& g, const uint8_t* img, int32_t stride, uint8_t* lut, int32_t* hist, uint8_t* dst) {
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            int32_t* hs = hist + ((size_t)ty * g.tiles_x + tx) * kBins;
            uint8_t* lt = lut + ((size_t)ty * g.tiles_x + tx) * kBins;
            for (int i = 0; i < kBins; ++i) hs[i] = 0;
            for (int r = 0; r < g.tile_h; ++r) {
                const uint8_t* row = img + (size_t)ext_index(ty * g.tile_h + r, g.h) * stride;
                for (int c = 0; c < g.tile_w; ++c) ++hs[row[ext_index(tx * g.tile_w + c, g.w)]];
            }
            if (g.clip > 0) {
                int32_t clipped = 0;
                for (int i = 0; i < kBins; ++i)
                    if (hs[i] > g.clip) { clipped += hs[i] - g.clip; hs[i] = g.clip; }
                for (int i = 0; i < kBins; ++i) hs[i] = redistribute(hs[i], i, clipped);
            }
            int32_t cum = 0;
            for (int i = 0; i < kBins; ++i) { cum += hs[i]; lt[i] = lut_value(cum, g.lut_scale); }
        }
    for (int y = 0; y < g.h; ++y) {
        const Axis Y = axis_of(y, g.inv_th, g.tiles_y);
        for (int x = 0; x < g.w; ++x)
            dst[(size_t)y * g.w + x] = blend(lut, g.tiles_x, axis_of(x, g.inv_tw, g.tiles_x), Y, img[(size_t)y * stride + x]);
    }
}

int device_equalise(visfs_flow* f, ClaheState* c, const Geom& g, int slot, const uint8_t* left, const uint8_t* right, int32_t stride) {
    uint8_t* const raw[2] = { c->d_raw.get(), c->d_raw.get() + c->raw_stride };
    const int rc = flow::device_stage(f, raw, left, right, stride);
    if (rc != VISFS_BA_OK) return rc;
    const size_t tile_cells = (size_t)g.tiles_x * g.tiles_y * kBins;
    LutArgs L;
    ApplyArgs P;
    for (int i = 0; i < 2; ++i) {
        L.raw[i] = P.raw[i] = raw[i];
        L.lut[i] = c->d_lut.get() + i * tile_cells; P.lut[i] = L.lut[i];
        L.hist[i] = c->d_hist.get() + i * tile_cells;
        P.dst[i] = f->dpx[slot][i];
    }
    hipLaunchKernelGGL(k_clahe_lut, dim3((unsigned)(g.tiles_x * g.tiles_y), 2), dim3(CL_T), 0, f->stream, L, g);
    HIP_TRY(f, hipGetLastError());
    const int64_t per_block = (int64_t)CL_T * CL_PX;
    const unsigned blocks = (unsigned)(((int64_t)g.w * g.h + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_clahe_apply, dim3(blocks, 2), dim3(CL_T), 0, f->stream, P, g);
    HIP_TRY(f, hipGetLastError());
    return flow::device_pyramids(f, slot);
}

}  // namespace

// ---------------------------------------------------------------- the tracker group's entry points (ba_tracker.hip)
namespace flow {

int group_clahe_prepare(visfs_flow* f) { return ensure_state(f); }

void group_clahe_fill(visfs_flow* f, const Geom& g, int slot, ClaheRec* r, uint8_t* raw[2]) {
    ClaheState* c = f->clahe;
    const size_t tile_cells = (size_t)g.tiles_x * g.tiles_y * kBins;
    for (int i = 0; i < 2; ++i) {
        raw[i] = c->d_raw.get() + i * c->raw_stride;
        r->raw[i] = raw[i];
        r->lut[i] = c->d_lut.get() + i * tile_cells;
        r->hist[i] = c->d_hist.get() + i * tile_cells;
        r->dst[i] = f->dpx[slot][i];
    }
    c->valid = false;
}

int group_clahe(visfs_flow* f, const Geom& g, int n, const ClaheRec* d_recs, GroupCounts* cnt) {
    hipLaunchKernelGGL(k_clahe_lut_g, dim3((unsigned)(g.tiles_x * g.tiles_y), 2, (unsigned)n), dim3(CL_T), 0, f->stream, d_recs, g);
    HIP_TRY(f, hipGetLastError());
    const int64_t per_block = (int64_t)CL_T * CL_PX;
    const unsigned blocks = (unsigned)(((int64_t)g.w * g.h + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_clahe_apply_g, dim3(blocks, 2, (unsigned)n), dim3(CL_T), 0, f->stream, d_recs, g);
    HIP_TRY(f, hipGetLastError());
    cnt->launches += 2;
    return VISFS_BA_OK;
}

void group_clahe_pushed(visfs_flow* f, const Geom& g) { f->clahe->g = g; f->clahe->valid = true; }

}  // namespace flow

// ====================================================================== exported C ABI
extern "C" {

int visfs_clahe_abi_version(void) { return VISFS_CLAHE_ABI_VERSION; }

void visfs_clahe_default_params(visfs_clahe_params* p) {
    if (!p) return;
    p->clip_limit = 3.0; p->tiles_x = 8; p->tiles_y = 8;
}

int visfs_flow_push_frame_clahe(visfs_flow* f, const visfs_clahe_params* p, const uint8_t* left, const uint8_t* right, int32_t stride) {
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (!p || !left || !right) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "a NULL argument");
        const char* why = "";
        int rc = check_params(p, f->w, f->h, &why);
        if (rc != VISFS_BA_OK) return fail(f, rc, why);
        if (stride < f->w) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "stride is smaller than the image width");
        rc = ensure_state(f);
        if (rc != VISFS_BA_OK) return rc;
        ClaheState* c = f->clahe;
        const Geom g = make_geom(f->w, f->h, p->tiles_x, p->tiles_y, p->clip_limit);
        const int slot = f->frames == 0 ? f->cur : 1 - f->cur;
        c->valid = false;
        if (f->device) {
            rc = device_equalise(f, c, g, slot, left, right, stride);
            if (rc != VISFS_BA_OK) return rc;
        } else {
            const size_t tile_cells = (size_t)g.tiles_x * g.tiles_y * kBins;
            const uint8_t* src[2] = { left, right };
            for (int i = 0; i < 2; ++i) {
                c->hlut[i].resize(tile_cells); c->hhist[i].resize(tile_cells);
                f->hpx[slot][i].resize((size_t)f->lay.cells);
                host_equalise(g, src[i], stride, c->hlut[i].data(), c->hhist[i].data(), f->hpx[slot][i].data());
                flow::host_pyramids(f, slot, i);
            }
        }
        c->g = g; c->valid = true;
        f->cur = slot;
        ++f->frames;
        return (int)VISFS_BA_OK;
    });
}

// ---- test hooks
int visfs_clahe_hook_geometry(const visfs_clahe_params* p, int32_t w, int32_t h, int32_t* ext_w, int32_t* ext_h, int32_t* tile_w,
                              int32_t* tile_h, int32_t* clip) {
    if (!p) return VISFS_BA_ERR_BAD_ARGUMENT;
    const char* why = "";
    const int rc = check_params(p, w, h, &why);
    if (rc != VISFS_BA_OK) return rc;
    const Geom g = make_geom(w, h, p->tiles_x, p->tiles_y, p->clip_limit);
    if (ext_w) *ext_w = g.ext_w;
    if (ext_h) *ext_h = g.ext_h;
    if (tile_w) *tile_w = g.tile_w;
    if (tile_h) *tile_h = g.tile_h;
    if (clip) *clip = g.clip;
    return VISFS_BA_OK;
}

int visfs_flow_clahe_last_tiles(const visfs_flow* f, int32_t* tiles_x, int32_t* tiles_y) {
    if (!f || !tiles_x || !tiles_y) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->clahe || !f->clahe->valid) return VISFS_BA_ERR_NOT_LOADED;
    *tiles_x = f->clahe->g.tiles_x; *tiles_y = f->clahe->g.tiles_y;
    return VISFS_BA_OK;
}

int visfs_flow_clahe_download(const visfs_flow* cf, int32_t image, uint8_t* lut, int32_t* hist) {
    visfs_flow* f = const_cast<visfs_flow*>(cf);
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (image < 0 || image > 1) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "image out of range");
        const ClaheState* c = f->clahe;
        if (!c || !c->valid) return fail(f, VISFS_BA_ERR_NOT_LOADED, "no equalised push to report on");
        const size_t tile_cells = (size_t)c->g.tiles_x * c->g.tiles_y * kBins;
        if (!f->device) {
            if (lut) std::memcpy(lut, c->hlut[image].data(), tile_cells);
            if (hist) std::memcpy(hist, c->hhist[image].data(), tile_cells * sizeof(int32_t));
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(f, hipSetDevice(f->dev));
        if (lut) HIP_TRY(f, hipMemcpyAsync(lut, c->d_lut.get() + image * tile_cells, tile_cells, hipMemcpyDeviceToHost, f->stream));
        if (hist) HIP_TRY(f, hipMemcpyAsync(hist, c->d_hist.get() + image * tile_cells, tile_cells * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

}  // extern "C"
