// Pyramidal Lucas-Kanade tracking with stereo triangulation on the GPU (include/visfs_flow.h).
//
// The pixel half of the reference's Tracker::imageProcess (Tracker.cpp:233-274, :343-388), two ways over the work items of ba_flow.hpp:
//   * host restatement (visfs_flow_create_host): every cell and every point in sequence on one core;
//   * device: the pyramids of the previous and the current stereo pair resident in HBM,
//       k_flow_pyr_down   one level from the one below, both images of the frame in one launch (grid.y)
//       k_flow_scharr     the (Ix, Iy) pairs of every level of both images, one launch per frame
//       k_flow_lk<BACK, TRI>  one wavefront per point: all levels and iterations of the forward pass, fused behind it the reverse
//                         pass with its gate and (TRI) the triangulation.  The 441 template values live in registers, 7 cells per
//                         lane; an iteration gathers the moving window's four neighbours per cell, multiplies in int32 and adds
//                         across the wavefront in int64; every lane then runs the scalar tail on the same sums.
// The sums are exact integers, so device and host agree to the byte whatever the order of summation.
#include "ba_flow_object.hpp"
#include "ba_group.hpp"
#include "ba_host.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace flow;
using namespace host;

// ---------------------------------------------------------------- kernels
namespace flow {

constexpr int FL_T = 256;

struct PyrDownArgs {
    const uint8_t* src[2];
    uint8_t* dst[2];
    int32_t sw, sh, dw, dh;
};

__device__ __forceinline__ void pyr_down_body(const uint8_t* src, uint8_t* dst, int32_t sw, int32_t sh, int32_t dw, int32_t dh) {
    const int64_t i = (int64_t)blockIdx.x * FL_T + threadIdx.x;
    if (i >= (int64_t)dw * dh) return;
    const int y = (int)(i / dw), x = (int)(i - (int64_t)y * dw);
    dst[i] = pyr_down_cell(src, sw, sh, x, y);
}

__global__ __launch_bounds__(FL_T) void k_flow_pyr_down(PyrDownArgs A) {
    pyr_down_body(A.src[blockIdx.y], A.dst[blockIdx.y], A.sw, A.sh, A.dw, A.dh);
}

// the batched forms (tracker groups): member blockIdx.z, its images read from the group's table
__global__ __launch_bounds__(FL_T) void k_flow_pyr_down_g(const PyrRec* __restrict__ recs, int64_t soff, int64_t doff, int32_t sw, int32_t sh,
                                                          int32_t dw, int32_t dh) {
    uint8_t* px = recs[blockIdx.z].px[blockIdx.y];
    pyr_down_body(px + soff, px + doff, sw, sh, dw, dh);
}

struct ScharrArgs {
    const uint8_t* px[2];
    uint32_t* der[2];
};

__device__ __forceinline__ void scharr_body(const uint8_t* px, uint32_t* der, const Layout& lay) {
    const int64_t i = (int64_t)blockIdx.x * FL_T + threadIdx.x;
    if (i >= lay.cells) return;
    int l = 0;
    while (l + 1 < lay.n_levels && i >= lay.L[l + 1].off) ++l;
    const Level L = lay.L[l];
    const int64_t c = i - L.off;
    const int y = (int)(c / L.w), x = (int)(c - (int64_t)y * L.w);
    der[i] = scharr_cell(px + L.off, L.w, L.h, x, y);
}

__global__ __launch_bounds__(FL_T) void k_flow_scharr(ScharrArgs A, Layout lay) { scharr_body(A.px[blockIdx.y], A.der[blockIdx.y], lay); }

__global__ __launch_bounds__(FL_T) void k_flow_scharr_g(const PyrRec* __restrict__ recs, Layout lay) {
    const PyrRec& r = recs[blockIdx.z];
    scharr_body(r.px[blockIdx.y], r.der[blockIdx.y], lay);
}

// the window cells of one wavefront: cell s * 64 + lane in slot s, per-lane int32 partial sums, int64 butterfly
//
// Why int32 holds a lane's partial sum: the unnormalised Scharr of 8-bit pixels is at most (3 + 10 + 3) * 255 = 4080 in size, and
// the bilinear weights sum to 2^14, so |gx|, |gy| <= 4080 after the descale (4081 with its rounding); a pixel sample keeps 5
// fractional bits, 0 .. 8160, so |diff| <= 8160.  A lane adds kLaneSlots = 7 products: at most 7 * 4081^2 = 1.17e8 for the normal
// matrix and 7 * 8160 * 4081 = 2.33e8 for the right-hand side, against 2^31 = 2.15e9.  The 0 / 255 images of
// tests/flow_cases.py (saturated_*) run this on the device.
struct WaveCells {
    static constexpr int kSlots = kLaneSlots;
    using acc_t = int32_t;
    int lane;
    __device__ int cell(int s) const { return s * 64 + lane; }
    __device__ int64_t total(acc_t v) const {
        long long x = v;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
        return x;
    }
};

struct LkArgs {
    Image I, J;
    const float* pts;          // [n][2]
    const float* init;         // [n][2] or nullptr
    float* to;                 // [n][2]
    uint8_t* status;           // [n]
    float* err;                // [n]
    float* xyz;                // [n][3] (TRI)
    int32_t n;
    float gate;
};

template <bool BACK, bool TRI>
__global__ __launch_bounds__(64) void k_flow_lk(LkArgs A, LkParams prm, Layout lay, Camera cam) {
    const int p = blockIdx.x;
    if (p >= A.n) return;
    WaveCells pol{ (int)threadIdx.x };
    const float ptx = A.pts[2 * p], pty = A.pts[2 * p + 1];
    const bool has_init = A.init != nullptr;
    const float inx = has_init ? A.init[2 * p] : 0.0f, iny = has_init ? A.init[2 * p + 1] : 0.0f;
    float tox, toy, err;
    uint8_t st;
    lk_gated(pol, prm, lay, A.I, A.J, ptx, pty, has_init, inx, iny, BACK, A.gate, tox, toy, st, err);
    if (threadIdx.x != 0) return;
    A.to[2 * p] = tox; A.to[2 * p + 1] = toy;
    A.status[p] = st;
    A.err[p] = err;
    if (TRI) {
        float xyz[3] = { __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("") };
        if (st) triangulate(cam, ptx, pty, tox, xyz);
        A.xyz[3 * p] = xyz[0]; A.xyz[3 * p + 1] = xyz[1]; A.xyz[3 * p + 2] = xyz[2];
    }
}

}  // namespace flow

namespace {

constexpr int32_t kInitialPoints = 1024;

int check_params(const visfs_flow_params* p, int32_t w, int32_t h, std::string& why) {
    if (p->win_size < 3 || p->win_size > kMaxWin) { why = "win_size must lie in 3 .. 21"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (p->max_level < 0 || p->max_level >= kMaxLevels) { why = "max_level must lie in 0 .. 7"; return VISFS_BA_ERR_UNSUPPORTED; }
    if (p->iterations < 0) { why = "iterations must not be negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (!(p->eps >= 0.0f) || !std::isfinite(p->eps) || !std::isfinite(p->min_eig_threshold) || !(p->back_gate_track >= 0.0f) ||
        !(p->back_gate_stereo >= 0.0f) || !std::isfinite(p->min_depth) || !std::isfinite(p->max_depth)) {
        why = "a threshold is not finite or is negative"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    if (w < 1 || h < 1 || w > 16384 || h > 16384) { why = "image size must lie in 1 .. 16384"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    // one reflection reaches every read of a window that starts in [-win, cols): the top level must be wider than win + 2
    int32_t tw = w, th = h;
    for (int l = 0; l < p->max_level; ++l) { tw = (tw + 1) / 2; th = (th + 1) / 2; }
    if (tw < p->win_size + 2 || th < p->win_size + 2) { why = "the top pyramid level is smaller than the window"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    return VISFS_BA_OK;
}

void init_common(visfs_flow* f, const visfs_flow_params* p, int32_t w, int32_t h) {
    f->prm = *p; f->w = w; f->h = h;
    f->lk.win = p->win_size; f->lk.max_level = p->max_level; f->lk.iterations = p->iterations;
    f->lk.eps2 = p->eps * p->eps; f->lk.min_eig = p->min_eig_threshold;
    int64_t off = 0;
    int32_t lw = w, lh = h;
    f->lay.n_levels = p->max_level + 1;
    for (int l = 0; l <= p->max_level; ++l) {
        f->lay.L[l].w = lw; f->lay.L[l].h = lh; f->lay.L[l].off = off;
        off += (int64_t)lw * lh;
        lw = (lw + 1) / 2; lh = (lh + 1) / 2;
    }
    f->lay.cells = off;
}

Camera make_camera(const visfs_flow_params& p, const visfs_flow_camera& c) {
    Camera k;
    k.fx = c.fx; k.fy = c.fy; k.cx = c.cx; k.cy = c.cy; k.cx_right = c.cx_right; k.baseline = c.baseline;
    k.min_depth = p.min_depth; k.max_depth = p.max_depth;
    for (int i = 0; i < 12; ++i) k.T[i] = c.Tir[i];
    return k;
}

// a call's buffer: [pts 8n][init 8n] in, [to 8n][err 4n][xyz 12n][status n] out
struct IoLayout { size_t pts, init, in_bytes, to, err, xyz, status, bytes; };
IoLayout io_layout(size_t n) {
    IoLayout o;
    o.pts = 0; o.init = 8 * n; o.in_bytes = 16 * n;
    o.to = up256(o.in_bytes); o.err = o.to + 8 * n; o.xyz = o.err + 4 * n; o.status = o.xyz + 12 * n; o.bytes = up256(o.status + n);
    return o;
}

int io_reserve(visfs_flow* f, int32_t n) {
    if (n <= f->io_cap) return VISFS_BA_OK;
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    f->io_cap = 0;
    const int32_t cap = std::max(n, kInitialPoints);
    const size_t bytes = io_layout((size_t)cap).bytes;                     // grows with the points, so the block's bytes are short as well
    RC_TRY(f->io.reserve(f, bytes, bytes));
    f->io_cap = cap;
    return VISFS_BA_OK;
}

int device_init(visfs_flow* f) {
    HIP_TRY(f, hipSetDevice(f->dev));
    const size_t bpx = up256((size_t)f->lay.cells), bder = up256((size_t)f->lay.cells * 4);
    RC_TRY(f->d_mem.alloc(f, 4 * (bpx + bder)));
    char* m = f->d_mem.get();
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < 2; ++i) {
            f->dder[s][i] = reinterpret_cast<uint32_t*>(m); m += bder;
            f->dpx[s][i] = reinterpret_cast<uint8_t*>(m); m += bpx;
        }
    RC_TRY(f->h_img.alloc(f, 2 * (size_t)f->w * f->h));
    return io_reserve(f, kInitialPoints);
}

}  // namespace

namespace flow {

void host_pyramids(visfs_flow* f, int slot, int image) {
    std::vector<uint8_t>& px = f->hpx[slot][image];
    std::vector<uint32_t>& der = f->hder[slot][image];
    px.resize((size_t)f->lay.cells); der.resize((size_t)f->lay.cells);
    for (int l = 1; l < f->lay.n_levels; ++l) {
        const Level &S = f->lay.L[l - 1], &D = f->lay.L[l];
        for (int32_t y = 0; y < D.h; ++y)
            for (int32_t x = 0; x < D.w; ++x) px[(size_t)D.off + (size_t)y * D.w + x] = pyr_down_cell(px.data() + S.off, S.w, S.h, x, y);
    }
    for (int l = 0; l < f->lay.n_levels; ++l) {
        const Level& L = f->lay.L[l];
        for (int32_t y = 0; y < L.h; ++y)
            for (int32_t x = 0; x < L.w; ++x) der[(size_t)L.off + (size_t)y * L.w + x] = scharr_cell(px.data() + L.off, L.w, L.h, x, y);
    }
}

int group_stage(visfs_flow* f, uint8_t* const dst[2], const uint8_t* left, const uint8_t* right, int32_t stride, GroupCounts* cnt) {
    const size_t n0 = (size_t)f->w * f->h;
    const uint8_t* src[2] = { left, right };
    for (int i = 0; i < 2; ++i) {
        for (int32_t y = 0; y < f->h; ++y) std::memcpy(f->h_img.get() + i * n0 + (size_t)y * f->w, src[i] + (size_t)y * stride, (size_t)f->w);
        HIP_TRY(f, hipMemcpyAsync(dst[i], f->h_img.get() + i * n0, n0, hipMemcpyHostToDevice, f->stream));
        if (cnt) ++cnt->copies;
    }
    return VISFS_BA_OK;
}

int device_stage(visfs_flow* f, uint8_t* const dst[2], const uint8_t* left, const uint8_t* right, int32_t stride) {
    HIP_TRY(f, hipSetDevice(f->dev));
    HIP_TRY(f, hipStreamSynchronize(f->stream));                        // the staging image of the frame before has left
    return group_stage(f, dst, left, right, stride, nullptr);
}

void group_pyr_fill(const visfs_flow* f, int slot, PyrRec* r) {
    for (int i = 0; i < 2; ++i) { r->px[i] = f->dpx[slot][i]; r->der[i] = f->dder[slot][i]; }
}

int group_pyramids(visfs_flow* f, int n, const PyrRec* d_recs, GroupCounts* cnt) {
    for (int l = 1; l < f->lay.n_levels; ++l) {
        const Level &S = f->lay.L[l - 1], &D = f->lay.L[l];
        hipLaunchKernelGGL(k_flow_pyr_down_g, dim3(blocks_for((int64_t)D.w * D.h, FL_T), 2, (unsigned)n), dim3(FL_T), 0, f->stream, d_recs, S.off, D.off,
                           S.w, S.h, D.w, D.h);
        HIP_TRY(f, hipGetLastError());
        ++cnt->launches;
    }
    hipLaunchKernelGGL(k_flow_scharr_g, dim3(blocks_for(f->lay.cells, FL_T), 2, (unsigned)n), dim3(FL_T), 0, f->stream, d_recs, f->lay);
    HIP_TRY(f, hipGetLastError());
    ++cnt->launches;
    return VISFS_BA_OK;
}

int device_pyramids(visfs_flow* f, int slot) {
    for (int l = 1; l < f->lay.n_levels; ++l) {
        const Level &S = f->lay.L[l - 1], &D = f->lay.L[l];
        PyrDownArgs A;
        for (int i = 0; i < 2; ++i) { A.src[i] = f->dpx[slot][i] + S.off; A.dst[i] = f->dpx[slot][i] + D.off; }
        A.sw = S.w; A.sh = S.h; A.dw = D.w; A.dh = D.h;
        hipLaunchKernelGGL(k_flow_pyr_down, dim3(blocks_for((int64_t)D.w * D.h, FL_T), 2), dim3(FL_T), 0, f->stream, A);
        HIP_TRY(f, hipGetLastError());
    }
    ScharrArgs S;
    for (int i = 0; i < 2; ++i) { S.px[i] = f->dpx[slot][i]; S.der[i] = f->dder[slot][i]; }
    hipLaunchKernelGGL(k_flow_scharr, dim3(blocks_for(f->lay.cells, FL_T), 2), dim3(FL_T), 0, f->stream, S, f->lay);
    HIP_TRY(f, hipGetLastError());
    return VISFS_BA_OK;
}

}  // namespace flow

namespace {

void host_push(visfs_flow* f, int slot, int image, const uint8_t* img, int32_t stride) {
    std::vector<uint8_t>& px = f->hpx[slot][image];
    px.resize((size_t)f->lay.cells);
    for (int32_t y = 0; y < f->h; ++y) std::memcpy(px.data() + (size_t)y * f->w, img + (size_t)y * stride, (size_t)f->w);
    host_pyramids(f, slot, image);
}

int device_push(visfs_flow* f, int slot, const uint8_t* left, const uint8_t* right, int32_t stride) {
    const int rc = device_stage(f, f->dpx[slot], left, right, stride);
    return rc != VISFS_BA_OK ? rc : device_pyramids(f, slot);
}

Image host_image(const visfs_flow* f, int slot, int image) { return Image{ f->hpx[slot][image].data(), f->hder[slot][image].data() }; }
Image device_image(const visfs_flow* f, int slot, int image) { return Image{ f->dpx[slot][image], f->dder[slot][image] }; }

// One gated pass for n points: template image (si, ii), moving image (sj, ij); cam != nullptr: the triangulation behind it.
int run_pass(visfs_flow* f, int si, int ii, int sj, int ij, int32_t n, const float* pts, const float* init, float gate, const Camera* cam,
             float* to, uint8_t* status, float* err, float* xyz) {
    if (n == 0) return VISFS_BA_OK;
    const bool back = f->prm.flow_back != 0;
    if (!f->device) {
        const Image I = host_image(f, si, ii), J = host_image(f, sj, ij);
        const HostCells pol;
        for (int32_t p = 0; p < n; ++p) {
            float tx, ty, e;
            uint8_t st;
            lk_gated(pol, f->lk, f->lay, I, J, pts[2 * p], pts[2 * p + 1], init != nullptr, init ? init[2 * p] : 0.0f,
                     init ? init[2 * p + 1] : 0.0f, back, gate, tx, ty, st, e);
            to[2 * p] = tx; to[2 * p + 1] = ty;
            status[p] = st;
            if (err) err[p] = e;
            if (cam) {
                float* o = xyz + 3 * p;
                o[0] = o[1] = o[2] = __builtin_nanf("");
                if (st) triangulate(*cam, pts[2 * p], pts[2 * p + 1], tx, o);
            }
        }
        return VISFS_BA_OK;
    }
    HIP_TRY(f, hipSetDevice(f->dev));
    int rc = io_reserve(f, n);
    if (rc != VISFS_BA_OK) return rc;
    HIP_TRY(f, hipStreamSynchronize(f->stream));                        // (the pinned block is free again)
    const IoLayout o = io_layout((size_t)n);
    std::memcpy(f->io.h.get() + o.pts, pts, 8 * (size_t)n);
    if (init) std::memcpy(f->io.h.get() + o.init, init, 8 * (size_t)n);
    HIP_TRY(f, hipMemcpyAsync(f->io.d.get(), f->io.h.get(), init ? o.in_bytes : o.init, hipMemcpyHostToDevice, f->stream));
    LkArgs A;
    A.I = device_image(f, si, ii); A.J = device_image(f, sj, ij);
    A.pts = reinterpret_cast<const float*>(f->io.d.get() + o.pts);
    A.init = init ? reinterpret_cast<const float*>(f->io.d.get() + o.init) : nullptr;
    A.to = reinterpret_cast<float*>(f->io.d.get() + o.to);
    A.err = reinterpret_cast<float*>(f->io.d.get() + o.err);
    A.xyz = reinterpret_cast<float*>(f->io.d.get() + o.xyz);
    A.status = reinterpret_cast<uint8_t*>(f->io.d.get() + o.status);
    A.n = n; A.gate = gate;
    const Camera c = cam ? *cam : Camera{};
    const dim3 grid((unsigned)n), block(64);
    if (cam) {
        if (back) hipLaunchKernelGGL((k_flow_lk<true, true>), grid, block, 0, f->stream, A, f->lk, f->lay, c);
        else hipLaunchKernelGGL((k_flow_lk<false, true>), grid, block, 0, f->stream, A, f->lk, f->lay, c);
    } else {
        if (back) hipLaunchKernelGGL((k_flow_lk<true, false>), grid, block, 0, f->stream, A, f->lk, f->lay, c);
        else hipLaunchKernelGGL((k_flow_lk<false, false>), grid, block, 0, f->stream, A, f->lk, f->lay, c);
    }
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipMemcpyAsync(f->io.h.get() + o.to, f->io.d.get() + o.to, o.status + (size_t)n - o.to, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    std::memcpy(to, f->io.h.get() + o.to, 8 * (size_t)n);
    std::memcpy(status, f->io.h.get() + o.status, (size_t)n);
    if (err) std::memcpy(err, f->io.h.get() + o.err, 4 * (size_t)n);
    if (cam) std::memcpy(xyz, f->io.h.get() + o.xyz, 12 * (size_t)n);
    return VISFS_BA_OK;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_flow_abi_version(void) { return VISFS_FLOW_ABI_VERSION; }

void visfs_flow_default_params(visfs_flow_params* p) {
    if (!p) return;
    p->win_size = 21; p->max_level = 3; p->iterations = 30; p->eps = 0.01f; p->flow_back = 1; p->min_eig_threshold = 1e-4f;
    p->back_gate_track = 1.5f; p->back_gate_stereo = 0.5f; p->min_depth = 0.2f; p->max_depth = 10.0f;
}

int visfs_flow_create_host(const visfs_flow_params* p, int32_t width, int32_t height, visfs_flow** out) {
    if (!p || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        std::string why;
        const int rc = check_params(p, width, height, why);
        if (rc != VISFS_BA_OK) return rc;
        visfs_flow* f = new visfs_flow();
        init_common(f, p, width, height);
        *out = f;
        return (int)VISFS_BA_OK;
    });
}

int visfs_flow_create(visfs_ba_handle* h, const visfs_flow_params* p, int32_t width, int32_t height, visfs_flow** out) {
    if (!h || !p || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        std::string why;
        int rc = check_params(p, width, height, why);
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, why.c_str()); return rc; }
        visfs_flow* f = new visfs_flow();
        init_common(f, p, width, height);
        f->device = true; f->ba = h; f->dev = visfs_internal_device(h); f->stream = visfs_internal_stream(h);
        rc = device_init(f);
        if (rc != VISFS_BA_OK) { visfs_internal_set_error(h, f->err.c_str()); delete f; return rc; }
        *out = f;
        return (int)VISFS_BA_OK;
    });
}

void visfs_flow_destroy(visfs_flow* f) {
    if (!f) return;
    flow::tracker_release(f);
    flow::corners_release(f);
    flow::clahe_release(f);
    delete f;
}

const char* visfs_flow_last_error(const visfs_flow* f) { return f ? f->err.c_str() : "null tracker"; }

int visfs_flow_push_frame(visfs_flow* f, const uint8_t* left, const uint8_t* right, int32_t stride) {
    if (!f || !left || !right) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (stride < f->w) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "stride is smaller than the image width");
        const int slot = f->frames == 0 ? f->cur : 1 - f->cur;
        if (f->device) {
            const int rc = device_push(f, slot, left, right, stride);
            if (rc != VISFS_BA_OK) return rc;
        } else {
            host_push(f, slot, 0, left, stride);
            host_push(f, slot, 1, right, stride);
        }
        f->cur = slot;
        ++f->frames;
        return (int)VISFS_BA_OK;
    });
}

int visfs_flow_track(visfs_flow* f, int32_t n, const float* from_xy, const float* guess_xy, float* to_xy, uint8_t* status, float* err) {
    if (!f || n < 0 || (n > 0 && (!from_xy || !to_xy || !status))) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (f->frames < 2) return fail(f, VISFS_BA_ERR_NOT_LOADED, "track needs two pushed frames");
        return run_pass(f, 1 - f->cur, 0, f->cur, 0, n, from_xy, guess_xy, f->prm.back_gate_track, nullptr, to_xy, status, err, nullptr);
    });
}

int visfs_flow_stereo(visfs_flow* f, int32_t n, const float* left_xy, const visfs_flow_camera* cam, float* right_xy, uint8_t* status,
                      float* xyz) {
    if (!f || !cam || n < 0 || (n > 0 && (!left_xy || !right_xy || !status || !xyz))) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (f->frames < 1) return fail(f, VISFS_BA_ERR_NOT_LOADED, "stereo needs a pushed frame");
        for (int i = 0; i < 12; ++i) if (!std::isfinite(cam->Tir[i])) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "Tir is not finite");
        const Camera c = make_camera(f->prm, *cam);
        return run_pass(f, f->cur, 0, f->cur, 1, n, left_xy, nullptr, f->prm.back_gate_stereo, &c, right_xy, status, nullptr, xyz);
    });
}

// ---- test hooks
int visfs_flow_level_size(const visfs_flow* f, int32_t level, int32_t* width, int32_t* height) {
    if (!f || !width || !height || level < 0 || level >= f->lay.n_levels) return VISFS_BA_ERR_BAD_ARGUMENT;
    *width = f->lay.L[level].w; *height = f->lay.L[level].h;
    return VISFS_BA_OK;
}

int visfs_flow_download_level(const visfs_flow* cf, int32_t slot, int32_t image, int32_t level, uint8_t* pixels, int16_t* derivative) {
    visfs_flow* f = const_cast<visfs_flow*>(cf);
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (slot < 0 || slot > 1 || image < 0 || image > 1 || level < 0 || level >= f->lay.n_levels)
            return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "slot, image or level out of range");
        if (f->frames < (slot == VISFS_FLOW_SLOT_CURRENT ? 1 : 2)) return fail(f, VISFS_BA_ERR_NOT_LOADED, "no frame in that slot");
        const int s = slot == VISFS_FLOW_SLOT_CURRENT ? f->cur : 1 - f->cur;
        const Level& L = f->lay.L[level];
        const size_t n = (size_t)L.w * L.h;
        if (!f->device) {
            if (pixels) std::memcpy(pixels, f->hpx[s][image].data() + L.off, n);
            if (derivative) std::memcpy(derivative, f->hder[s][image].data() + L.off, 4 * n);
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(f, hipSetDevice(f->dev));
        if (pixels) HIP_TRY(f, hipMemcpyAsync(pixels, f->dpx[s][image] + L.off, n, hipMemcpyDeviceToHost, f->stream));
        if (derivative) HIP_TRY(f, hipMemcpyAsync(derivative, f->dder[s][image] + L.off, 4 * n, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_flow_hook_triangulate(const visfs_flow_params* p, const visfs_flow_camera* cam, int32_t n, const float* left_xy,
                                const float* right_xy, float* xyz) {
    if (!p || !cam || n < 0 || (n > 0 && (!left_xy || !right_xy || !xyz))) return VISFS_BA_ERR_BAD_ARGUMENT;
    const Camera c = make_camera(*p, *cam);
    for (int32_t i = 0; i < n; ++i) triangulate(c, left_xy[2 * i], left_xy[2 * i + 1], right_xy[2 * i], xyz + 3 * i);
    return VISFS_BA_OK;
}

}  // extern "C"
