// Pyramidal Lucas-Kanade tracking and stereo triangulation (include/visfs_flow.h): the work items the kernels
// of ba_flow.hip and the host restatement (visfs_flow_create_host) share.
//
// Everything up to the window sums is integer arithmetic (fixed-point bilinear weights, CV_DESCALE rounding, exact int64 sums), so
// it is independent of the order of summation and of the compiler.  The scalar tail is float32, one rounded operation per
// statement; contraction is switched off for this translation unit so that neither hipcc's device nor its host pass fuses a
// product into a sum.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

struct visfs_ba_handle;

namespace flow {

#define FLOW_HD __host__ __device__ inline

constexpr int kMaxLevels = 8;     // max_level 0 .. 7
constexpr int kMaxWin = 21;       // 21 x 21 = 441 window cells: 7 per lane of a wavefront
constexpr int kWBits = 14;        // fixed-point bits of the bilinear weights
constexpr int kLaneSlots = 7;

struct Level {
    int32_t w, h;
    int64_t off;                  // first cell of the level in an image's storage (pixels: bytes; derivative: int16 pairs)
};

struct Layout {
    Level L[kMaxLevels];
    int32_t n_levels;
    int64_t cells;                // cells of all levels
};

struct LkParams {
    int32_t win, max_level, iterations;
    float eps2, min_eig;
};

struct Camera {
    float fx, fy, cx, cy, cx_right, baseline, min_depth, max_depth;
    double T[12];
};

FLOW_HD int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

// pyrDown: separable (1 4 6 4 1), BORDER_REFLECT_101, (v + 128) >> 8
FLOW_HD uint8_t pyr_down_cell(const uint8_t* s, int sw, int sh, int x, int y) {
    const int k[5] = { 1, 4, 6, 4, 1 };
    int xs[5];
    for (int i = 0; i < 5; ++i) xs[i] = reflect101(2 * x + i - 2, sw);
    int acc = 0;
    for (int j = 0; j < 5; ++j) {
        const uint8_t* r = s + (int64_t)reflect101(2 * y + j - 2, sh) * sw;
        int row = 0;
        for (int i = 0; i < 5; ++i) row += k[i] * (int)r[xs[i]];
        acc += k[j] * row;
    }
    return (uint8_t)((acc + 128) >> 8);
}

// unnormalised Scharr, image border REFLECT_101; the (Ix, Iy) pair packed as the derivative storage holds it
FLOW_HD uint32_t scharr_cell(const uint8_t* p, int w, int h, int x, int y) {
    const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
    const uint8_t* r0 = p + (int64_t)reflect101(y - 1, h) * w;
    const uint8_t* r1 = p + (int64_t)y * w;
    const uint8_t* r2 = p + (int64_t)reflect101(y + 1, h) * w;
    const int ix = 3 * ((int)r0[xp] - (int)r0[xm]) + 10 * ((int)r1[xp] - (int)r1[xm]) + 3 * ((int)r2[xp] - (int)r2[xm]);
    const int iy = 3 * ((int)r2[xm] - (int)r0[xm]) + 10 * ((int)r2[x] - (int)r0[x]) + 3 * ((int)r2[xp] - (int)r0[xp]);
    return (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
}

// floor of a window corner and whether it stays in [-win, cols) x [-win, rows); decided on the floats, so NaN is outside
FLOW_HD bool corner(float px, float py, int win, int w, int h, int& ix, int& iy) {
    const float fx = floorf(px), fy = floorf(py);
    const bool ok = fx >= (float)(-win) && fx < (float)w && fy >= (float)(-win) && fy < (float)h;
    ix = ok ? (int)fx : 0;
    iy = ok ? (int)fy : 0;
    return ok;
}

struct Weights { int32_t w00, w01, w10, w11; };

FLOW_HD Weights weights(float px, float py, int ix, int iy) {
    const float a = px - (float)ix;
    const float b = py - (float)iy;
    const float na = 1.0f - a;
    const float nb = 1.0f - b;
    const float s = (float)(1 << kWBits);
    const float p00 = na * nb;
    const float p01 = a * nb;
    const float p10 = na * b;
    Weights q;
    q.w00 = (int32_t)rintf(p00 * s);
    q.w01 = (int32_t)rintf(p01 * s);
    q.w10 = (int32_t)rintf(p10 * s);
    q.w11 = (1 << kWBits) - q.w00 - q.w01 - q.w10;
    return q;
}

FLOW_HD int32_t descale(int32_t v, int bits) { return (v + (1 << (bits - 1))) >> bits; }

// the bilinear sample of the pixels whose top-left neighbour is (x, y), 5 fractional bits kept; REFLECT_101 outside the level
FLOW_HD int32_t sample_px(const uint8_t* img, int w, int h, int x, int y, const Weights& q) {
    const int x0 = reflect101(x, w), x1 = reflect101(x + 1, w);
    const uint8_t* r0 = img + (int64_t)reflect101(y, h) * w;
    const uint8_t* r1 = img + (int64_t)reflect101(y + 1, h) * w;
    const int32_t v = (int32_t)r0[x0] * q.w00 + (int32_t)r0[x1] * q.w01 + (int32_t)r1[x0] * q.w10 + (int32_t)r1[x1] * q.w11;
    return descale(v, kWBits - 5);
}

// the bilinear sample of the derivative pairs; 0 outside the level
FLOW_HD void sample_der(const uint32_t* der, int w, int h, int x, int y, const Weights& q, int32_t& gx, int32_t& gy) {
    const bool cx0 = x >= 0 && x < w, cx1 = x + 1 >= 0 && x + 1 < w;
    const bool cy0 = y >= 0 && y < h, cy1 = y + 1 >= 0 && y + 1 < h;
    const uint32_t d00 = (cx0 && cy0) ? der[(int64_t)y * w + x] : 0u;
    const uint32_t d01 = (cx1 && cy0) ? der[(int64_t)y * w + x + 1] : 0u;
    const uint32_t d10 = (cx0 && cy1) ? der[(int64_t)(y + 1) * w + x] : 0u;
    const uint32_t d11 = (cx1 && cy1) ? der[(int64_t)(y + 1) * w + x + 1] : 0u;
    auto lo = [](uint32_t d) { return (int32_t)(int16_t)(uint16_t)(d & 0xffffu); };
    auto hi = [](uint32_t d) { return (int32_t)(int16_t)(uint16_t)(d >> 16); };
    gx = descale(lo(d00) * q.w00 + lo(d01) * q.w01 + lo(d10) * q.w10 + lo(d11) * q.w11, kWBits);
    gy = descale(hi(d00) * q.w00 + hi(d01) * q.w01 + hi(d10) * q.w10 + hi(d11) * q.w11, kWBits);
}

// ---------------------------------------------------------------- the scalar tail (float32, one operation per statement)
struct Normal { float A11, A12, A22, D, min_eig; };

FLOW_HD Normal tail_normal(int64_t s11, int64_t s12, int64_t s22, int win) {
    const float scale = 9.5367431640625e-07f;      // 2^-20
    Normal m;
    m.A11 = (float)s11 * scale;
    m.A12 = (float)s12 * scale;
    m.A22 = (float)s22 * scale;
    const float t0 = m.A11 * m.A22;
    const float t1 = m.A12 * m.A12;
    m.D = t0 - t1;
    const float df = m.A11 - m.A22;
    const float df2 = df * df;
    const float q = 4.0f * m.A12;
    const float q2 = q * m.A12;
    const float rad = sqrtf(df2 + q2);
    const float tr = m.A22 + m.A11;
    const float num = tr - rad;
    m.min_eig = num / (float)(2 * win * win);
    return m;
}

FLOW_HD void tail_step(const Normal& m, int64_t sb1, int64_t sb2, float& dx, float& dy) {
    const float scale = 9.5367431640625e-07f;
    const float b1 = (float)sb1 * scale;
    const float b2 = (float)sb2 * scale;
    const float u0 = m.A12 * b2;
    const float u1 = m.A22 * b1;
    dx = (u0 - u1) / m.D;
    const float v0 = m.A12 * b1;
    const float v1 = m.A11 * b2;
    dy = (v0 - v1) / m.D;
}

FLOW_HD float l2_distance(float ax, float ay, float bx, float by) {
    const float dx = ax - bx;
    const float dy = ay - by;
    const float dx2 = dx * dx;
    const float dy2 = dy * dy;
    return sqrtf(dx2 + dy2);
}

// ---------------------------------------------------------------- one calcOpticalFlowPyrLK pass of one point
// Policy P spreads the window cells: kSlots cells per caller, cell(s) their index (>= win * win: none), acc_t the partial sum type,
// total() the sum over all callers.  HostCells walks all cells on one core; the kernel's policy gives 7 to each lane of a wavefront.
struct HostCells {
    static constexpr int kSlots = kMaxWin * kMaxWin;
    using acc_t = int64_t;
    FLOW_HD int cell(int s) const { return s; }
    FLOW_HD int64_t total(acc_t v) const { return v; }
};

struct Image {
    const uint8_t* px;
    const uint32_t* der;
};

template <class P>
FLOW_HD void lk_pass(const P& pol, const LkParams& prm, const Layout& lay, const Image& I, const Image& J, float ptx, float pty,
                     bool has_init, float inx, float iny, float& outx, float& outy, uint8_t& status, float& err) {
    const int win = prm.win, cells = win * win;
    const float half = (float)(win - 1) * 0.5f;
    int32_t cxy[P::kSlots];                        // the cell's (column, row), or -1
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int s = 0; s < P::kSlots; ++s) {
        const int c = pol.cell(s);
        cxy[s] = c < cells ? ((c / win) << 8 | (c % win)) : -1;
    }
    int32_t tI[P::kSlots], tG[P::kSlots];          // the template: I (5 fractional bits) and the (Ix, Iy) pair packed
    status = 1;
    err = 0.0f;
    float nx = 0.0f, ny = 0.0f;
    for (int level = prm.max_level; level >= 0; --level) {
        const Level& L = lay.L[level];
        const float sc = 1.0f / (float)(1 << level);
        float px = ptx * sc, py = pty * sc;
        if (level == prm.max_level) {
            nx = has_init ? inx * sc : px;
            ny = has_init ? iny * sc : py;
        } else {
            nx = nx * 2.0f;
            ny = ny * 2.0f;
        }
        px = px - half;
        py = py - half;
        int ix, iy;
        if (!corner(px, py, win, L.w, L.h, ix, iy)) {
            if (level == 0) { status = 0; err = 0.0f; }
            continue;
        }
        const uint8_t* Ipx = I.px + L.off;
        const uint32_t* Ider = I.der + L.off;
        const uint8_t* Jpx = J.px + L.off;
        const Weights q = weights(px, py, ix, iy);
        typename P::acc_t s11 = 0, s12 = 0, s22 = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (int s = 0; s < P::kSlots; ++s) {
            int32_t v = 0, gx = 0, gy = 0;
            if (cxy[s] >= 0) {
                const int x = ix + (cxy[s] & 0xff), y = iy + (cxy[s] >> 8);
                v = sample_px(Ipx, L.w, L.h, x, y, q);
                sample_der(Ider, L.w, L.h, x, y, q, gx, gy);
            }
            tI[s] = v;
            tG[s] = (int32_t)((uint32_t)(uint16_t)(int16_t)gx | ((uint32_t)(uint16_t)(int16_t)gy << 16));
            s11 += gx * gx;
            s12 += gx * gy;
            s22 += gy * gy;
        }
        const Normal m = tail_normal(pol.total(s11), pol.total(s12), pol.total(s22), win);
        err = m.min_eig;
        if (m.min_eig < prm.min_eig || m.D < FLT_EPSILON) {
            if (level == 0) status = 0;
            continue;
        }
        float cx = nx - half, cy = ny - half;      // corner of the moving window
        float pdx = 0.0f, pdy = 0.0f;
        for (int j = 0; j < prm.iterations; ++j) {
            int jx, jy;
            if (!corner(cx, cy, win, L.w, L.h, jx, jy)) {
                if (level == 0) status = 0;
                break;
            }
            const Weights qj = weights(cx, cy, jx, jy);
            typename P::acc_t sb1 = 0, sb2 = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
            for (int s = 0; s < P::kSlots; ++s) {
                if (cxy[s] < 0) continue;
                const int x = jx + (cxy[s] & 0xff), y = jy + (cxy[s] >> 8);
                const int32_t diff = sample_px(Jpx, L.w, L.h, x, y, qj) - tI[s];
                sb1 += diff * (int32_t)(int16_t)(uint16_t)((uint32_t)tG[s] & 0xffffu);
                sb2 += diff * (int32_t)(int16_t)(uint16_t)((uint32_t)tG[s] >> 16);
            }
            float dx, dy;
            tail_step(m, pol.total(sb1), pol.total(sb2), dx, dy);
            cx = cx + dx;
            cy = cy + dy;
            nx = cx + half;
            ny = cy + half;
            const float dxx = dx * dx;
            const float dyy = dy * dy;
            if (dxx + dyy <= prm.eps2) break;
            if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
                nx = nx - dx * 0.5f;
                ny = ny - dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
    }
    outx = nx;
    outy = ny;
}

// Forward pass and, when `back`, the reverse pass started from the point, with the gate on the round trip.  The reverse pass of a
// point the forward pass dropped cannot change what is reported, and is not run.
template <class P>
FLOW_HD void lk_gated(const P& pol, const LkParams& prm, const Layout& lay, const Image& I, const Image& J, float ptx, float pty,
                      bool has_init, float inx, float iny, bool back, float gate, float& tox, float& toy, uint8_t& status, float& err) {
    lk_pass(pol, prm, lay, I, J, ptx, pty, has_init, inx, iny, tox, toy, status, err);
    if (!back || !status) return;
    float bx, by, berr;
    uint8_t bst;
    lk_pass(pol, prm, lay, J, I, tox, toy, true, ptx, pty, bx, by, bst, berr);
    const float d = l2_distance(bx, by, ptx, pty);
    status = (bst && d <= gate) ? 1 : 0;
}

// generateKeyPoints3DStereo of one pair: projectDisparityTo3D in float as written, the depth gates, the image -> robot transform in
// double (each row summed left to right) rounded to float; NaN where the reference leaves badPoint.
FLOW_HD void triangulate(const Camera& c, float lx, float ly, float rx, float xyz[3]) {
    const float bad = __builtin_nanf("");
    xyz[0] = xyz[1] = xyz[2] = bad;
    const float disp = lx - rx;
    if (!(disp != 0.0f)) return;
    if (!(disp > 0.0f && c.baseline > 0.0f && c.fx > 0.0f)) return;
    float cc = 0.0f;
    if (c.cx > 0.0f && c.cx_right > 0.0f) cc = c.cx_right - c.cx;
    const float den = disp + cc;
    const float W = c.baseline / den;
    const float ux = lx - c.cx;
    const float uy = ly - c.cy;
    const float x = ux * W;
    const float y = uy * W;
    const float z = c.fx * W;
    if (!(__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z))) return;
    if (!((c.min_depth < 0.0f || z > c.min_depth) && (c.max_depth <= 0.0f || z <= c.max_depth))) return;
    const double p0 = (double)x, p1 = (double)y, p2 = (double)z;
    for (int r = 0; r < 3; ++r) {
        const double a = c.T[4 * r] * p0;
        const double b = c.T[4 * r + 1] * p1;
        const double d = c.T[4 * r + 2] * p2;
        const double s0 = a + b;
        const double s1 = s0 + d;
        xyz[r] = (float)(s1 + c.T[4 * r + 3]);
    }
}

}  // namespace flow

// Internal entry points of ba_api.cpp (the handle's device and stream).
hipStream_t visfs_internal_stream(visfs_ba_handle* h);
int visfs_internal_device(visfs_ba_handle* h);
void visfs_internal_set_error(visfs_ba_handle* h, const char* msg);
