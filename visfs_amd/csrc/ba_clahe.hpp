// Contrast-limited adaptive histogram equalisation of 8-bit images (include/visfs_clahe.h): the arithmetic the
// kernels of ba_clahe.hip and the host restatement share.
//
// Histogram, clipping, redistribution and prefix sum are integer arithmetic, so they do not depend on the order of summation.  The
// look-up table takes one float32 multiply and one rounding, the blend of four tables float32 with one rounded operation per
// statement; contraction is switched off so that neither hipcc's device nor its host pass fuses a product into a sum.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace clahe {

#define CLAHE_HD __host__ __device__ inline

constexpr int kBins = 256;
constexpr int kMaxTiles = 32;     // per axis

struct Geom {
    int32_t w, h;                 // the image
    int32_t tiles_x, tiles_y;
    int32_t ext_w, ext_h;         // the reflected extension the tiles are cut from (an index map, never stored)
    int32_t tile_w, tile_h;
    int32_t clip;                 // counts per bin, 0: no clipping
    float lut_scale;              // 255.0f / (float)area
    float inv_tw, inv_th;         // 1.0f / tile_w, 1.0f / tile_h
};

// Tiles of a w x h image: the image as it is when both sides divide, otherwise tiles - side % tiles more columns and rows (a full
// tile count on a side that does divide).  The caller has checked 1 <= tiles <= kMaxTiles, tiles < side and clip_limit >= 0.
inline Geom make_geom(int32_t w, int32_t h, int32_t tiles_x, int32_t tiles_y, double clip_limit) {
    Geom g;
    g.w = w; g.h = h; g.tiles_x = tiles_x; g.tiles_y = tiles_y;
    const bool divides = w % tiles_x == 0 && h % tiles_y == 0;
    g.ext_w = divides ? w : w + (tiles_x - w % tiles_x);
    g.ext_h = divides ? h : h + (tiles_y - h % tiles_y);
    g.tile_w = g.ext_w / tiles_x; g.tile_h = g.ext_h / tiles_y;
    const int64_t area = (int64_t)g.tile_w * g.tile_h;
    g.clip = 0;
    if (clip_limit > 0.0) {
        const double c = clip_limit * (double)area / 256.0;
        g.clip = c >= (double)INT_MAX ? INT_MAX : (int32_t)c;      // (a bin never holds more than the area, so this clips nothing)
        if (g.clip < 1) g.clip = 1;
    }
    g.lut_scale = 255.0f / (float)area;
    g.inv_tw = 1.0f / (float)g.tile_w;
    g.inv_th = 1.0f / (float)g.tile_h;
    return g;
}

// BORDER_REFLECT_101 past the far edge: the extension never reaches further than one reflection
CLAHE_HD int ext_index(int i, int n) { return i >= n ? 2 * n - 2 - i : i; }

// What bin `bin` holds after the excess `clipped` of the whole tile went back: an equal share to every bin, the rest one each to
// bins 0, step, 2 step, ... ; `count` is the bin after min(count, clip).
CLAHE_HD int32_t redistribute(int32_t count, int bin, int32_t clipped) {
    const int32_t batch = clipped / kBins, residual = clipped - batch * kBins;
    count += batch;
    if (residual != 0) {
        const int32_t step = kBins / residual > 1 ? kBins / residual : 1;
        if (bin % step == 0 && bin / step < residual) ++count;
    }
    return count;
}

CLAHE_HD uint8_t round_u8(float v) {
    const float r = rintf(v);                                       // half to even
    return (uint8_t)(r < 0.0f ? 0.0f : r > 255.0f ? 255.0f : r);
}

CLAHE_HD uint8_t lut_value(int32_t cumulative, float lut_scale) {
    const float s = (float)cumulative * lut_scale;
    return round_u8(s);
}

// The two tiles and weights of one axis for pixel coordinate c.
struct Axis { int32_t t1, t2; float a, a1; };
CLAHE_HD Axis axis_of(int c, float inv_tile, int tiles) {
    const float scaled = (float)c * inv_tile;
    const float tf = scaled - 0.5f;
    const float fl = floorf(tf);
    int32_t t1 = (int32_t)fl;
    Axis o;
    o.a = tf - fl;
    o.a1 = 1.0f - o.a;
    o.t2 = t1 + 1 < tiles - 1 ? t1 + 1 : tiles - 1;
    o.t1 = t1 > 0 ? t1 : 0;
    return o;
}

// lut: [tiles_y][tiles_x][256] of one image
CLAHE_HD uint8_t blend(const uint8_t* lut, int tiles_x, const Axis& X, const Axis& Y, int v) {
    const uint8_t* r1 = lut + (int64_t)Y.t1 * tiles_x * kBins + v;
    const uint8_t* r2 = lut + (int64_t)Y.t2 * tiles_x * kBins + v;
    const float p11 = (float)r1[X.t1 * kBins] * X.a1, p12 = (float)r1[X.t2 * kBins] * X.a;
    const float p21 = (float)r2[X.t1 * kBins] * X.a1, p22 = (float)r2[X.t2 * kBins] * X.a;
    const float top = p11 + p12, bot = p21 + p22;
    const float wt = top * Y.a1, wb = bot * Y.a;
    const float res = wt + wb;
    return round_u8(res);
}

}  // namespace clahe
