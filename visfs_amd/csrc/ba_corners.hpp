// Corner extraction (include/visfs_corners.h): the arithmetic the kernels of ba_corners.hip and the host
// restatement share.
//
// Derivatives, products and box sums are int32 and exact, so they do not depend on the order of summation.  The response is float32,
// one rounded operation per statement; contraction is switched off so that neither hipcc's device nor its host pass fuses a product
// into a sum.  Keys, the mask's discs and the distance test are integers again.
#pragma once
#include "ba_flow.hpp"

#pragma clang fp contract(off)

namespace flow {

constexpr int kMaxCorners = 4096;
constexpr int kMaxRadius = 32768;

// Sobel 3 x 3, unnormalised, of the pixel (x, y) inside the image; the image border reflects (REFLECT_101)
FLOW_HD void sobel_cell(const uint8_t* p, int w, int h, int x, int y, int& dx, int& dy) {
    const int xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
    const uint8_t* r0 = p + (int64_t)reflect101(y - 1, h) * w;
    const uint8_t* r1 = p + (int64_t)y * w;
    const uint8_t* r2 = p + (int64_t)reflect101(y + 1, h) * w;
    dx = ((int)r0[xp] + 2 * (int)r1[xp] + (int)r2[xp]) - ((int)r0[xm] + 2 * (int)r1[xm] + (int)r2[xm]);
    dy = ((int)r2[xm] + 2 * (int)r2[x] + (int)r2[xp]) - ((int)r0[xm] + 2 * (int)r0[x] + (int)r0[xp]);
}

// the minimum eigenvalue of the 2 x 2 matrix of box sums, as cornerMinEigenVal scales it (1 / (255 * 4 * 3) per derivative)
FLOW_HD float min_eig_response(int32_t sxx, int32_t sxy, int32_t syy) {
    const float k = (float)(1.0 / (3060.0 * 3060.0));
    const float ak = (float)sxx * k;
    const float a = ak * 0.5f;
    const float b = (float)sxy * k;
    const float ck = (float)syy * k;
    const float c = ck * 0.5f;
    const float d = a - c;
    const float d2 = d * d;
    const float b2 = b * b;
    const float s = d2 + b2;
    const float r = sqrtf(s);
    const float t = a + c;
    return t - r;
}

// a float as an unsigned integer of the same order; 0 is no float's image but a NaN's, and stands for "none"
FLOW_HD uint32_t ordered_bits(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FLOW_HD float from_ordered_bits(uint32_t o) {
    if (o == 0u) return 0.0f;
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __builtin_bit_cast(float, u);
}

// t = (float)((double)maxVal * quality_level)
FLOW_HD float quality_threshold(float max_val, double quality) {
    const double t = (double)max_val * quality;
    return (float)t;
}

// the sort key of a candidate: the response in the order of its value, the raster index breaks ties (both descending); never 0
FLOW_HD uint64_t corner_key(float v, uint32_t index) { return ((uint64_t)ordered_bits(v) << 32) | index; }

// a disc as the raster reads it: centre, radius and where its half-width table starts
struct Disc { int32_t cx, cy, r, hw; };

// the half-widths of cv::circle(..., thickness = -1)'s midpoint walk: hw[0 .. r]
inline void disc_halfwidth(int r, int32_t* hw) {
    for (int i = 0; i <= r; ++i) hw[i] = -1;
    int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
    while (dx >= dy) {
        if (hw[dy] < dx) hw[dy] = dx;
        if (hw[dx] < dy) hw[dx] = dy;
        ++dy;
        err += plus;
        plus += 2;
        const int m = (err <= 0) - 1;
        err -= minus & m;
        dx += m;
        minus -= m & 2;
    }
}

// lrintf with the default rounding (half to even), kept within what the integer tests behind it can hold
FLOW_HD int32_t round_centre(float v) {
    const double r = rint((double)v);
    return (int32_t)fmin(fmax(r, -1073741824.0), 1073741824.0);
}

FLOW_HD bool disc_covers(const Disc& d, const int32_t* hw, int x, int y) {
    int ay = y - d.cy;
    if (ay < 0) ay = -ay;
    if (ay > d.r) return false;
    int ax = x - d.cx;
    if (ax < 0) ax = -ax;
    return ax <= hw[d.hw + ay];
}

// disc_covers without a branch: the table is read at a clamped row whatever the answer, so a loop over discs has no load that
// waits for a comparison (hw: the table of this disc, hw[0 .. r])
FLOW_HD bool disc_covers_flat(int cx, int cy, int r, const int32_t* hw, int x, int y) {
    int ay = y - cy;
    ay = ay < 0 ? -ay : ay;
    int ax = x - cx;
    ax = ax < 0 ? -ax : ax;
    const int32_t half = hw[ay < r ? ay : r];
    return ay <= r && ax <= half;
}

FLOW_HD bool masked(const Disc* discs, int n, const int32_t* hw, int x, int y) {
    for (int i = 0; i < n; ++i)
        if (disc_covers(discs[i], hw, x, y)) return true;
    return false;
}

// (dx^2 + dy^2 < min_distance^2) for integer offsets is (dx^2 + dy^2 < ceil(min_distance^2)); 2 * 16384^2 fits int32
inline int32_t distance_gate(double min_distance) {
    const double d2 = std::ceil(min_distance * min_distance);
    return d2 >= 2147483647.0 ? 2147483647 : (int32_t)d2;
}

FLOW_HD bool too_close(int32_t a, int32_t b, int32_t gate) {       // points packed x | y << 16
    const int dx = (a & 0xffff) - (b & 0xffff), dy = (a >> 16) - (b >> 16);
    return dx * dx + dy * dy < gate;
}

}  // namespace flow
