// The resident front end (include/visfs_tracker.h): the arithmetic and the decisions the kernels of
// ba_tracker.hip and the host restatement share.
//
// The guess projection is float64, one rounded operation per statement, sums left to right; contraction is switched off so that
// neither hipcc's device nor its host pass fuses a product into a sum.  Everything else here is a comparison or an integer.
#pragma once
#include "ba_corners.hpp"

#pragma clang fp contract(off)

namespace trk {

constexpr int kMaxFeatures = 4096;
constexpr int kMaxOutliers = 4096;

// result flags of include/visfs_tracker.h
constexpr int32_t kNoPrevious = 1, kBootstrapped = 2, kLost = 4;

// guessCameraRef of Tracker.cpp:240 and the left camera's K in double (cvKdouble, :250)
struct Guess {
    double R[9], t[3];
    double fx, fy, cx, cy;
};

// (delta_guess * Tir)^-1 of two 3x4 row-major isometries: the product, then (R^T | -R^T t)
inline void guess_camera_ref(const double D[12], const double T[12], Guess& g) {
    double R[9], t[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            const double a = D[4 * i] * T[j];
            const double b = D[4 * i + 1] * T[4 + j];
            const double c = D[4 * i + 2] * T[8 + j];
            const double s = a + b;
            R[3 * i + j] = s + c;
        }
        const double a = D[4 * i] * T[3];
        const double b = D[4 * i + 1] * T[7];
        const double c = D[4 * i + 2] * T[11];
        const double s0 = a + b;
        const double s1 = s0 + c;
        t[i] = s1 + D[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) g.R[3 * i + j] = R[3 * j + i];
        const double a = R[i] * t[0];
        const double b = R[3 + i] * t[1];
        const double c = R[6 + i] * t[2];
        const double s0 = a + b;
        const double s1 = s0 + c;
        g.t[i] = -s1;
    }
}

// cv::projectPoints without distortion (Tracker.cpp:251): X = R P + t, u = fx X / Z + cx, v = fy Y / Z + cy, cast to float.  The
// Rodrigues round trip in front of it (:242-247) is the identity up to rounding and is not restated.
FLOW_HD void project_guess(const Guess& g, const float p[3], float& u, float& v) {
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
    double X[3];
    for (int r = 0; r < 3; ++r) {
        const double a = g.R[3 * r] * p0;
        const double b = g.R[3 * r + 1] * p1;
        const double c = g.R[3 * r + 2] * p2;
        const double s0 = a + b;
        const double s1 = s0 + c;
        X[r] = s1 + g.t[r];
    }
    const double nx = g.fx * X[0];
    const double ny = g.fy * X[1];
    const double qx = nx / X[2];
    const double qy = ny / X[2];
    u = (float)(qx + g.cx);
    v = (float)(qy + g.cy);
}

// uIsInBounds(v, 0, size) of utilite/include/Math.h:47: finite, >= 0, < size
FLOW_HD bool in_bounds(float v, int32_t size) { return __builtin_isfinite(v) && v >= 0.0f && v < (float)size; }

// a row of the table after the track pass is a covisible word (Tracker.cpp:286)
FLOW_HD bool kept_row(uint8_t status, float x, float y, int32_t w, int32_t h) { return status != 0 && in_bounds(x, w) && in_bounds(y, h); }

// getMask's order (Tracker.cpp:126) with FlowTracker::maskDiscs' stable rule: count descending, equal counts in row (= id) order
FLOW_HD bool drawn_before(int32_t cnt_a, int32_t row_a, int32_t cnt_b, int32_t row_b) {
    return cnt_a > cnt_b || (cnt_a == cnt_b && row_a < row_b);
}

// The draw decision's view of a disc: the rounded centre packed with which of the two radii it has.  Centres of kept and blocked
// words lie in [0, 16384] (they passed the bounds test of an image of at most 16384 pixels a side), so 15 bits hold each.
FLOW_HD uint32_t pack_disc(int32_t cx, int32_t cy, int kind) { return (uint32_t)cx | ((uint32_t)cy << 15) | ((uint32_t)kind << 30); }
FLOW_HD flow::Disc unpack_disc(uint32_t p, int32_t r_track, int32_t r_blocked) {
    const int kind = (int)(p >> 30);
    return flow::Disc{ (int32_t)(p & 0x7fffu), (int32_t)((p >> 15) & 0x7fffu), kind ? r_blocked : r_track, kind ? r_track + 1 : 0 };
}
FLOW_HD bool centre_inside(int32_t cx, int32_t cy, int32_t w, int32_t h) { return cx >= 0 && cx < w && cy >= 0 && cy < h; }
// a drawn disc that does not touch the image is not part of the raster (as decide_discs of ba_corners.hip leaves it out)
FLOW_HD bool touches_image(const flow::Disc& d, int32_t w, int32_t h) {
    return !(d.cx + d.r < 0 || d.cx - d.r >= w || d.cy + d.r < 0 || d.cy - d.r >= h);
}

// a stereo row survives (Tracker.cpp:376, :390)
FLOW_HD bool stereo_row(uint8_t status, float rx, float ry, const float xyz[3], int32_t w, int32_t h) {
    return status != 0 && in_bounds(rx, w) && in_bounds(ry, h) && __builtin_isfinite(xyz[0]) && __builtin_isfinite(xyz[1]) &&
           __builtin_isfinite(xyz[2]);
}

}  // namespace trk
