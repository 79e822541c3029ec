// ba_place_verify.hpp — the arithmetic of the guided search of a verified place query (include/visfs_place_verify.h, DESIGN.md section
// 9x) that the HIP kernel of ba_place_verify.hip and the one-core twin share: the window test, an entry's pick, a query's keep, and
// the twin over plain arrays.  The projection of an entry is pnp::project and stays with ba_place_verify.hip; this file takes pixels.
// It needs nothing of HIP: a host compiler takes it as it is (tools/place_verify_sanitize.cpp).
#pragma once

#include "ba_place.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace place_verify {

using place::kDescWords;
using place::kMaxPoints;

constexpr int32_t kNone = -1;

// Is the query at (qx, qy) inside the window of radius sqrt(r2) about the projection (pu, pv)?  In double, in this order: the two
// differences from the query's float pixel, their two squares, one sum, one comparison; nothing is contracted.  A pixel that is not
// finite is in no window.
PLACE_HD bool in_window(double pu, double pv, float qx, float qy, double r2) {
    const double dx = (double)qx - pu, dy = (double)qy - pv;
    const double xx = dx * dx, yy = dy * dy;
    const double d2 = xx + yy;
    return d2 <= r2;
}

// the radius squared as the device and the twin both take it
PLACE_HD double radius2(float r) { return (double)r * (double)r; }

// an entry's pick among the queries, and a query's keep among the entries that picked it: both the minimum of D * 1024 + index
PLACE_HD int32_t pair_key(int d, int index) { return d * 1024 + index; }
PLACE_HD int32_t better(int32_t key, int32_t best) { return (best == kNone || key < best) ? key : best; }

// One entry: e[8] its descriptor, (pu, pv) its projection.  Returns D * 1024 + i of the query it picks, or kNone.
PLACE_HD int32_t pick_of(const uint32_t* e, double pu, double pv, const uint32_t* qdesc, const uint8_t* qvalid, const float* qxy, int nq, double r2,
                         int max_distance) {
    int32_t best = kNone;
    for (int i = 0; i < nq; ++i) {
        if (!qvalid[i] || !in_window(pu, pv, qxy[2 * i], qxy[2 * i + 1], r2)) continue;
        const int d = place::hamming(qdesc + kDescWords * i, e);
        if (d <= max_distance) best = better(pair_key(d, i), best);
    }
    return best;
}

// One query: D * 1024 + j of the entry it keeps among those whose pick is i, or kNone.
PLACE_HD int32_t keep_of(int i, const int32_t* pick, int ne) {
    int32_t best = kNone;
    for (int j = 0; j < ne; ++j) {
        const int32_t p = pick[j];
        if (p != kNone && (p & 1023) == i) best = better(pair_key(p >> 10, j), best);
    }
    return best;
}

// ---------------------------------------------------------------------------------------------------------------- the one-core twin
// ok[j]: entry j is valid, has a finite point, a positive depth and a finite pixel (pu[j], pv[j]).  pick and keep have kMaxPoints
// entries each; those from ne and from nq on are kNone.  Returns the number of kept pairs.
inline int guided_twin(const double* pu, const double* pv, const uint8_t* ok, const uint32_t* edesc, int ne, const uint32_t* qdesc,
                       const uint8_t* qvalid, const float* qxy, int nq, double r2, int max_distance, int32_t* pick, int32_t* keep) {
    for (int j = 0; j < kMaxPoints; ++j)
        pick[j] = (j < ne && ok[j]) ? pick_of(edesc + kDescWords * j, pu[j], pv[j], qdesc, qvalid, qxy, nq, r2, max_distance) : kNone;
    int kept = 0;
    for (int i = 0; i < kMaxPoints; ++i) {
        keep[i] = i < nq ? keep_of(i, pick, ne) : kNone;
        kept += keep[i] != kNone;
    }
    return kept;
}

}  // namespace place_verify
