// Branch-and-bound scan matching over frozen grid stacks (include/visfs_scan_fast.h): what the kernels of
// ba_scan_fast.hip and the one-core twin share.  Everything here is integer work on the cells that scan::discretise (ba_scan.hpp)
// forms, so the device and the twin agree by construction.
#pragma once
#include "ba_scan.hpp"
#include "../../include/visfs_scan_fast.h"

namespace scanfast {

constexpr int kThreads = 256;                 // work items of one workgroup: four wavefronts
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxDepth = VISFS_SCAN_FAST_MAX_DEPTH;

// Level h of a stack as stored: [ht][w] uint16 over x in [-e, nx), y in [-e, ny), e = 2^h - 1 (the low-side extension: a window
// that starts left of or above the grid still reaches into it); everything outside reads 0.
struct LevelView {
    const uint16_t* p = nullptr;
    int32_t w = 0, ht = 0, e = 0;
};

struct Levels { LevelView v[kMaxDepth]; };

// P_h(x, y), bounds-checked against the extended array (x, y: the limits' cell coordinates, |x|, |y| <= 2^30 + 2^16)
__host__ __device__ inline int32_t level_read(const LevelView& v, int32_t x, int32_t y) {
    x += v.e; y += v.e;
    if (x < 0 || y < 0 || x >= v.w || y >= v.ht) return 0;
    return v.p[(int64_t)y * v.w + x];
}

// P_h at the stored position (sx, sy) from level h - 1: the maximum of its four values at offsets 0 and 2^(h-1) per axis
__host__ __device__ inline uint16_t level_up(const LevelView& lo, int32_t e_hi, int32_t half, int32_t sx, int32_t sy) {
    const int32_t x = sx - e_hi, y = sy - e_hi;
    int32_t m = level_read(lo, x, y);
    const int32_t b = level_read(lo, x + half, y), c = level_read(lo, x, y + half), d = level_read(lo, x + half, y + half);
    if (b > m) m = b;
    if (c > m) m = c;
    if (d > m) m = d;
    return (uint16_t)m;
}

// nodes per axis of level h in a window of L offsets: offsets -nl + i * 2^h, i in [0, nodes_per_axis)
__host__ __device__ inline int32_t nodes_per_axis(int32_t L, int32_t h) { return (int32_t)(((int64_t)L + ((int64_t)1 << h) - 1) >> h); }

// A node of level h is (k, i, j): scan k, offsets xo = -nl + i 2^h, yo = -nl + j 2^h; its id is (k m + i) m + j with m nodes per
// axis, which at level 0 is the generation-order index of the leaf.
__host__ __device__ inline int32_t node_id(int32_t m, int32_t k, int32_t i, int32_t j) { return (k * m + i) * m + j; }
__host__ __device__ inline void node_decode(int32_t m, int32_t id, int32_t& k, int32_t& i, int32_t& j) {
    j = id % m; const int32_t r = id / m; i = r % m; k = r / m;
}

// the order of the search: the larger sum, and among equal sums the lower id
__host__ __device__ inline bool better(int32_t ua, int32_t ia, int32_t ub, int32_t ib) { return ua > ub || (ua == ub && ia < ib); }

// what the device reports of one call, in one download
struct Ctrl {
    int32_t B;                                // the incumbent: the best leaf sum of the greedy descents
    int32_t overflow;                         // 0, or 1 + the highest level whose kept set exceeded the capacity
    int32_t best_index, best_sum;
    int32_t scored[kMaxDepth], kept[kMaxDepth];
};

}  // namespace scanfast
