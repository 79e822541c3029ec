// KLD-adaptive particle counts (include/visfs_mcl_kld.h): the definition of the bins, of the limit table and
// of the record, which k_mcl_kld_resample of ba_mcl_kld.hip and the one-core twin both use.
//
// The device and the twin agree byte for byte: a bin index is one IEEE division and one floor, everything after it is an integer.
#pragma once
#pragma clang fp contract(off)

#include "ba_mcl.hpp"

#include "../../include/visfs_mcl_kld.h"

namespace mcl {

constexpr int kKldThreads = 1024;             // the one workgroup of k_mcl_kld_resample
constexpr int kKldWaves = kKldThreads / 64;
constexpr int32_t kKldMaxSlots = 2 * VISFS_MCL_KLD_MAX_PARTICLES;   // the table at its fullest: 32768 slots of 4 bytes, 128 KiB of LDS
constexpr int32_t kKldMaxBlocks = VISFS_MCL_KLD_MAX_PARTICLES / kThreads;   // workgroup totals of k_mcl_finish: at most 64
constexpr int32_t kKldEmpty = 0x7fffffff;     // a slot holds a draw index or this
constexpr uint64_t kKldDraw = 3;              // the draw of key(): the motion has 0 .. 2, the comb particle N with draw 0

// floor(v / size), clamped to [-2^24, 2^24]
__host__ __device__ inline int32_t bin_of(double v, double size) {
    const double q = ::floor(v / size);
    if (!(q < (double)VISFS_MCL_KLD_BIN_CLAMP)) return VISFS_MCL_KLD_BIN_CLAMP;
    if (!(q > -(double)VISFS_MCL_KLD_BIN_CLAMP)) return -VISFS_MCL_KLD_BIN_CLAMP;
    return (int32_t)q;
}

// What chooses a bin's home slot; bins are compared as triples, so it decides no result.
__host__ __device__ inline uint64_t bin_hash(int32_t bx, int32_t by, int32_t bz) {
    const uint64_t h = pnp::mix64(((uint64_t)(uint32_t)bx << 32) | (uint64_t)(uint32_t)by);
    return pnp::mix64(h + kGold * ((uint64_t)(uint32_t)bz + 1));
}

// What a KLD update downloads: k_mcl_finish writes r, k_mcl_kld_resample the rest (only when it resamples).
struct KldRec {
    Rec r;
    int32_t n_after, bins, limit, pad;
};

// What k_mcl_kld_resample is told beside the update's header.
struct KldArgs {
    double bin_xy, bin_yaw;
    const int32_t* limit;                     // [cap + 1]
    int32_t* work;                            // [5 cap]: the draws' ancestors, their slots, their bins [cap][3]
    int32_t cap, slots, home_mask, pad;       // slots: a power of two, at least 2 cap; home_mask: what of the hash chooses the home slot
};

// ---------------------------------------------------------------- host only

inline int32_t kld_slots(int32_t cap) { return pow2_at_least(2 * cap); }

// limit[0 .. cap]; every line is one rounding, in this order.
inline void kld_limits(const visfs_mcl_kld_params& p, int32_t cap, std::vector<int32_t>& limit) {
    limit.assign((size_t)cap + 1, cap);
    for (int32_t k = 2; k <= cap; ++k) {
        const double km1 = (double)(k - 1);
        const double b = 2.0 / (9.0 * km1);
        const double c = std::sqrt(b) * p.kld_z;
        const double x = 1.0 - b + c;
        const double v = std::ceil(km1 / (2.0 * p.kld_err) * x * x * x);
        double l = v;
        if (!(l >= (double)p.min_particles)) l = (double)p.min_particles;
        if (!(l <= (double)cap)) l = (double)cap;
        limit[(size_t)k] = (int32_t)l;
    }
}

}  // namespace mcl
