// The laser pretreatment with its voxel filters (include/visfs_scan_filter.h): the definition, written once.
// k_scan_filter of ba_scan_filter.hip and the one-core twin both call what is here: the classification of a point
// (Estimator::laserPretreatment, as scan::pretreat of ba_scan.hpp states it), the voxel of a point, the range cut of the match
// cloud and the adaptive search of Cartographer 1.0's AdaptivelyVoxelFiltered, restated in double.  fp64, + - * / sqrt and round
// only, built without contraction; the kept set of a voxel filter ("the lowest index of each voxel") is a property of the data,
// so a schedule cannot change it.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/visfs_scan_filter.h"

#pragma clang fp contract(off)

namespace sfilt {

constexpr int kThreads = 1024;                // one workgroup per scan
constexpr int kWaves = kThreads / 64;
constexpr int32_t kMaxPoints = VISFS_SCAN_FILTER_MAX_POINTS;
constexpr int32_t kMaxSlots = 2 * kMaxPoints; // the table at its fullest: 32768 slots of 4 bytes, 128 KiB of LDS
constexpr int32_t kMinSlots = 16;
constexpr int32_t kEmpty = 0x7fffffff;        // a slot holds a point index or this
constexpr int32_t kMaxSub = VISFS_SCAN_FILTER_MAX_SUBDIVISIONS;
constexpr int32_t kMaxTrace = VISFS_SCAN_FILTER_MAX_TRACE;

// one byte per input point: bits 0-1 the class, bit 2 kept by the fixed filter, bits 3-6 the subdivision
constexpr uint8_t kClassMask = 3, kKept = 4, kListMask = 0x7b;
constexpr int kSubShift = 3;

// One scan of the upload block: offsets are bytes into the upload, download and work blocks.
struct ScanHdr {
    double T[12];
    double origin[3];
    int32_t n, pad;
    int64_t in_pts;                           // upload:   [n][3] raw points
    int64_t out_rm, out_match, out_hook;      // download: [n][3] returns then misses, [n][3] match cloud, [n] bytes
    int64_t work_pts, work_keys;              // work:     [n][3] doubles, [n] keys
};

// What a scan's workgroup leaves at the head of the download block.
struct DevRec {
    int32_t status, n_returns, n_misses, n_in_range, n_match, passes, pad0, pad1;
    double match_length;
    double origin[3];                         // T * origin
    double trace_length[kMaxTrace];
    int32_t trace_count[kMaxTrace];
    int32_t off_ret[kMaxSub], off_mis[kMaxSub];   // returns / misses kept before the first point of a non-empty subdivision
};

// Isometry3d * Vector3d in the order of scan::transform_xyz
__host__ __device__ inline void transform_xyz(const double T[12], const double p[3], double o[3]) {
    for (int r = 0; r < 3; ++r) o[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3];
}

// The class of the transformed point q seen from the transformed origin o, and the point it becomes (Estimator.cpp:137-152).
__host__ __device__ inline int classify(const visfs_scan_pretreat_params& p, const double o[3], const double q[3], double out[3]) {
    const double dx = q[0] - o[0], dy = q[1] - o[1], dz = q[2] - o[2];
    const double range = ::sqrt((dx * dx + dy * dy) + dz * dz);
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    if (!(range >= p.min_range)) return VISFS_SCAN_FILTER_DROPPED;
    if (range <= p.max_range) return VISFS_SCAN_FILTER_RETURN;
    const double f = p.missing_ray_length / range;
    out[0] = o[0] + f * dx; out[1] = o[1] + f * dy; out[2] = o[2] + f * dz;
    return VISFS_SCAN_FILTER_MISS;
}

// First point of subdivision s of n points split S ways (Estimator.cpp:124-126); n s <= 16384 * 16.
__host__ __device__ inline int32_t sub_begin(int32_t n, int32_t S, int32_t s) { return n * s / S; }

// The subdivision point i falls into: the largest s with sub_begin(s) <= i, i.e. with s < (i + 1) S / n.
__host__ __device__ inline int32_t sub_of(int32_t n, int32_t S, int32_t i) { return ((i + 1) * S - 1) / n; }

// The voxel of p at length len as three 21-bit fields; false when a component leaves +-(2^20 - 1) (a NaN does).
__host__ __device__ inline bool voxel_key(const double p[3], double len, uint64_t& key) {
    bool ok = true;
    key = 0;
    for (int c = 0; c < 3; ++c) {
        const double r = ::round(p[c] / len);
        if (!(::fabs(r) <= (double)VISFS_SCAN_FILTER_MAX_VOXEL)) ok = false;
        else key |= (uint64_t)((int64_t)r + 1048576) << (21 * c);
    }
    return ok;
}

__host__ __device__ inline int32_t table_slots(int32_t count) {
    int32_t s = kMinSlots;
    while (s < 2 * count) s <<= 1;
    return s;
}

// Where the probing of a key starts: a 64-bit finaliser over the key and the list it belongs to.
__host__ __device__ inline uint32_t hash_slot(uint64_t key, int32_t list, int32_t slots) {
    uint64_t k = key + (uint64_t)list * 0x9e3779b97f4a7c15ull;
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (uint32_t)k & (uint32_t)(slots - 1);
}

// The norm in the robot frame, not the range from the origin.
__host__ __device__ inline bool in_range(const double p[3], double max_range) {
    return ::sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) <= max_range;
}

// AdaptivelyVoxelFiltered: count(length) is the size of the cloud filtered at `length` (negative: a voxel out of range, the search
// ends at once with -1).  Returns the length the result is filtered at, 0: the cloud unchanged.  At most 1 + 7 + 4 counts.
template <class Count>
__host__ __device__ inline double adaptive_search(double max_length, int32_t min_num_points, int32_t n, Count&& count) {
    if (n <= min_num_points) return 0.0;
    int32_t c = count(max_length);
    if (c < 0) return -1.0;
    if (c >= min_num_points) return max_length;
    double result = max_length;
    for (double high = max_length; high > 1e-2 * max_length; high /= 2.0) {
        double low = high / 2.0;
        c = count(low);
        if (c < 0) return -1.0;
        result = low;
        if (c >= min_num_points) {
            while ((high - low) / low > 1e-1) {
                const double mid = (low + high) / 2.0;
                c = count(mid);
                if (c < 0) return -1.0;
                if (c >= min_num_points) { low = mid; result = mid; }
                else high = mid;
            }
            return result;
        }
    }
    return result;
}

}  // namespace sfilt
