// MotionEstimator.h — VISFS::estimateMotion3DTo2D (corelib/src/MultiviewGeometry.cpp:94-216) over the C ABI of
// include/visfs_pnp.h.  Header only.
//
// The function keeps the reference's argument order over std::map<std::size_t, ...>; it does the id matching of :113-129 (the ids of
// words2dTo in ascending order, kept when words3dFrom holds the id) and hands rows to visfs_pnp_solve, which drops the rows whose 3-D
// word is not finite and runs the RANSAC search, the refit and the refinement loop on the device of the solver.  OpenCV and Eigen
// types are replaced by plain ones: a point is three floats, a key-point carries its `pt`, a transform is a 4x4 row-major array and
// the camera is the visfs_pnp_camera (cvKdouble() and getTansformImageToRobot()).  flagPnP is accepted and not used (one generator,
// P3P, and one iterative refit: DESIGN.md section 9e); so is the guess, which the reference computes and then passes with
// useExtrinsicGuess = false (:145).
#ifndef VISFS_AMD_MOTION_ESTIMATOR_H
#define VISFS_AMD_MOTION_ESTIMATOR_H

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "visfs_pnp.h"

namespace VISFS {

struct PnpPoint2f { float x, y; };
struct PnpPoint3f { float x, y, z; };
struct PnpKeyPoint { PnpPoint2f pt; };
using PnpTransform = std::array<double, 16>;        // 4x4 row-major; all zero: the reference's null transform (Estimator.cpp:209)
using PnpCovariance = std::array<double, 36>;       // 6x6 row-major

// Owns a visfs_pnp for up to `capacity` correspondences on the device and stream of `ba`.
class MotionEstimator {
public:
    MotionEstimator(const MotionEstimator&) = delete;
    MotionEstimator& operator=(const MotionEstimator&) = delete;
    explicit MotionEstimator(visfs_ba_handle* ba, int capacity = VISFS_PNP_MAX_POINTS) {
        const int rc = visfs_pnp_create(ba, capacity, &p_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_pnp_create failed with status " + std::to_string(rc));
    }
    ~MotionEstimator() { visfs_pnp_destroy(p_); }
    visfs_pnp* get() const { return p_; }
    const char* lastError() const { return visfs_pnp_last_error(p_); }

private:
    visfs_pnp* p_ = nullptr;
};

inline PnpTransform estimateMotion3DTo2D(
    visfs_pnp* solver,
    const std::map<std::size_t, PnpPoint3f>& words3dFrom,
    const std::map<std::size_t, PnpKeyPoint>& words2dTo,
    const visfs_pnp_camera& cameraModel,
    int minInliers,
    int iterations,
    double reProjError,
    int /*flagPnP*/,
    int refineIterations,
    const std::map<std::size_t, PnpPoint3f>& words3dTo,
    PnpCovariance& covariance,
    std::vector<std::size_t>& matchesOut,
    std::vector<std::size_t>& inliersOut,
    const PnpTransform* /*guess*/ = nullptr,
    std::uint64_t seed = 0) {
    std::vector<std::size_t> ids;
    std::vector<float> from, to2d, to3d;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (const auto& kv : words2dTo) {                                           // uKeys(_words2dTo): ascending
        const auto it = words3dFrom.find(kv.first);
        if (it == words3dFrom.end()) continue;
        ids.push_back(kv.first);
        from.insert(from.end(), { it->second.x, it->second.y, it->second.z });
        to2d.insert(to2d.end(), { kv.second.pt.x, kv.second.pt.y });
        if (!words3dTo.empty()) {
            const auto jt = words3dTo.find(kv.first);
            if (jt != words3dTo.end()) to3d.insert(to3d.end(), { jt->second.x, jt->second.y, jt->second.z });
            else to3d.insert(to3d.end(), { nan, nan, nan });
        }
    }
    visfs_pnp_params prm;
    visfs_pnp_default_params(&prm);
    prm.min_inliers = minInliers; prm.iterations = iterations; prm.reproj_error = (float)reProjError;
    prm.refine_iterations = refineIterations; prm.seed = seed;
    const std::int32_t n = (std::int32_t)ids.size();
    std::vector<std::int32_t> matches((std::size_t)n + 1), inliers((std::size_t)n + 1);
    std::int32_t nMatches = 0, nInliers = 0;
    PnpTransform transform{};
    const int rc = visfs_pnp_solve(solver, &prm, &cameraModel, n, from.data(), to2d.data(), words3dTo.empty() ? nullptr : to3d.data(),
                                   transform.data(), covariance.data(), matches.data(), &nMatches, inliers.data(), &nInliers);
    if (rc != VISFS_BA_OK)
        throw std::runtime_error("visfs_pnp_solve failed with status " + std::to_string(rc) + ": " + visfs_pnp_last_error(solver));
    matchesOut.resize((std::size_t)nMatches);
    for (std::int32_t i = 0; i < nMatches; ++i) matchesOut[(std::size_t)i] = ids[(std::size_t)matches[(std::size_t)i]];
    inliersOut.resize((std::size_t)nInliers);
    for (std::int32_t i = 0; i < nInliers; ++i) inliersOut[(std::size_t)i] = ids[(std::size_t)inliers[(std::size_t)i]];
    return transform;
}

}  // namespace VISFS

#endif
