// EpipolarCull.h — VISFS::rejectOutlierWithFundationMatrix (corelib/src/Tracker.cpp:83-96) over the C ABI of include/visfs_fund.h.
// Header only.
//
// The function keeps the reference's argument order: cornersFrom, cornersTo and the Lucas-Kanade status, which it ANDs with the
// RANSAC mask of the fundamental matrix in place.  imageProcess runs it when Tracker/FlowBack is off and
// Tracker/CullByFundationMatrix is on (:275-277), between the forward LK pass (FlowTracker::track with flowBack = false) and the
// compaction of :285-301.  cv::Point2f is replaced by any struct of two floats x, y (FlowTracker::Point2f is one).  Every hypothesis
// is evaluated, so the reference's confidence 0.99 has no counterpart.
#ifndef VISFS_AMD_EPIPOLAR_CULL_H
#define VISFS_AMD_EPIPOLAR_CULL_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "visfs_fund.h"

namespace VISFS {

using FundamentalMatrix = std::array<double, 9>;     // row-major, x_to^T F x_from = 0; all zero without a model

// Owns a visfs_fund for up to `capacity` corners on the device and stream of `ba`.
class EpipolarCull {
public:
    EpipolarCull(const EpipolarCull&) = delete;
    EpipolarCull& operator=(const EpipolarCull&) = delete;
    explicit EpipolarCull(visfs_ba_handle* ba, int capacity = VISFS_FUND_MAX_POINTS) {
        const int rc = visfs_fund_create(ba, capacity, &p_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_fund_create failed with status " + std::to_string(rc));
    }
    ~EpipolarCull() { visfs_fund_destroy(p_); }
    visfs_fund* get() const { return p_; }
    const char* lastError() const { return visfs_fund_last_error(p_); }

private:
    visfs_fund* p_ = nullptr;
};

// Returns the number of rows the fundamental matrix keeps (the ones of its mask), or -1 when fewer than seven corners with finite
// coordinates were given and the status is left as it was (OpenCV returns an empty matrix there; the reference then reads an empty
// mask).
template <class Point2f>
inline int rejectOutlierWithFundationMatrix(visfs_fund* fund, const std::vector<Point2f>& cornersFrom, const std::vector<Point2f>& cornersTo,
                                            std::vector<unsigned char>& status, float fundationPixelError = 1.0f,
                                            FundamentalMatrix* F = nullptr, int iterations = 1000, std::uint64_t seed = 0) {
    static_assert(sizeof(Point2f) == 2 * sizeof(float), "a corner is two floats");
    if (cornersFrom.size() != cornersTo.size() || status.size() != cornersFrom.size())
        throw std::invalid_argument("cornersFrom, cornersTo and status must have one size");
    visfs_fund_params prm;
    visfs_fund_default_params(&prm);
    prm.pixel_error = fundationPixelError; prm.iterations = iterations; prm.seed = seed;
    const std::int32_t n = (std::int32_t)cornersFrom.size();
    std::vector<std::uint8_t> mask((std::size_t)n + 1);
    std::int32_t nInliers = 0, applied = 0;
    FundamentalMatrix f{};
    const int rc = visfs_fund_cull(fund, &prm, n, n ? &cornersFrom[0].x : nullptr, n ? &cornersTo[0].x : nullptr, status.data(), status.data(),
                                   mask.data(), f.data(), &nInliers, &applied);
    if (rc != VISFS_BA_OK)
        throw std::runtime_error("visfs_fund_cull failed with status " + std::to_string(rc) + ": " + visfs_fund_last_error(fund));
    if (F) *F = f;
    return applied ? (int)nInliers : -1;
}

}  // namespace VISFS

#endif
