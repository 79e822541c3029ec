// FlowTracker.h — the pixel half of VISFS::Tracker::imageProcess (corelib/src/Tracker.cpp:233-274, :343-388) backed by the
// GPU-resident image pyramids of include/visfs_flow.h.  Header only, over the C ABI.
//
// It keeps what imageProcess does with pixels, and the equalisation System::inputPrimarySensorData runs in front of it when
// System/CLAHE is set (System.cpp:107-111, include/visfs_clahe.h): the two cv::goodFeaturesToTrack calls behind the mask of getMask (:116-141, :181, :327,
// include/visfs_corners.h), the four cv::calcOpticalFlowPyrLK passes of a frame with their forward-backward gates and
// generateKeyPoints3DStereo.  The bounds test and the compaction of the surviving words stay with the caller, as in the reference
// they surround these calls.  The fundamental-matrix cull (flowBack off) is EpipolarCull.h, the PnP guess MotionEstimator.h.
#ifndef VISFS_AMD_FLOW_TRACKER_H
#define VISFS_AMD_FLOW_TRACKER_H

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "visfs_clahe.h"
#include "visfs_corners.h"
#include "visfs_flow.h"

namespace VISFS {

class FlowTracker {
public:
    struct Point2f { float x, y; };
    struct Point3f { float x, y, z; };

    FlowTracker(const FlowTracker&) = delete;
    FlowTracker& operator=(const FlowTracker&) = delete;

    // ba: the handle whose device and stream the pyramids live on; the Tracker/* keys as the reference names them.
    FlowTracker(visfs_ba_handle* ba, int width, int height, int flowWinSize = 21, int flowMaxLevel = 3, int flowIterations = 30,
                float flowEps = 0.01f, bool flowBack = true, float minDepth = 0.2f, float maxDepth = 10.0f) {
        visfs_flow_params p;
        visfs_flow_default_params(&p);
        p.win_size = flowWinSize; p.max_level = flowMaxLevel; p.iterations = flowIterations; p.eps = flowEps;
        p.flow_back = flowBack ? 1 : 0; p.min_depth = minDepth; p.max_depth = maxDepth;
        const int rc = visfs_flow_create(ba, &p, width, height, &f_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_flow_create failed with status " + std::to_string(rc));
    }
    ~FlowTracker() { visfs_flow_destroy(f_); }

    // A new stereo pair (8-bit grey, `stride` bytes per row); the pair pushed before becomes imageFrom.
    int pushFrame(const uint8_t* left, const uint8_t* right, int stride) { return visfs_flow_push_frame(f_, left, right, stride); }

    // pushFrame with System/CLAHE set: cv::createCLAHE(clipLimit, cv::Size(tilesX, tilesY))->apply on both images first
    // (System.cpp:107-111), on the device; the buffers of the caller are not written.
    int pushFrameCLAHE(const uint8_t* left, const uint8_t* right, int stride, double clipLimit = 3.0, int tilesX = 8, int tilesY = 8) {
        visfs_clahe_params p;
        visfs_clahe_default_params(&p);
        p.clip_limit = clipLimit; p.tiles_x = tilesX; p.tiles_y = tilesY;
        return visfs_flow_push_frame_clahe(f_, &p, left, right, stride);
    }

    // Tracker.cpp:257-274: cornersFrom -> cornersTo (cornersTo non-empty on entry: OPTFLOW_USE_INITIAL_FLOW), status after the gate.
    int track(const std::vector<Point2f>& cornersFrom, std::vector<Point2f>& cornersTo, std::vector<unsigned char>& status,
              std::vector<float>* err = nullptr) {
        const bool guess = cornersTo.size() == cornersFrom.size() && !cornersFrom.empty();
        std::vector<Point2f> init;
        if (guess) init = cornersTo;
        cornersTo.resize(cornersFrom.size());
        status.resize(cornersFrom.size());
        if (err) err->resize(cornersFrom.size());
        return visfs_flow_track(f_, (int32_t)cornersFrom.size(), flat(cornersFrom), guess ? flat(init) : nullptr, flat(cornersTo),
                                status.data(), err ? err->data() : nullptr);
    }

    // Tracker.cpp:354-371 + generateKeyPoints3DStereo (:388): cornersLeft -> cornersRight, status after the gate, kpts3D (robot frame,
    // NaN where the reference leaves badPoint or the point was dropped).
    int stereo(const std::vector<Point2f>& cornersLeft, const visfs_flow_camera& camera, std::vector<Point2f>& cornersRight,
               std::vector<unsigned char>& status, std::vector<Point3f>& kpts3D) {
        cornersRight.resize(cornersLeft.size());
        status.resize(cornersLeft.size());
        kpts3D.resize(cornersLeft.size());
        return visfs_flow_stereo(f_, (int32_t)cornersLeft.size(), flat(cornersLeft), &camera, flat(cornersRight), status.data(),
                                 kpts3D.empty() ? nullptr : &kpts3D[0].x);
    }

    // cv::goodFeaturesToTrack(image, out, maxCorners, qualityLevel, minDistance, mask) on the resident left image of the newest pair
    // (previous: of the pair before it), the mask given as the discs of maskDiscs.  Strongest first.
    int corners(std::vector<Point2f>& out, int maxCorners, double qualityLevel, double minDistance,
                const std::vector<visfs_corners_disc>& discs = {}, bool previous = false) {
        visfs_corners_params p;
        visfs_corners_default_params(&p);
        p.max_corners = maxCorners; p.quality_level = qualityLevel; p.min_distance = minDistance;
        out.resize((size_t)std::min(std::max(maxCorners, 0), VISFS_CORNERS_MAX_CORNERS));    // beyond it the library refuses
        int32_t n = 0;
        Point2f none{ 0.0f, 0.0f };
        const int rc = visfs_flow_corners(f_, previous ? VISFS_FLOW_SLOT_PREVIOUS : VISFS_FLOW_SLOT_CURRENT, VISFS_FLOW_IMAGE_LEFT, &p,
                                          (int32_t)discs.size(), discs.empty() ? nullptr : discs.data(), (int32_t)out.size(),
                                          out.empty() ? &none.x : &out[0].x, &n);
        out.resize(rc == VISFS_BA_OK ? (size_t)n : 0);
        return rc;
    }

    // The disc list of Tracker::getMask (Tracker.cpp:116-141): the tracked points by track count descending at radius minDistance,
    // then the blocked points at radius minDistance / 2 (integer division, as the reference writes it).  The reference's std::sort
    // (:126) leaves the order among equal counts open; this helper uses std::stable_sort, so equal counts keep the order given.
    static std::vector<visfs_corners_disc> maskDiscs(const std::vector<std::pair<int, Point2f>>& trackCountAndPoint,
                                                     const std::vector<Point2f>& blocked, int minDistance) {
        std::vector<std::pair<int, Point2f>> sorted = trackCountAndPoint;
        std::stable_sort(sorted.begin(), sorted.end(),
                         [](const std::pair<int, Point2f>& a, const std::pair<int, Point2f>& b) { return a.first > b.first; });
        std::vector<visfs_corners_disc> discs;
        discs.reserve(sorted.size() + blocked.size());
        for (const auto& cp : sorted) discs.push_back(visfs_corners_disc{ cp.second.x, cp.second.y, minDistance });
        for (const Point2f& b : blocked) discs.push_back(visfs_corners_disc{ b.x, b.y, minDistance / 2 });
        return discs;
    }

    const char* lastError() const { return visfs_flow_last_error(f_); }

private:
    static const float* flat(const std::vector<Point2f>& v) { return v.empty() ? nullptr : &v[0].x; }
    static float* flat(std::vector<Point2f>& v) { return v.empty() ? nullptr : &v[0].x; }
    visfs_flow* f_ = nullptr;
};

}  // namespace VISFS

#endif
