// ResidentTracker.h — VISFS::Tracker::pretreatment + VISFS::Tracker::imageProcess (corelib/src/Tracker.cpp:143-419) as one call
// on the GPU-resident word table of include/visfs_tracker.h.  Header only, over the C ABI.
//
// What the reference keeps in trackCnt_, globalFeatureId_, the words of lastSignature_ and the blocked words of pretreatment lives
// in the library; this class turns the arrays of a call into the std::maps the Signature setters take (ascending id, as uKeys and
// uValues read them) and keeps the one test that belongs to the caller's types: getDeltaPoseGuess().isApprox(Identity) (:237).
//
// enablePnP() puts VISFS::estimateMotion3DTo2D (MultiviewGeometry.cpp:94-216) into the same call (include/visfs_tracker_pnp.h):
// poseGuess() then hands out the transform, the covariance and the match and inlier ids of the last imageProcess, with the row
// numbers turned into ids as MotionEstimator.h does.
//
// VISFS::ResidentTrackerGroup runs the imageProcess of several ResidentTrackers (a rig's cameras) in one call of
// include/visfs_tracker_group.h.
#ifndef VISFS_AMD_RESIDENT_TRACKER_H
#define VISFS_AMD_RESIDENT_TRACKER_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "visfs_tracker.h"
#include "visfs_tracker_group.h"
#include "visfs_tracker_pnp.h"

namespace VISFS {

class ResidentTracker {
public:
    struct Point2f { float x, y; };
    struct Point3f { float x, y, z; };

    // The contents imageProcess sets on the to-signature (and setBlockedWords on the from-signature).
    struct Frame {
        bool noPrevious = false, bootstrapped = false, lost = false;
        std::map<std::size_t, Point2f> covisibleWords;              // setCovisibleWords
        std::map<std::size_t, Point3f> covisibleWords3d;            // setCovisibleWords3d
        std::map<std::size_t, Point2f> keyPointsMatchesFormer;      // setkeyPointsMatchesFormer
        std::map<std::size_t, Point2f> keyPointsNewExtract;         // setKeyPointsNewExtract
        std::map<std::size_t, Point2f> words;                       // setWords
        std::map<std::size_t, Point2f> keyPointMatchesImageRight;   // setKeyPointMatchesImageRight
        std::map<std::size_t, Point3f> words3d;                     // setWords3d
        std::map<std::size_t, int> trackCount;                      // trackCnt_ after updateTrackCounter
        std::set<std::size_t> blockedWords;                         // keys of setBlockedWords
        std::size_t nextFeatureId = 0;                              // globalFeatureId_
    };

    // What estimateMotion3DTo2D returns: `transform` all zero is the reference's null transform (Estimator.cpp:209).
    struct PoseGuess {
        bool ran = false;                                           // false: enablePnP() is not in force, or the frame had no previous one
        std::array<double, 16> transform{};                         // 4 x 4 row-major
        std::array<double, 36> covariance{};                        // 6 x 6 row-major
        std::vector<std::size_t> matches, inliers;                  // word ids
    };

    ResidentTracker(const ResidentTracker&) = delete;
    ResidentTracker& operator=(const ResidentTracker&) = delete;

    // flow: the object that holds the pyramids (visfs_flow_create, or visfs_flow_create_host for the one-core twin); it must outlive
    // this tracker.  The Tracker/* and Estimator/MinInliers keys as the reference names them.  cullByFundationMatrix
    // (Tracker/CullByFundationMatrix, with Tracker/FundationPixelError) takes effect, as in the reference, only on a flow object whose
    // flow_back is off (Tracker.cpp:275); cullIterations and cullSeed are the two keys the search has on top (visfs_fund.h).
    ResidentTracker(visfs_flow* flow, const visfs_flow_camera& camera, int maxFeatures = 300, double qualityLevel = 0.01,
                    int minFeatureDistance = 40, int minInliers = 10, bool clahe = false, double clipLimit = 3.0, int tilesX = 8,
                    int tilesY = 8, bool cullByFundationMatrix = false, float fundationPixelError = 1.0f, int cullIterations = 1000,
                    uint64_t cullSeed = 0) {
        visfs_tracker_params p;
        visfs_tracker_default_params(&p);
        p.max_features = maxFeatures; p.quality_level = qualityLevel; p.min_distance = minFeatureDistance; p.min_inliers = minInliers;
        p.clahe = clahe ? 1 : 0; p.clahe_params.clip_limit = clipLimit; p.clahe_params.tiles_x = tilesX; p.clahe_params.tiles_y = tilesY;
        p.cull = cullByFundationMatrix ? 1 : 0; p.cull_params.pixel_error = fundationPixelError; p.cull_params.iterations = cullIterations;
        p.cull_params.seed = cullSeed;
        const int rc = visfs_tracker_create(flow, &p, &camera, &t_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_tracker_create failed with status " + std::to_string(rc));
    }
    ~ResidentTracker() { visfs_tracker_destroy(t_); }

    // Tracker::pretreatment (:143-165): the outliers Estimator::getOutliers() returned leave the table in the next imageProcess.
    void pretreatment(const std::set<std::size_t>& outliers) { outliers_.assign(outliers.begin(), outliers.end()); }

    // Eigen's isApprox against the identity (:237): ||T - I||^2 <= 1e-24 * min(||T||^2, ||I||^2) over the 4 x 4 matrix.
    static bool isIdentity(const double T[16]) {
        double diff = 0.0, norm = 0.0;
        for (int i = 0; i < 16; ++i) {
            const double e = (i % 5 == 0) ? 1.0 : 0.0;
            diff += (T[i] - e) * (T[i] - e);
            norm += T[i] * T[i];
        }
        return diff <= 1e-24 * (norm < 4.0 ? norm : 4.0);
    }

    // Tracker::imageProcess (:167-419) on a new stereo pair (8-bit grey).  deltaPoseGuess: getDeltaPoseGuess() as a 4 x 4 row-major
    // matrix, or nullptr; an identity-equal guess is "not set", as in the reference.
    int imageProcess(const uint8_t* left, const uint8_t* right, int stride, const double* deltaPoseGuess, Frame& out) {
        const bool guessSet = deltaPoseGuess != nullptr && !isIdentity(deltaPoseGuess);
        std::vector<uint64_t> ids(outliers_.begin(), outliers_.end());
        outliers_.clear();
        visfs_tracker_result r;
        const int rc = visfs_tracker_process(t_, left, right, stride, guessSet ? deltaPoseGuess : nullptr, (int32_t)ids.size(),
                                             ids.empty() ? nullptr : ids.data(), &r);
        out = Frame();
        if (rc != VISFS_BA_OK) return rc;
        fill(r, out);
        remember(r);
        return rc;
    }

    // Estimator/MinInliers, Estimator/PnPIterations, Estimator/PnPReprojError and Estimator/RefineIterations as the reference names
    // them: from the next imageProcess on the pose guess runs inside it.  Call it before the tracker joins a ResidentTrackerGroup,
    // with the same values on every member.
    void enablePnP(int minInliers = 12, int iterations = 50, double reProjError = 2.0, int refineIterations = 5, uint64_t seed = 0) {
        visfs_pnp_params p;
        visfs_pnp_default_params(&p);
        p.min_inliers = minInliers; p.iterations = iterations; p.reproj_error = (float)reProjError; p.refine_iterations = refineIterations;
        p.seed = seed;
        const int rc = visfs_tracker_enable_pnp(t_, &p);
        if (rc != VISFS_BA_OK)
            throw std::runtime_error("visfs_tracker_enable_pnp failed with status " + std::to_string(rc) + ": " + visfs_tracker_last_error(t_));
    }
    int disablePnP() { return visfs_tracker_enable_pnp(t_, nullptr); }

    // The pose guess of the last imageProcess (of this tracker or of its group).  Nothing is issued to the device.
    int poseGuess(PoseGuess& out) const {
        out = PoseGuess();
        visfs_tracker_pnp_result r;
        const int rc = visfs_tracker_pnp_last(t_, &r);
        if (rc != VISFS_BA_OK) return rc;
        out.ran = r.ran != 0;
        for (int i = 0; i < 16; ++i) out.transform[(std::size_t)i] = r.T[i];
        for (int i = 0; i < 36; ++i) out.covariance[(std::size_t)i] = r.cov[i];
        for (int32_t i = 0; i < r.n_matches; ++i) out.matches.push_back(covisibleIds_.at((std::size_t)r.matches[i]));
        for (int32_t i = 0; i < r.n_inliers; ++i) out.inliers.push_back(covisibleIds_.at((std::size_t)r.inliers[i]));
        return rc;
    }

    int reset() { return visfs_tracker_reset(t_); }
    const char* lastError() const { return visfs_tracker_last_error(t_); }
    visfs_tracker* handle() { return t_; }

private:
    friend class ResidentTrackerGroup;
    // the arrays of a call as the maps the Signature setters take
    static void fill(const visfs_tracker_result& r, Frame& out) {
        out.noPrevious = (r.flags & VISFS_TRACKER_NO_PREVIOUS) != 0;
        out.bootstrapped = (r.flags & VISFS_TRACKER_BOOTSTRAPPED) != 0;
        out.lost = (r.flags & VISFS_TRACKER_LOST) != 0;
        out.nextFeatureId = (std::size_t)r.next_id;
        for (int32_t i = 0; i < r.n_covisible; ++i) {
            const std::size_t id = (std::size_t)r.covisible_id[i];
            out.covisibleWords.emplace_hint(out.covisibleWords.end(), id, p2(r.covisible_from_xy, i));
            out.covisibleWords3d.emplace_hint(out.covisibleWords3d.end(), id, p3(r.covisible_from_xyz, i));
            out.keyPointsMatchesFormer.emplace_hint(out.keyPointsMatchesFormer.end(), id, p2(r.covisible_to_xy, i));
        }
        for (int32_t i = 0; i < r.n_new; ++i)
            out.keyPointsNewExtract.emplace_hint(out.keyPointsNewExtract.end(), (std::size_t)r.new_id[i], p2(r.new_xy, i));
        for (int32_t i = 0; i < r.n_words; ++i) {
            const std::size_t id = (std::size_t)r.word_id[i];
            out.words.emplace_hint(out.words.end(), id, p2(r.word_left_xy, i));
            out.keyPointMatchesImageRight.emplace_hint(out.keyPointMatchesImageRight.end(), id, p2(r.word_right_xy, i));
            out.words3d.emplace_hint(out.words3d.end(), id, p3(r.word_xyz, i));
            out.trackCount.emplace_hint(out.trackCount.end(), id, (int)r.word_count[i]);
        }
        for (int32_t i = 0; i < r.n_blocked; ++i) out.blockedWords.insert(out.blockedWords.end(), (std::size_t)r.blocked_id[i]);
    }
    void remember(const visfs_tracker_result& r) {                  // the ids poseGuess() turns row numbers into
        covisibleIds_.assign(r.covisible_id, r.covisible_id + r.n_covisible);
    }
    static Point2f p2(const float* a, int32_t i) { return Point2f{ a[2 * i], a[2 * i + 1] }; }
    static Point3f p3(const float* a, int32_t i) { return Point3f{ a[3 * i], a[3 * i + 1], a[3 * i + 2] }; }
    visfs_tracker* t_ = nullptr;
    std::vector<std::size_t> outliers_;
    std::vector<std::size_t> covisibleIds_;
};

// Tracker::imageProcess of every camera of a rig in one call.  The members are ResidentTrackers on flow objects of their own (all of
// one handle, or all host twins) with equal keys (cullByFundationMatrix and fundationPixelError among them: the cull of every member
// runs inside the one call; enablePnP and its values too: a group takes its members' setting) and image size; they must outlive the group and stay usable on their own.
class ResidentTrackerGroup {
public:
    struct Input {
        const uint8_t* left; const uint8_t* right; int stride;
        const double* deltaPoseGuess;                                  // 4 x 4 row-major or nullptr, as ResidentTracker::imageProcess takes it
    };

    ResidentTrackerGroup(const ResidentTrackerGroup&) = delete;
    ResidentTrackerGroup& operator=(const ResidentTrackerGroup&) = delete;

    explicit ResidentTrackerGroup(const std::vector<ResidentTracker*>& members) : members_(members) {
        std::vector<visfs_tracker*> h;
        for (ResidentTracker* m : members_) h.push_back(m->t_);
        const int rc = visfs_tracker_group_create((int32_t)h.size(), h.data(), &g_);
        if (rc != VISFS_BA_OK)
            throw std::runtime_error("visfs_tracker_group_create failed with status " + std::to_string(rc) + ": " + visfs_tracker_group_last_error(nullptr));
    }
    ~ResidentTrackerGroup() { visfs_tracker_group_destroy(g_); }

    // Each member's pretreatment() outliers go in and are used up, as in its own imageProcess.  out[i] is member i's Frame.
    int imageProcess(const std::vector<Input>& in, std::vector<ResidentTracker::Frame>& out) {
        const std::size_t n = members_.size();
        if (in.size() != n) return VISFS_BA_ERR_BAD_ARGUMENT;
        std::vector<std::vector<uint64_t>> ids(n);
        std::vector<visfs_tracker_frame> fr(n);
        std::vector<visfs_tracker_result> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            ids[i].assign(members_[i]->outliers_.begin(), members_[i]->outliers_.end());
            const bool guessSet = in[i].deltaPoseGuess != nullptr && !ResidentTracker::isIdentity(in[i].deltaPoseGuess);
            fr[i].left = in[i].left; fr[i].right = in[i].right; fr[i].stride = in[i].stride;
            fr[i].delta_guess = guessSet ? in[i].deltaPoseGuess : nullptr;
            fr[i].n_outliers = (int32_t)ids[i].size();
            fr[i].outlier_ids = ids[i].empty() ? nullptr : ids[i].data();
        }
        const int rc = visfs_tracker_group_process(g_, fr.data(), res.data());
        out.assign(n, ResidentTracker::Frame());
        if (rc != VISFS_BA_OK) return rc;                              // nothing was pushed: the outliers stay for the next call
        for (std::size_t i = 0; i < n; ++i) {
            members_[i]->outliers_.clear();
            ResidentTracker::fill(res[i], out[i]);
            members_[i]->remember(res[i]);
        }
        return rc;
    }

    // what the last imageProcess issued on the device (all zero for host twins)
    void lastCounts(int& kernelLaunches, int& copiesAndMemsets, int& synchronisations) const {
        int32_t k = 0, c = 0, s = 0;
        visfs_tracker_group_last_counts(g_, &k, &c, &s);
        kernelLaunches = k; copiesAndMemsets = c; synchronisations = s;
    }
    const char* lastError() const { return visfs_tracker_group_last_error(g_); }
    std::size_t size() const { return members_.size(); }

private:
    std::vector<ResidentTracker*> members_;
    visfs_tracker_group* g_ = nullptr;
};

}  // namespace VISFS

#endif
