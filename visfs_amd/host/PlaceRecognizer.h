// PlaceRecognizer.h — visual place recognition beside VISFS::Tracker: what the reference's localisation launch files run rtabmap for
// (Kp/DetectorStrategy 8: GFTT corners with ORB descriptors, Kp/MaxFeatures 500, Mem/STMSize 30), over include/visfs_place.h.
// Header only, over the C ABI.
//
// The recognizer owns the key-frame store.  A flow object (a visfs_flow of the caller) is attached to it;
// describe() then works on that object's resident left image, addKeyFrame() appends what was described with the words' ids and 3-D
// points, and query() returns, per recognised key-frame, the from_xyz / to_xy rows visfs_pnp_solve takes.  queryVerify() runs the
// same query and verifies every candidate by PnP in the same call (include/visfs_place_verify.h), and closureEdge() turns a verified
// candidate into what a visfs_pose_graph_edge between the key-frame's vertex and the query's takes.  A lost tracker is
// replaced by a fresh one: attach() the new flow object and query.  detach() (or the destructor) must run before the attached flow
// object is destroyed.
#ifndef VISFS_AMD_PLACE_RECOGNIZER_H
#define VISFS_AMD_PLACE_RECOGNIZER_H

#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "visfs_place.h"
#include "visfs_place_verify.h"

namespace VISFS {

class PlaceRecognizer {
public:
    struct Point2f { float x, y; };
    struct Point3f { float x, y, z; };

    // One candidate of a query, unpacked: rows i of fromXyz / toXy are one correspondence.
    struct Candidate {
        int slot = -1;
        int64_t key = 0;
        std::vector<int32_t> ids, queryIndex, distance;
        std::vector<Point3f> fromXyz;
        std::vector<Point2f> toXy;
    };

    // One candidate of queryVerify(): the pose of the query in the frame of the key-frame (4 x 4 row-major, all zero: not verified), its
    // covariance (x y z roll pitch yaw) and inlier count, from the guided stage where it ran and from the PnP stage otherwise.
    struct Verified {
        int slot = -1;
        int64_t key = 0;
        bool guided = false;
        int rows = 0, inliers = 0;
        double T[16] = {}, cov[36] = {};
    };

    PlaceRecognizer(const PlaceRecognizer&) = delete;
    PlaceRecognizer& operator=(const PlaceRecognizer&) = delete;

    // ba: the handle whose device and stream the store lives on, or nullptr for the one-core twin (with host flow objects).
    explicit PlaceRecognizer(visfs_ba_handle* ba, int maxKeyFrames = 30, int maxFeatures = 500)
        : capacity_(std::min(std::max(maxFeatures, 1), VISFS_PLACE_MAX_POINTS)), result_(new visfs_place_result()),
          verify_(new visfs_place_verify_result()) {
        visfs_place_default_params(&params_);
        const int rc = visfs_place_db_create(ba, maxKeyFrames, &db_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_place_db_create failed with status " + std::to_string(rc));
        const int rv = visfs_place_verifier_create(db_, &verifier_);             // every buffer of queryVerify() is allocated here
        if (rv != VISFS_BA_OK) {
            visfs_place_db_destroy(db_);
            throw std::runtime_error("visfs_place_verifier_create failed with status " + std::to_string(rv));
        }
    }
    ~PlaceRecognizer() {
        detach();
        visfs_place_verifier_destroy(verifier_);
        visfs_place_db_destroy(db_);
    }

    int attach(visfs_flow* flow) {
        detach();
        return visfs_place_set_create(flow, capacity_, &set_);
    }
    void detach() {
        visfs_place_set_destroy(set_);
        set_ = nullptr;
    }

    visfs_place_params& params() { return params_; }

    // Descriptors of the key-points on the left image of the newest pair (previous: of the pair before it).  At most maxFeatures.
    int describe(const std::vector<Point2f>& keyPoints, bool previous = false) {
        if (!set_) return VISFS_BA_ERR_NOT_LOADED;
        return visfs_place_describe(set_, previous ? VISFS_FLOW_SLOT_PREVIOUS : VISFS_FLOW_SLOT_CURRENT, VISFS_FLOW_IMAGE_LEFT, (int32_t)keyPoints.size(),
                                    keyPoints.empty() ? nullptr : &keyPoints[0].x);
    }

    // What describe() left becomes the next key-frame: ids[i] and xyz[i] belong to key-point i.  Returns the status; *slot the slot taken.
    int addKeyFrame(const std::vector<int32_t>& ids, const std::vector<Point3f>& xyz, int64_t key, int* slot = nullptr) {
        if (!set_) return VISFS_BA_ERR_NOT_LOADED;
        int32_t n = 0;
        int rc = visfs_place_set_download(set_, &n, nullptr, nullptr, nullptr, nullptr);
        if (rc != VISFS_BA_OK) return rc;
        if ((size_t)n != ids.size() || (size_t)n != xyz.size()) return VISFS_BA_ERR_BAD_ARGUMENT;
        int32_t taken = -1;
        rc = visfs_place_db_add(db_, set_, ids.empty() ? nullptr : ids.data(), xyz.empty() ? nullptr : &xyz[0].x, key, &taken);
        if (slot) *slot = taken;
        return rc;
    }

    int keyFrames() const {
        int32_t n = 0;
        visfs_place_db_size(db_, &n);
        return n;
    }
    void reset() { visfs_place_db_reset(db_); }

    // What describe() left against the store.  counts: the accepted matches of every slot in range; candidates: best first.
    int query(std::vector<Candidate>& candidates, std::vector<int32_t>* counts = nullptr) {
        candidates.clear();
        if (!set_) return VISFS_BA_ERR_NOT_LOADED;
        const int rc = visfs_place_query(db_, set_, &params_, result_.get());
        if (rc != VISFS_BA_OK) return rc;
        const visfs_place_result& r = *result_;
        if (counts) counts->assign(r.count, r.count + r.n_slots);
        for (int c = 0; c < r.n_candidates; ++c) {
            Candidate k;
            k.slot = r.candidate[c].slot; k.key = r.candidate[c].key;
            for (int i = 0; i < r.candidate[c].count; ++i) {
                const visfs_place_row& row = r.row[c][i];
                k.ids.push_back(row.id); k.queryIndex.push_back(row.query_index); k.distance.push_back(row.distance);
                k.fromXyz.push_back(Point3f{ row.from_xyz[0], row.from_xyz[1], row.from_xyz[2] });
                k.toXy.push_back(Point2f{ row.to_xy[0], row.to_xy[1] });
            }
            candidates.push_back(std::move(k));
        }
        return rc;
    }

    // query() with every candidate verified in the same call.  vp: the PnP parameters, the camera and the guided fields
    // (visfs_place_verify_default_params, then the caller's camera); queryXyz: the 3-D points of the key-points now (one per key-point
    // of describe(), for the covariance) or empty.  *best: the index into `verified` of the candidate with the most inliers, or -1.
    int queryVerify(const visfs_place_verify_params& vp, const std::vector<Point3f>& queryXyz, std::vector<Verified>& verified, int* best) {
        verified.clear();
        if (best) *best = -1;
        if (!set_) return VISFS_BA_ERR_NOT_LOADED;
        int32_t n = 0;
        int rc = visfs_place_set_download(set_, &n, nullptr, nullptr, nullptr, nullptr);
        if (rc != VISFS_BA_OK) return rc;
        if (!queryXyz.empty() && queryXyz.size() != (size_t)n) return VISFS_BA_ERR_BAD_ARGUMENT;
        rc = visfs_place_query_verify(verifier_, set_, &params_, &vp, queryXyz.empty() ? nullptr : &queryXyz[0].x, result_.get(), verify_.get());
        if (rc != VISFS_BA_OK) return rc;
        const visfs_place_result& r = *result_;
        for (int c = 0; c < r.n_candidates; ++c) {
            const visfs_place_verify_candidate& k = verify_->candidate[c];
            Verified v;
            v.slot = r.candidate[c].slot; v.key = r.candidate[c].key; v.guided = k.stage2.ran != 0;
            v.rows = v.guided ? k.stage2.n_rows : k.stage1.n_matches;
            v.inliers = v.guided ? k.stage2.n_inliers : k.stage1.n_inliers;
            std::copy(v.guided ? k.stage2.T : k.stage1.T, (v.guided ? k.stage2.T : k.stage1.T) + 16, v.T);
            std::copy(v.guided ? k.stage2.cov : k.stage1.cov, (v.guided ? k.stage2.cov : k.stage1.cov) + 36, v.cov);
            verified.push_back(v);
        }
        if (best) *best = verify_->best;
        return rc;
    }

    // The loop-closure edge of a verified candidate between the key-frame's vertex i and the query's vertex j: z (x, y, yaw of j in
    // the frame of i), its information (3 x 3 row-major) and (z, roll, pitch) for a gate on poses that leave the plane.
    static int closureEdge(const Verified& v, double z[3], double information[9], double outOfPlane[3]) {
        return visfs_place_closure_edge(v.T, v.cov, z, information, outOfPlane);
    }

    const char* lastError() const { return visfs_place_db_last_error(db_); }
    const char* lastVerifyError() const { return visfs_place_verifier_last_error(verifier_); }
    const char* lastDescribeError() const { return set_ ? visfs_place_set_last_error(set_) : "no flow object attached"; }

private:
    int capacity_;
    visfs_place_params params_{};
    visfs_place_db* db_ = nullptr;
    visfs_place_set* set_ = nullptr;
    visfs_place_verifier* verifier_ = nullptr;
    std::unique_ptr<visfs_place_result> result_;      // 150 KiB: not on the stack
    std::unique_ptr<visfs_place_verify_result> verify_;
};

}  // namespace VISFS

#endif
