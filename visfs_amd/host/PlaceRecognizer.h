// PlaceRecognizer.h — visual place recognition beside VISFS::Tracker: what the reference's localisation launch files run rtabmap for
// (Kp/DetectorStrategy 8: GFTT corners with ORB descriptors, Kp/MaxFeatures 500, Mem/STMSize 30), over include/visfs_place.h.
// Header only, over the C ABI.
//
// The recognizer owns the key-frame store.  A flow object (a visfs_flow of the caller) is attached to it;
// describe() then works on that object's resident left image, addKeyFrame() appends what was described with the words' ids and 3-D
// points, and query() returns, per recognised key-frame, the from_xyz / to_xy rows visfs_pnp_solve takes.  A lost tracker is
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

    PlaceRecognizer(const PlaceRecognizer&) = delete;
    PlaceRecognizer& operator=(const PlaceRecognizer&) = delete;

    // ba: the handle whose device and stream the store lives on, or nullptr for the one-core twin (with host flow objects).
    explicit PlaceRecognizer(visfs_ba_handle* ba, int maxKeyFrames = 30, int maxFeatures = 500)
        : capacity_(std::min(std::max(maxFeatures, 1), VISFS_PLACE_MAX_POINTS)), result_(new visfs_place_result()) {
        visfs_place_default_params(&params_);
        const int rc = visfs_place_db_create(ba, maxKeyFrames, &db_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_place_db_create failed with status " + std::to_string(rc));
    }
    ~PlaceRecognizer() {
        detach();
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

    const char* lastError() const { return visfs_place_db_last_error(db_); }
    const char* lastDescribeError() const { return set_ ? visfs_place_set_last_error(set_) : "no flow object attached"; }

private:
    int capacity_;
    visfs_place_params params_{};
    visfs_place_db* db_ = nullptr;
    visfs_place_set* set_ = nullptr;
    std::unique_ptr<visfs_place_result> result_;      // 150 KiB: not on the stack
};

}  // namespace VISFS

#endif
