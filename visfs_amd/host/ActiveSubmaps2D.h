// ActiveSubmaps2D.h — drop-in for the sub-map side of VISFS::Map::ActiveSubmaps2D (corelib/include/Map/2d/Submap2D.h) backed by
// the GPU-resident sub-maps of include/visfs_submap.h.  Header only, over the C ABI.
//
// It keeps what LocalMap uses of the reference class: the constructor taking the LocalMap/* keys, insertion of a frame's range data
// at its pose (LocalMap::insertMatchingSubMap2d, LocalMap.cpp:355-360), whether a matching sub-map exists (hasMatchingSubmap2D) and
// the BA against it (Estimator.cpp:247-250 + Optimizer::localOptimize).  The grids stay on the device: there is no Submap2D object to
// hand out; download() copies one to the host for those who want grid2Image.  match() is the correlative scan match that
// Estimator::laserPretreatment names and leaves out (include/visfs_scan_match.h): it corrects a pose guess against a sub-map.
// freeze() snapshots a sub-map as a VISFS::ScanStack (ScanStack.h) for relocalisation and loop closure.  refine() takes a matched
// pose off the search lattice (include/visfs_scan_refine.h).  addToMap() freezes a sub-map's raw cells as a tile of a
// VISFS::GlobalMap2D (GlobalMap2D.h), the map drawn from the sub-maps at their corrected poses.
#ifndef VISFS_AMD_ACTIVE_SUBMAPS_2D_H
#define VISFS_AMD_ACTIVE_SUBMAPS_2D_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "GlobalMap2D.h"
#include "ScanStack.h"
#include "visfs_scan_match.h"
#include "visfs_submap.h"

namespace VISFS {
namespace Map {

class ActiveSubmaps2D {
public:
    // One Sensor::RangeData in the robot frame: origin, returns and misses as xyz triples.
    struct RangeData {
        double origin[3] = { 0.0, 0.0, 0.0 };
        std::vector<double> returns;   // [k][3]
        std::vector<double> misses;    // [m][3]
    };

    ActiveSubmaps2D(const ActiveSubmaps2D&) = delete;
    ActiveSubmaps2D& operator=(const ActiveSubmaps2D&) = delete;

    // ba: the handle whose device and stream the grids live on.  Throws std::runtime_error when creation fails (GridMapType 1 = TSDF
    // included, where the reference stops with LOG_FATAL).
    ActiveSubmaps2D(visfs_ba_handle* ba, int numRangeDataLimit = 50, int gridType = 0, double gridResolution = 0.05,
                    bool insertFreeSpace = true, double hitProbability = 0.55, double missProbability = 0.49) : ba_(ba) {
        visfs_submap_params p;
        visfs_submap_default_params(&p);
        p.num_range_data_limit = numRangeDataLimit; p.grid_map_type = gridType; p.map_resolution = gridResolution;
        p.insert_free_space = insertFreeSpace ? 1 : 0; p.hit_probability = hitProbability; p.miss_probability = missProbability;
        const int rc = visfs_submaps_create(ba, &p, &s_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_submaps_create failed with status " + std::to_string(rc));
    }
    ~ActiveSubmaps2D() { visfs_submaps_destroy(s_); }

    // LocalMap::insertMatchingSubMap2d: each range data its own insertion, in order, at pose Twr (3x4 row-major).
    int insertRangeData(const std::vector<RangeData>& rangeDatas, const double Twr[12]) {
        std::vector<visfs_range_data> rd(rangeDatas.size());
        for (size_t i = 0; i < rangeDatas.size(); ++i) {
            const RangeData& r = rangeDatas[i];
            for (int k = 0; k < 3; ++k) rd[i].origin[k] = r.origin[k];
            rd[i].n_returns = (int32_t)(r.returns.size() / 3); rd[i].returns = r.returns.data();
            rd[i].n_misses = (int32_t)(r.misses.size() / 3); rd[i].misses = r.misses.data();
        }
        return visfs_submaps_insert(s_, Twr, (int32_t)rd.size(), rd.data());
    }

    // LocalMap::hasMatchingSubmap2D
    bool hasMatchingSubmap2D() const { int32_t n = 0; visfs_submaps_describe(s_, &n, nullptr); return n > 0; }

    // the sub-maps, front (matching) first
    std::vector<visfs_submap_info> submaps() const {
        int32_t n = 0;
        visfs_submap_info info[2];
        visfs_submaps_describe(s_, &n, info);
        return std::vector<visfs_submap_info>(info, info + n);
    }

    // Estimator.cpp:247-250 + localOptimize: the window's laser factor reads getMatchingSubmap2D() in device memory
    int solveWindow(const visfs_ba_window* w, visfs_ba_result* r) const { return visfs_submaps_solve_window(ba_, s_, w, r); }

    // The pose guess (x, y, yaw) corrected by the correlative scan match of the returns (robot frame, xyz triples) against sub-map
    // `index` (0: the matching sub-map).  Before the first insertion, or without returns, the guess comes back with matched = false.
    struct Match { double x = 0.0, y = 0.0, yaw = 0.0, score = 0.0; bool matched = false; };
    int match(const double guess[3], const std::vector<double>& returns, Match* out, const visfs_scan_match_params* params = nullptr,
              int index = 0, visfs_scan_match_result* full = nullptr) const {
        visfs_scan_match_params p;
        if (params) p = *params; else visfs_scan_match_default_params(&p);
        visfs_scan_match_result r;
        const int rc = visfs_scan_match(s_, index, &p, guess, (int32_t)(returns.size() / 3), returns.data(), &r);
        if (rc != VISFS_BA_OK) return rc;
        if (out) { out->x = r.x; out->y = r.y; out->yaw = r.yaw; out->score = r.score; out->matched = r.matched != 0; }
        if (full) *full = r;
        return rc;
    }

    // The pose `initial` (x, y, yaw; match()'s result) refined on sub-map `index` towards the translation `target` (the prediction):
    // the continuous step that follows the correlative match (include/visfs_scan_refine.h).  Nothing in the sub-maps changes.
    int refine(const double initial[3], const double target[2], const std::vector<double>& returns, RefinedPose* out,
               const visfs_scan_refine_params* params = nullptr, int index = 0, visfs_scan_refine_result* full = nullptr) const {
        visfs_scan_refine_params p;
        if (params) p = *params; else visfs_scan_refine_default_params(&p);
        visfs_scan_refine_result r;
        const int rc = visfs_scan_refine(s_, index, &p, initial, target, (int32_t)(returns.size() / 3), returns.data(), &r);
        if (rc != VISFS_BA_OK) return rc;
        if (out) *out = RefinedPose::from(r);
        if (full) *full = r;
        return rc;
    }

    // Sub-map `index` as it is now, frozen with `depth` levels for the branch-and-bound search (include/visfs_scan_fast.h): later
    // insertions, finishing and cropping do not change the stack.  Throws std::runtime_error when there is no such sub-map.
    ScanStack freeze(int index = 0, int depth = 7) const {
        visfs_scan_stack* st = nullptr;
        const int rc = visfs_scan_stack_create(s_, index, depth, &st);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_scan_stack_create failed with status " + std::to_string(rc) + ": " + lastError());
        return ScanStack(st);
    }

    // Sub-map `index` as it is now becomes the next tile of `map` (GlobalMap2D.h) at `pose` (nullptr: the identity): the way to keep
    // a finished front sub-map's raw cells, which are dropped with it.  The cells go from device memory to device memory.
    int addToMap(GlobalMap2D& map, int index = 0, const double pose[3] = nullptr, int* tile = nullptr) const {
        return map.addSubmap(s_, index, pose, tile);
    }

    // one sub-map's cells and float costs on the host ([num_y_cells][num_x_cells])
    int download(int index, std::vector<uint16_t>* cells, std::vector<float>* cost) const {
        const std::vector<visfs_submap_info> v = submaps();
        if (index < 0 || index >= (int)v.size()) return VISFS_BA_ERR_BAD_ARGUMENT;
        const size_t n = (size_t)v[index].num_x_cells * v[index].num_y_cells;
        if (cells) cells->resize(n);
        if (cost) cost->resize(n);
        return visfs_submaps_download(s_, index, cells ? cells->data() : nullptr, cost ? cost->data() : nullptr);
    }

    const char* lastError() const { return visfs_submaps_last_error(s_); }

private:
    visfs_ba_handle* ba_ = nullptr;
    visfs_submaps* s_ = nullptr;
};

}  // namespace Map
}  // namespace VISFS

#endif
