// GlobalMap2D.h — the map drawn from finished sub-maps at their corrected poses (include/visfs_map.h).  Header only, over the C ABI.
//
// ActiveSubmaps2D drops a finished front sub-map; ActiveSubmaps2D::addToMap freezes its raw cells as a tile of a GlobalMap2D before
// that happens (on the device the cells never cross to the host).  A tile carries the pose that takes its grid frame into the map
// frame: the identity when it is added, and after a pose-graph optimisation poseFromAnchor(anchor as it was, anchor as it is now).
// compose() draws every tile into one grid; download() fetches it; freeze() makes one ScanStack of it, so that relocalisation after
// a loop closure searches one stack instead of one per sub-map.  A device map runs on the stream of the handle it was made on, which
// must outlive it; ba == nullptr gives the one-core host twin, which returns the same bytes.
#ifndef VISFS_AMD_GLOBAL_MAP_2D_H
#define VISFS_AMD_GLOBAL_MAP_2D_H

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ScanStack.h"
#include "visfs_map.h"

namespace VISFS {

class GlobalMap2D {
public:
    enum Combine { Odds = VISFS_MAP_ODDS, Latest = VISFS_MAP_LATEST, Occupied = VISFS_MAP_OCCUPIED };

    // Throws std::runtime_error when creation fails.
    explicit GlobalMap2D(visfs_ba_handle* ba) {
        const int rc = visfs_map_create(ba, &m_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_map_create failed with status " + std::to_string(rc));
    }
    GlobalMap2D(const GlobalMap2D&) = delete;
    GlobalMap2D& operator=(const GlobalMap2D&) = delete;
    ~GlobalMap2D() { visfs_map_destroy(m_); }

    visfs_map* get() const { return m_; }

    // Sub-map `index` of `s` as it stands becomes the next tile (pose == nullptr: the identity).  The sub-maps must be of the map's
    // flavour.  ActiveSubmaps2D::addToMap calls this.
    int addSubmap(visfs_submaps* s, int index = 0, const double pose[3] = nullptr, int* tile = nullptr) {
        const double id[3] = { 0.0, 0.0, 0.0 };
        int32_t t = -1;
        const int rc = visfs_map_add_submap(m_, s, index, pose ? pose : id, &t);
        if (tile) *tile = t;
        return rc;
    }
    // The same from a saved grid: cells [num_y_cells][num_x_cells].
    int addGrid(const visfs_submap_info& limits, const std::vector<uint16_t>& cells, const double pose[3] = nullptr, int* tile = nullptr) {
        if (limits.num_x_cells < 1 || limits.num_y_cells < 1 || cells.size() != (size_t)limits.num_x_cells * (size_t)limits.num_y_cells)
            return VISFS_BA_ERR_BAD_ARGUMENT;
        const double id[3] = { 0.0, 0.0, 0.0 };
        int32_t t = -1;
        const int rc = visfs_map_add_grid(m_, &limits, cells.data(), pose ? pose : id, &t);
        if (tile) *tile = t;
        return rc;
    }

    // The tile pose that follows an anchor from where it was when the tile was frozen to where it is now.
    static std::array<double, 3> poseFromAnchor(const double anchorWhenFrozen[3], const double anchorNow[3]) {
        std::array<double, 3> p{ { 0.0, 0.0, 0.0 } };
        if (visfs_map_pose_from_anchor(anchorWhenFrozen, anchorNow, p.data()) != VISFS_BA_OK) throw std::runtime_error("poseFromAnchor: a pose is not finite");
        return p;
    }
    // poses: [count][3] for the tiles first .. first + count - 1.  Host only: nothing is launched or copied.
    int setPoses(int first, const std::vector<double>& poses) { return visfs_map_set_poses(m_, first, (int32_t)(poses.size() / 3), poses.data()); }
    int clear() { return visfs_map_clear(m_); }

    // Draws the tiles at `resolution`, the limits taken from their extents (or `limits` when given).
    int compose(Combine combine = Odds, double resolution = 0.05, const visfs_submap_info* limits = nullptr, visfs_map_info* info = nullptr) {
        visfs_map_params p;
        visfs_map_default_params(&p);
        p.combine = combine; p.resolution = resolution;
        if (limits) { p.explicit_limits = 1; p.limits = *limits; }
        visfs_map_info i{};
        const int rc = visfs_map_compose(m_, &p, &i);
        if (rc == VISFS_BA_OK) info_ = i;
        if (info) *info = i;
        return rc;
    }
    const visfs_map_info& info() const { return info_; }                  // of the last successful compose

    // the last composed grid on the host ([num_y_cells][num_x_cells]); either pointer may be null
    int download(std::vector<uint16_t>* cells, std::vector<uint8_t>* counts = nullptr) const {
        const size_t n = (size_t)info_.limits.num_x_cells * (size_t)info_.limits.num_y_cells;
        if (cells) cells->resize(n);
        if (counts) counts->resize(n);
        return visfs_map_download(m_, cells ? cells->data() : nullptr, counts ? counts->data() : nullptr);
    }

    // The last composed grid frozen with `depth` levels, read where it lives.  Throws when there is no composed grid.
    ScanStack freeze(int depth = 7) const {
        visfs_scan_stack* st = nullptr;
        const int rc = visfs_scan_stack_create_from_map(m_, depth, &st);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_scan_stack_create_from_map failed with status " + std::to_string(rc) + ": " + lastError());
        return ScanStack(st);
    }

    // what the last compose issued on the device (all zero on the twin)
    void lastCounts(int* launches, int* copies, int* waits) const {
        int32_t k = 0, c = 0, w = 0;
        visfs_map_last_counts(m_, &k, &c, &w);
        if (launches) *launches = k;
        if (copies) *copies = c;
        if (waits) *waits = w;
    }

    const char* lastError() const { return visfs_map_last_error(m_); }

private:
    visfs_map* m_ = nullptr;
    visfs_map_info info_{};
};

}  // namespace VISFS

#endif
