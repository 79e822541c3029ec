// ScanStack.h — a frozen sub-map grid with its window-maximum levels, searched by branch and bound (include/visfs_scan_fast.h):
// relocalisation in a known map and loop closure against a finished sub-map.  Header only, over the C ABI.
//
// A ScanStack comes from ActiveSubmaps2D::freeze (a snapshot of a live sub-map: later insertions do not change it) or from a saved
// grid (fromGrid: the cells and limits ActiveSubmaps2D::download and submaps() hand out).  A device stack runs on the stream of the
// handle it was made on, which must outlive it.
#ifndef VISFS_AMD_SCAN_STACK_H
#define VISFS_AMD_SCAN_STACK_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "visfs_scan_fast.h"

namespace VISFS {

class ScanStack {
public:
    ScanStack() = default;
    explicit ScanStack(visfs_scan_stack* st) : st_(st) {}                 // takes ownership
    ScanStack(const ScanStack&) = delete;
    ScanStack& operator=(const ScanStack&) = delete;
    ScanStack(ScanStack&& o) noexcept : st_(o.st_) { o.st_ = nullptr; }
    ScanStack& operator=(ScanStack&& o) noexcept { if (this != &o) { visfs_scan_stack_destroy(st_); st_ = o.st_; o.st_ = nullptr; } return *this; }
    ~ScanStack() { visfs_scan_stack_destroy(st_); }

    // From a saved grid: cells [num_y_cells][num_x_cells].  ba == nullptr: the one-core host twin.  Throws when creation fails.
    static ScanStack fromGrid(visfs_ba_handle* ba, const visfs_submap_info& limits, const std::vector<uint16_t>& cells, int depth = 7) {
        if (limits.num_x_cells < 1 || limits.num_y_cells < 1 || cells.size() != (size_t)limits.num_x_cells * (size_t)limits.num_y_cells)
            throw std::runtime_error("ScanStack::fromGrid: the cells do not fit the limits");
        visfs_scan_stack* st = nullptr;
        const int rc = visfs_scan_stack_create_from_grid(ba, &limits, cells.data(), depth, &st);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_scan_stack_create_from_grid failed with status " + std::to_string(rc));
        return ScanStack(st);
    }

    bool valid() const { return st_ != nullptr; }
    visfs_scan_stack_info info() const { visfs_scan_stack_info i{}; visfs_scan_stack_describe(st_, &i); return i; }

    // The pose guess (x, y, yaw) corrected by the search of the returns (robot frame, xyz triples) within the windows of `params`
    // (default: 7 m, 30 degrees).  matched is false when the best score lies below params->min_score, or without returns.
    struct Match { double x = 0.0, y = 0.0, yaw = 0.0, score = 0.0; bool matched = false; };
    int match(const double guess[3], const std::vector<double>& returns, Match* out, const visfs_scan_stack_params* params = nullptr,
              visfs_scan_stack_result* full = nullptr) const {
        visfs_scan_stack_params p;
        if (params) p = *params; else visfs_scan_stack_default_params(&p);
        visfs_scan_stack_result r;
        const int rc = visfs_scan_stack_match(st_, &p, guess, (int32_t)(returns.size() / 3), returns.data(), &r);
        if (rc != VISFS_BA_OK) return rc;
        if (out) { out->x = r.match.x; out->y = r.match.y; out->yaw = r.match.yaw; out->score = r.match.score; out->matched = r.match.matched != 0; }
        if (full) *full = r;
        return rc;
    }

    const char* lastError() const { return visfs_scan_stack_last_error(st_); }

private:
    visfs_scan_stack* st_ = nullptr;
};

}  // namespace VISFS

#endif
