// ScanFilter.h — the "Filter." step of Estimator::laserPretreatment, with the split and the range classification around it
// (include/visfs_scan_filter.h).  Header only, over the C ABI.
//
// process() takes raw scans in the laser frame, up to 64 a call, and leaves per scan the range data ActiveSubmaps2D inserts
// (returns and misses of every subdivision, each through the fixed voxel filter) and the match cloud the scan matchers take (the
// filtered returns within a range, through the adaptive voxel filter).  A device filter runs one kernel a call on the stream of the
// handle it was made on, which must outlive it; ba == nullptr gives the one-core host twin, which returns the same bytes.
#ifndef VISFS_AMD_SCAN_FILTER_H
#define VISFS_AMD_SCAN_FILTER_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "visfs_scan_filter.h"

namespace VISFS {

class ScanFilter {
public:
    // One raw scan: points [n][3] in the laser frame (the vector must stay alive through process()).
    struct Scan {
        const std::vector<double>* points = nullptr;
        double T_laser_to_camera[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        double origin[3] = { 0, 0, 0 };
    };

    // Throws std::runtime_error when creation fails.
    explicit ScanFilter(visfs_ba_handle* ba) {
        const int rc = visfs_scan_filter_create(ba, &f_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_scan_filter_create failed with status " + std::to_string(rc));
        visfs_scan_filter_default_params(&params_);
    }
    ScanFilter(const ScanFilter&) = delete;
    ScanFilter& operator=(const ScanFilter&) = delete;
    ~ScanFilter() { visfs_scan_filter_destroy(f_); }

    visfs_scan_filter* get() const { return f_; }
    visfs_scan_filter_params& params() { return params_; }                // what process() uses; the defaults at first

    // A refusal (VISFS_BA_ERR_BAD_ARGUMENT / _UNSUPPORTED) leaves the last call's results in place.
    int process(const std::vector<Scan>& scans) {
        std::vector<visfs_scan_filter_scan> s(scans.size());
        for (size_t i = 0; i < scans.size(); ++i) {
            for (int k = 0; k < 12; ++k) s[i].T_laser_to_camera[k] = scans[i].T_laser_to_camera[k];
            for (int k = 0; k < 3; ++k) s[i].origin[k] = scans[i].origin[k];
            s[i].n = scans[i].points ? (int32_t)(scans[i].points->size() / 3) : 0;
            s[i].points_xyz = scans[i].points ? scans[i].points->data() : nullptr;
        }
        return visfs_scan_filter_process(f_, &params_, (int32_t)s.size(), s.data(), nullptr);
    }
    int process(const std::vector<double>& points) {                      // one scan already in the robot frame
        Scan s;
        s.points = &points;
        return process(std::vector<Scan>{ s });
    }

    int numScans() const { int32_t m = 0; visfs_scan_filter_num_scans(f_, &m); return m; }
    // Throws std::out_of_range for a scan the last call did not hold.
    visfs_scan_filter_record record(int scan) const {
        visfs_scan_filter_record r{};
        if (visfs_scan_filter_record_of(f_, scan, &r) != VISFS_BA_OK) throw std::out_of_range("ScanFilter::record");
        return r;
    }
    // The range data of a scan as visfs_submaps_insert takes them; they point into the filter and are valid until the next process().
    std::vector<visfs_range_data> rangeData(int scan) const {
        std::vector<visfs_range_data> rd(VISFS_SCAN_FILTER_MAX_SUBDIVISIONS);
        int32_t n = 0;
        if (visfs_scan_filter_range_data(f_, scan, (int32_t)rd.size(), rd.data(), &n) != VISFS_BA_OK) throw std::out_of_range("ScanFilter::rangeData");
        rd.resize((size_t)n);
        return rd;
    }
    // The match cloud [n][3] where it lies in the filter (valid until the next process()); returns n.
    int matchCloud(int scan, const double** xyz) const {
        int32_t n = 0;
        if (visfs_scan_filter_match_cloud(f_, scan, xyz, &n) != VISFS_BA_OK) throw std::out_of_range("ScanFilter::matchCloud");
        return n;
    }

    // what the last call issued on the device (all zero on the twin)
    void lastCounts(int* launches, int* copies, int* waits) const {
        int32_t k = 0, c = 0, w = 0;
        visfs_scan_filter_last_counts(f_, &k, &c, &w);
        if (launches) *launches = k;
        if (copies) *copies = c;
        if (waits) *waits = w;
    }

    const char* lastError() const { return visfs_scan_filter_last_error(f_); }

private:
    visfs_scan_filter* f_ = nullptr;
    visfs_scan_filter_params params_{};
};

}  // namespace VISFS

#endif
