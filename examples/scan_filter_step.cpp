// scan_filter_step.cpp — the "Filter." step of Estimator::laserPretreatment in front of the laser calls: a dense scan of a room is
// pretreated and voxel-filtered (include/visfs_scan_filter.h), the filtered range data are inserted into the sub-maps, and the match
// cloud is matched with visfs_scan_match.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/scan_filter_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o scan_filter_step && ./scan_filter_step [host]
//
// A robot in a 6 m x 4 m room with a pillar carries a laser 0.1 m ahead of the camera that delivers 7200 returns a turn.  Five
// frames go through the filter in ONE call and are inserted; a sixth is filtered and matched from a guess that is off by
// (0.12 m, -0.08 m, 0.05 rad), once with the match cloud and once with every return of the scan.  `host` runs the filter, the
// sub-maps and the match on the one-core twins: the same bits.  Prints one JSON line.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ScanFilter.h"
#include "visfs_ba.h"
#include "visfs_scan_match.h"
#include "visfs_submap.h"

namespace scan_filter_step {

struct Rng {                      // SplitMix64 -> uniform / normal
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
    double normal() { const double u = uni() + 1e-300, v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

constexpr double kLaserAhead = 0.1;           // the laser's place in the robot (camera) frame
constexpr int kReturns = 7200, kFrames = 5;

inline void planar(double x, double y, double yaw, double T[12]) {
    const double c = std::cos(yaw), s = std::sin(yaw);
    const double v[12] = { c, -s, 0, x, s, c, 0, y, 0, 0, 1, 0 };
    for (int i = 0; i < 12; ++i) T[i] = v[i];
}

// distance along (dx, dy) from (x, y) to the box [x0, x1] x [y0, y1] seen from outside (infinity when missed)
inline double hit_box(double x, double y, double dx, double dy, double x0, double x1, double y0, double y1) {
    double lo = 0.0, hi = 1e30;
    const double o[2] = { x, y }, d[2] = { dx, dy }, a[2] = { x0, y0 }, b[2] = { x1, y1 };
    for (int k = 0; k < 2; ++k) {
        if (std::fabs(d[k]) < 1e-12) { if (o[k] < a[k] || o[k] > b[k]) return 1e30; continue; }
        double t0 = (a[k] - o[k]) / d[k], t1 = (b[k] - o[k]) / d[k];
        if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
        lo = std::max(lo, t0); hi = std::min(hi, t1);
    }
    return lo <= hi && lo > 0.0 ? lo : 1e30;
}

// n returns on the walls of the room [-3, 3] x [-2, 2] and of the pillar [0.9, 1.4] x [-1.3, -0.8] from the laser of the robot at
// (x, y, yaw), in the LASER frame
inline std::vector<double> scan(double x, double y, double yaw, int n, Rng& rng) {
    const double lx = x + kLaserAhead * std::cos(yaw), ly = y + kLaserAhead * std::sin(yaw);
    std::vector<double> out;
    out.reserve(3 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        const double a = 6.283185307179586 * (i + 0.5) / n, dx = std::cos(a + yaw), dy = std::sin(a + yaw);
        const double tx = dx > 0 ? (3.0 - lx) / dx : (-3.0 - lx) / dx, ty = dy > 0 ? (2.0 - ly) / dy : (-2.0 - ly) / dy;
        double r = std::min(std::min(tx, ty), hit_box(lx, ly, dx, dy, 0.9, 1.4, -1.3, -0.8));
        r += 0.005 * rng.normal();
        out.insert(out.end(), { r * std::cos(a), r * std::sin(a), 0.0 });
    }
    return out;
}

inline void true_pose(int f, double p[3]) { p[0] = -0.6 + 0.15 * f; p[1] = 0.2 + 0.04 * f; p[2] = 0.1 * f; }

struct Summary {
    int raw = 0, returns = 0, misses = 0, in_range = 0, match = 0, passes = 0, inserted_raw = 0, inserted_returns = 0;
    int launches = 0, copies = 0, waits = 0;
    double length = 0.0;
    visfs_scan_match_result filtered{}, unfiltered{};
    double err_filtered = 0.0, err_unfiltered = 0.0;
};

inline VISFS::ScanFilter::Scan laser_scan(const std::vector<double>& pts) {
    VISFS::ScanFilter::Scan s;
    s.points = &pts;
    s.T_laser_to_camera[3] = kLaserAhead;
    return s;
}

// ba == nullptr: the one-core twins
inline int run(visfs_ba_handle* ba, Summary& out) {
    visfs_submap_params sp;
    visfs_submap_default_params(&sp);
    visfs_submaps* sub = nullptr;
    if ((ba ? visfs_submaps_create(ba, &sp, &sub) : visfs_submaps_create_host(&sp, &sub)) != VISFS_BA_OK) return 1;
    VISFS::ScanFilter filter(ba);
    filter.params().pretreat.num_subdivisions = 2;
    filter.params().pretreat.max_range = 3.5;                                  // the far corners become misses
    int rc = 1;
    do {
        Rng rng{ 99 };
        std::vector<std::vector<double>> raw((size_t)kFrames);
        std::vector<VISFS::ScanFilter::Scan> scans;
        for (int f = 0; f < kFrames; ++f) {
            double p[3];
            true_pose(f, p);
            raw[(size_t)f] = scan(p[0], p[1], p[2], kReturns, rng);
            scans.push_back(laser_scan(raw[(size_t)f]));
        }
        if (filter.process(scans) != VISFS_BA_OK) { std::fprintf(stderr, "filter failed: %s\n", filter.lastError()); break; }   // five scans, one call
        bool ok = true;
        for (int f = 0; f < kFrames && ok; ++f) {
            double p[3], T[12];
            true_pose(f, p); planar(p[0], p[1], p[2], T);
            const std::vector<visfs_range_data> rd = filter.rangeData(f);
            ok = visfs_submaps_insert(sub, T, (int32_t)rd.size(), rd.data()) == VISFS_BA_OK;
            out.inserted_raw += kReturns; out.inserted_returns += filter.record(f).n_returns;
        }
        if (!ok) { std::fprintf(stderr, "insert failed: %s\n", visfs_submaps_last_error(sub)); break; }

        double truth[3];
        true_pose(kFrames, truth);
        const double guess[3] = { truth[0] + 0.12, truth[1] - 0.08, truth[2] + 0.05 };
        const std::vector<double> last = scan(truth[0], truth[1], truth[2], kReturns, rng);
        if (filter.process({ laser_scan(last) }) != VISFS_BA_OK) { std::fprintf(stderr, "filter failed: %s\n", filter.lastError()); break; }
        filter.lastCounts(&out.launches, &out.copies, &out.waits);
        const visfs_scan_filter_record r = filter.record(0);
        out.raw = kReturns; out.returns = r.n_returns; out.misses = r.n_misses; out.in_range = r.n_in_range; out.match = r.n_match;
        out.passes = r.passes; out.length = r.match_length;
        visfs_scan_match_params mp;
        visfs_scan_match_default_params(&mp);
        mp.linear_search_window = 0.3; mp.angular_search_window = 0.2;
        const double* cloud = nullptr;
        const int n = filter.matchCloud(0, &cloud);
        if (visfs_scan_match(sub, 0, &mp, guess, n, cloud, &out.filtered) != VISFS_BA_OK) { std::fprintf(stderr, "match failed: %s\n", visfs_submaps_last_error(sub)); break; }
        // without the filter: every return of the scan, taken to the robot frame by hand
        std::vector<double> all(last);
        for (size_t i = 0; i < all.size(); i += 3) all[i] += kLaserAhead;
        if (visfs_scan_match(sub, 0, &mp, guess, kReturns, all.data(), &out.unfiltered) != VISFS_BA_OK) { std::fprintf(stderr, "match failed: %s\n", visfs_submaps_last_error(sub)); break; }
        out.err_filtered = std::hypot(out.filtered.x - truth[0], out.filtered.y - truth[1]);
        out.err_unfiltered = std::hypot(out.unfiltered.x - truth[0], out.unfiltered.y - truth[1]);
        rc = 0;
    } while (false);
    visfs_submaps_destroy(sub);
    return rc;
}

}  // namespace scan_filter_step

int main(int argc, char** argv) {
    const bool host = argc > 1 && std::strcmp(argv[1], "host") == 0;
    scan_filter_step::Summary s;
    int rc;
    if (host) {
        rc = scan_filter_step::run(nullptr, s);
    } else {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        visfs_ba_handle* ba = nullptr;
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
        rc = scan_filter_step::run(ba, s);
        visfs_ba_destroy(ba);
    }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"raw_points\": %d, \"returns\": %d, \"misses\": %d, \"in_range\": %d, \"match_points\": %d, \"passes\": %d, "
                "\"match_length\": %.17g, \"inserted_raw\": %d, \"inserted_returns\": %d, "
                "\"filtered\": {\"matched\": %d, \"x\": %.17g, \"y\": %.17g, \"yaw\": %.17g, \"score\": %.17g, \"err_m\": %.17g}, "
                "\"unfiltered\": {\"matched\": %d, \"x\": %.17g, \"y\": %.17g, \"yaw\": %.17g, \"score\": %.17g, \"err_m\": %.17g}, "
                "\"launches\": %d, \"copies\": %d, \"waits\": %d}\n",
                host ? "host" : "device", s.raw, s.returns, s.misses, s.in_range, s.match, s.passes, s.length, s.inserted_raw, s.inserted_returns,
                s.filtered.matched, s.filtered.x, s.filtered.y, s.filtered.yaw, s.filtered.score, s.err_filtered,
                s.unfiltered.matched, s.unfiltered.x, s.unfiltered.y, s.unfiltered.yaw, s.unfiltered.score, s.err_unfiltered,
                s.launches, s.copies, s.waits);
    return 0;
}
