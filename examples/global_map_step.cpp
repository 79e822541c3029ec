// global_map_step.cpp — the map drawn from the finished sub-maps before and after a loop closure has corrected their poses
// (VISFS::GlobalMap2D over include/visfs_map.h).
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/global_map_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o global_map_step && ./global_map_step [host]
//
// A robot drives a lap and a fifth of a circle in a room, 40 poses a lap, on odometry that turns a little too far at every step.
// Every scan is inserted into the sub-maps at the drifted pose, and each finished front sub-map is added to a global map as a tile
// (ActiveSubmaps2D::addToMap) before the next insertion drops it.  The poses are the vertices of a pose graph, the second lap's first
// poses are closed against the first lap's, and the graph is optimised.  Each tile then follows its anchor vertex:
// visfs_map_pose_from_anchor -> setPoses -> compose.  Printed, before and after the correction: the output cells that one tile knows
// as occupied (v < 16384) and a later one as free (v > 16384), from an OCCUPIED and a LATEST compose of the same tiles.  `host` runs
// the one-core twins.  Prints one JSON line; the device and the twin print the same numbers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <vector>

#include "ActiveSubmaps2D.h"
#include "GlobalMap2D.h"
#include "PoseGraph2D.h"
#include "visfs_ba.h"

namespace global_map_step {

struct Rng {                      // SplitMix64 -> uniform / normal
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
    double normal() { const double u = uni() + 1e-300, v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

struct Pose { double x, y, yaw; };

inline Pose compose(const Pose& a, const Pose& z) {
    const double c = std::cos(a.yaw), s = std::sin(a.yaw);
    return { a.x + c * z.x - s * z.y, a.y + s * z.x + c * z.y, a.yaw + z.yaw };
}
inline Pose between(const Pose& a, const Pose& b) {
    const double c = std::cos(a.yaw), s = std::sin(a.yaw), dx = b.x - a.x, dy = b.y - a.y;
    return { c * dx + s * dy, c * dy - s * dx, b.yaw - a.yaw };
}

inline void planar(const Pose& p, double T[12]) {
    const double c = std::cos(p.yaw), s = std::sin(p.yaw);
    const double v[12] = { c, -s, 0, p.x, s, c, 0, p.y, 0, 0, 1, 0 };
    for (int i = 0; i < 12; ++i) T[i] = v[i];
}

// n returns on the walls of the room [-3, 3] x [-2, 2], in the robot frame of `p`
inline std::vector<double> scan(const Pose& p, int n, Rng& rng) {
    std::vector<double> out;
    for (int i = 0; i < n; ++i) {
        const double a = 6.283185307179586 * (i + 0.5) / n, dx = std::cos(a + p.yaw), dy = std::sin(a + p.yaw);
        const double tx = dx > 0 ? (3.0 - p.x) / dx : (-3.0 - p.x) / dx, ty = dy > 0 ? (2.0 - p.y) / dy : (-2.0 - p.y) / dy;
        const double r = std::min(tx, ty) + 0.005 * rng.normal();
        out.insert(out.end(), { r * std::cos(a), r * std::sin(a), 0.0 });
    }
    return out;
}

constexpr int kLap = 40, kFrames = 48, kLimit = 4, kReturns = 360;

struct Summary {
    int frames = 0, tiles = 0, closures = 0, launches = 0, copies = 0, waits = 0;
    int cells_before = 0, cells_after = 0, known_before = 0, known_after = 0, conflicts_before = 0, conflicts_after = 0;
    uint64_t hash_before = 0, hash_after = 0;
    double cost_before = 0.0, cost_after = 0.0, end_error_before = 0.0, end_error_after = 0.0;
};

// What the two flavours differ in: inserting a frame, whether the front is finished, and adding the front to the map.
struct Submaps {
    std::function<int(const double T[12], const std::vector<double>& returns)> insert;
    std::function<bool()> front_finished;
    std::function<int(VISFS::GlobalMap2D& map)> add_front;
};

inline uint64_t fnv(const std::vector<uint16_t>& v, uint64_t h = 1469598103934665603ull) {
    for (uint16_t c : v) { h ^= c; h *= 1099511628211ull; }
    return h;
}

// The cells some tile knows as occupied and the latest tile that knows them as free; `known` and `hash` of the ODDS map.
inline int conflicts(VISFS::GlobalMap2D& map, int* cells, int* known, uint64_t* hash) {
    std::vector<uint16_t> latest, occupied, odds;
    if (map.compose(VISFS::GlobalMap2D::Latest) != VISFS_BA_OK || map.download(&latest) != VISFS_BA_OK) return -1;
    if (map.compose(VISFS::GlobalMap2D::Occupied) != VISFS_BA_OK || map.download(&occupied) != VISFS_BA_OK) return -1;
    if (map.compose(VISFS::GlobalMap2D::Odds) != VISFS_BA_OK || map.download(&odds) != VISFS_BA_OK) return -1;
    if (latest.size() != occupied.size() || latest.size() != odds.size()) return -1;
    int n = 0;
    *known = 0;
    for (size_t i = 0; i < latest.size(); ++i) {
        if (odds[i] != 0) ++*known;
        if (occupied[i] != 0 && occupied[i] < 16384 && latest[i] > 16384) ++n;
    }
    *cells = (int)latest.size();
    *hash = fnv(odds, fnv(occupied, fnv(latest)));
    return n;
}

inline int run(visfs_ba_handle* ba, const Submaps& subs, Summary& out) {
    Rng rng{ 4242 };
    const Pose step{ 0.6 * 6.283185307179586 / kLap, 0.0, 6.283185307179586 / kLap };    // a circle of 0.6 m radius
    const double odo_sigma[3] = { 0.004, 0.004, 0.002 };
    const double odo_information[9] = { 1.0 / (0.01 * 0.01), 0, 0, 0, 1.0 / (0.01 * 0.01), 0, 0, 0, 1.0 / (0.006 * 0.006) };
    std::vector<Pose> truth(kFrames), dead(kFrames);
    truth[0] = dead[0] = { 0.6, -0.3, 1.5707963267948966 };
    VISFS::PoseGraph2D graph(ba, kFrames, kFrames + 16);
    VISFS::GlobalMap2D map(ba);
    std::vector<int> anchor;                                                   // per tile: the vertex it follows
    graph.addVertex(dead[0].x, dead[0].y, dead[0].yaw, true);
    for (int f = 0; f < kFrames; ++f) {
        if (f > 0) {
            truth[(size_t)f] = compose(truth[(size_t)f - 1], step);
            // the odometry turns 0.004 rad too far at every step, and is a little noisy
            const Pose z{ step.x + odo_sigma[0] * rng.normal(), step.y + odo_sigma[1] * rng.normal(), step.yaw + 0.004 + odo_sigma[2] * rng.normal() };
            dead[(size_t)f] = compose(dead[(size_t)f - 1], z);
            graph.addVertex(dead[(size_t)f].x, dead[(size_t)f].y, dead[(size_t)f].yaw);
            const double zz[3] = { z.x, z.y, z.yaw };
            graph.addEdge(f - 1, f, zz, odo_information);
        }
        double T[12];
        planar(dead[(size_t)f], T);
        if (subs.insert(T, scan(truth[(size_t)f], kReturns, rng)) != VISFS_BA_OK) return 1;
        ++out.frames;
        if (subs.front_finished()) {                                            // finished and cropped: kept before the next insertion drops it
            if (subs.add_front(map) != VISFS_BA_OK) { std::fprintf(stderr, "add failed: %s\n", map.lastError()); return 1; }
            anchor.push_back(f - kLimit > 0 ? f - kLimit : 0);                  // the middle of its 2 * kLimit insertions
        }
    }
    out.tiles = (int)anchor.size();
    if (anchor.empty()) return 1;
    for (int j = kLap; j < kFrames; ++j) {                                      // the second lap's poses closed against the first lap's
        const int i = j - kLap;
        Pose rel = between(truth[(size_t)i], truth[(size_t)j]);
        rel.x += 0.002 * rng.normal(); rel.y += 0.002 * rng.normal(); rel.yaw += 0.001 * rng.normal();
        const Pose refined = compose(dead[(size_t)i], rel);
        visfs_scan_refine_result r{};
        r.status = VISFS_BA_OK; r.refined = 1;
        r.x = refined.x; r.y = refined.y; r.yaw = refined.yaw;
        const double W[9] = { 2.4e5, 1.0e4, 3.0e4, 1.0e4, 2.1e5, -2.0e4, 3.0e4, -2.0e4, 9.0e5 };
        for (int k = 0; k < 9; ++k) r.information[k] = W[k];
        const double a[3] = { dead[(size_t)i].x, dead[(size_t)i].y, dead[(size_t)i].yaw };
        if (graph.addClosure(i, j, r, a, 3.0) != VISFS_BA_OK) return 1;
        ++out.closures;
    }

    // the map as the drifted odometry draws it: every tile where it was frozen
    out.conflicts_before = conflicts(map, &out.cells_before, &out.known_before, &out.hash_before);
    if (out.conflicts_before < 0) { std::fprintf(stderr, "compose failed: %s\n", map.lastError()); return 1; }
    out.end_error_before = std::hypot(dead[kFrames - 1].x - truth[kFrames - 1].x, dead[kFrames - 1].y - truth[kFrames - 1].y);

    const VISFS::PoseGraph2D::Summary opt = graph.optimize();
    if (opt.status != VISFS_BA_OK) { std::fprintf(stderr, "optimize failed: %d (%s)\n", opt.status, graph.lastError()); return 1; }
    out.cost_before = opt.initialCost; out.cost_after = opt.finalCost;
    const double* last = graph.pose(kFrames - 1);
    out.end_error_after = std::hypot(last[0] - truth[kFrames - 1].x, last[1] - truth[kFrames - 1].y);

    // every tile follows its anchor vertex
    std::vector<double> poses;
    for (int v : anchor) {
        const double frozen[3] = { dead[(size_t)v].x, dead[(size_t)v].y, dead[(size_t)v].yaw };
        const std::array<double, 3> p = VISFS::GlobalMap2D::poseFromAnchor(frozen, graph.pose(v));
        poses.insert(poses.end(), p.begin(), p.end());
    }
    if (map.setPoses(0, poses) != VISFS_BA_OK) return 1;
    out.conflicts_after = conflicts(map, &out.cells_after, &out.known_after, &out.hash_after);
    if (out.conflicts_after < 0) { std::fprintf(stderr, "compose failed: %s\n", map.lastError()); return 1; }
    map.lastCounts(&out.launches, &out.copies, &out.waits);
    return 0;
}

inline bool finished(const visfs_submaps* s) {
    int32_t n = 0;
    visfs_submap_info info[2];
    return visfs_submaps_describe(s, &n, info) == VISFS_BA_OK && n > 0 && info[0].finished != 0;
}

// the one-core twins: host sub-maps over the C ABI
inline int run_host(Summary& out) {
    visfs_submap_params sp;
    visfs_submap_default_params(&sp);
    sp.num_range_data_limit = kLimit;
    visfs_submaps* s = nullptr;
    if (visfs_submaps_create_host(&sp, &s) != VISFS_BA_OK) return 1;
    Submaps subs;
    subs.insert = [&](const double T[12], const std::vector<double>& ret) {
        visfs_range_data rd{};
        rd.n_returns = (int32_t)(ret.size() / 3); rd.returns = ret.data();
        return visfs_submaps_insert(s, T, 1, &rd);
    };
    subs.front_finished = [&]() { return finished(s); };
    subs.add_front = [&](VISFS::GlobalMap2D& map) { return map.addSubmap(s, 0); };
    const int rc = run(nullptr, subs, out);
    visfs_submaps_destroy(s);
    return rc;
}

// the device: VISFS::Map::ActiveSubmaps2D, the tiles and the map on the handle's stream
inline int run_device(visfs_ba_handle* ba, Summary& out) {
    VISFS::Map::ActiveSubmaps2D submaps(ba, kLimit);
    Submaps subs;
    subs.insert = [&](const double T[12], const std::vector<double>& ret) {
        std::vector<VISFS::Map::ActiveSubmaps2D::RangeData> rds(1);
        rds[0].returns = ret;
        return submaps.insertRangeData(rds, T);
    };
    subs.front_finished = [&]() { const auto v = submaps.submaps(); return !v.empty() && v[0].finished != 0; };
    subs.add_front = [&](VISFS::GlobalMap2D& map) { return submaps.addToMap(map, 0); };
    return run(ba, subs, out);
}

}  // namespace global_map_step

int main(int argc, char** argv) {
    bool host = false;
    for (int i = 1; i < argc; ++i) if (std::strcmp(argv[i], "host") == 0) host = true;
    global_map_step::Summary s;
    int rc;
    try {
        if (host) {
            rc = global_map_step::run_host(s);
        } else {
            visfs_ba_params prm;
            visfs_ba_default_params(&prm);
            visfs_ba_handle* ba = nullptr;
            if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
            rc = global_map_step::run_device(ba, s);                             // the map and the sub-maps go before the handle
            visfs_ba_destroy(ba);
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"frames\": %d, \"tiles\": %d, \"closures\": %d, \"cost_before\": %.17g, \"cost_after\": %.17g, "
                "\"end_error_before_m\": %.17g, \"end_error_after_m\": %.17g, \"cells_before\": %d, \"cells_after\": %d, \"known_before\": %d, "
                "\"known_after\": %d, \"conflicts_before\": %d, \"conflicts_after\": %d, \"hash_before\": \"%016llx\", \"hash_after\": \"%016llx\", "
                "\"launches\": %d, \"copies\": %d, \"waits\": %d}\n",
                host ? "host" : "device", s.frames, s.tiles, s.closures, s.cost_before, s.cost_after, s.end_error_before, s.end_error_after,
                s.cells_before, s.cells_after, s.known_before, s.known_after, s.conflicts_before, s.conflicts_after,
                (unsigned long long)s.hash_before, (unsigned long long)s.hash_after, s.launches, s.copies, s.waits);
    return 0;
}
