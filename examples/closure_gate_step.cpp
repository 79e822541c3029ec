// closure_gate_step.cpp — the link back from the pose graph to the loop-closure search: how far and how wide the search for one
// candidate closure has to look, from how uncertain the optimised graph is about the scan's vertex relative to the sub-map's anchor
// vertex (VISFS::PoseGraph2D::searchWindow over include/visfs_pose_graph_cov.h).
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/closure_gate_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o closure_gate_step && ./closure_gate_step [host]
//
// A robot drives a lap and six tenths of a circle, 100 poses a lap.  Three closures early in the second lap are already in the graph,
// which is optimised.  The candidate is the scan of the last vertex against the sub-map anchored a lap earlier: its window is three
// standard deviations of the relative pose of the two vertices, instead of the blanket 7 m / 30 degrees.  For comparison the window
// of two neighbours on the chain, which only the odometry edge between them separates.  Pose 0 is held.  `host` runs the one-core
// twin.  Prints one JSON line; the device and the twin print the same numbers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "PoseGraph2D.h"
#include "visfs_ba.h"

namespace closure_gate_step {

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

constexpr int kLap = 100, kVertices = 160, kSigmas = 3;
constexpr double kBlanketLinear = 7.0, kBlanketAngular = 0.5235987755982988;     // 7 m, 30 degrees

struct Summary {
    int vertices = 0, edges = 0, closures = 0, anchor = 0, scan = 0, launches = 0, copies = 0, waits = 0;
    VISFS::PoseGraph2D::Summary opt;
    visfs_pose_graph_cov_result cov{};
    double linear = 0.0, angular = 0.0, near_linear = 0.0, near_angular = 0.0, miss_m = 0.0, miss_rad = 0.0;
};

inline int run(visfs_ba_handle* ba, Summary& out) {
    Rng rng{ 2025 };
    const Pose step{ 0.25, 0.0, 6.283185307179586 / kLap };
    std::vector<Pose> truth(kVertices), dead(kVertices);
    truth[0] = dead[0] = { 0.0, 0.0, 0.0 };
    VISFS::PoseGraph2D graph(ba, kVertices, kVertices + 8);
    graph.addVertex(0.0, 0.0, 0.0, true);
    const double odo_sigma[3] = { 0.004, 0.004, 0.002 };
    const double odo_information[9] = { 1.0 / (0.004 * 0.004), 0, 0, 0, 1.0 / (0.004 * 0.004), 0, 0, 0, 1.0 / (0.002 * 0.002) };
    for (int i = 1; i < kVertices; ++i) {
        truth[(size_t)i] = compose(truth[(size_t)i - 1], step);
        const Pose z{ step.x + odo_sigma[0] * rng.normal(), step.y + odo_sigma[1] * rng.normal(), step.yaw + odo_sigma[2] * rng.normal() };
        dead[(size_t)i] = compose(dead[(size_t)i - 1], z);
        graph.addVertex(dead[(size_t)i].x, dead[(size_t)i].y, dead[(size_t)i].yaw);
        const double zz[3] = { z.x, z.y, z.yaw };
        graph.addEdge(i - 1, i, zz, odo_information);
    }
    for (int j = kLap + 10; j <= kLap + 30; j += 10) {                         // the closures found so far
        const int i = j - kLap;
        Pose rel = between(truth[(size_t)i], truth[(size_t)j]);
        rel.x += 0.002 * rng.normal(); rel.y += 0.002 * rng.normal(); rel.yaw += 0.001 * rng.normal();
        const Pose refined = compose(dead[(size_t)i], rel);
        visfs_scan_refine_result r{};
        r.status = VISFS_BA_OK; r.refined = 1;
        r.x = refined.x; r.y = refined.y; r.yaw = refined.yaw;
        const double W[9] = { 2.4e5, 1.0e4, 3.0e4, 1.0e4, 2.1e5, -2.0e4, 3.0e4, -2.0e4, 9.0e5 };
        for (int k = 0; k < 9; ++k) r.information[k] = W[k];
        const double anchor[3] = { dead[(size_t)i].x, dead[(size_t)i].y, dead[(size_t)i].yaw };
        if (graph.addClosure(i, j, r, anchor, 3.0) != VISFS_BA_OK) return 1;
        ++out.closures;
    }
    out.vertices = graph.numVertices(); out.edges = graph.numEdges();
    out.opt = graph.optimize();
    if (out.opt.status != VISFS_BA_OK) { std::fprintf(stderr, "optimize failed: %d (%s)\n", out.opt.status, graph.lastError()); return 1; }

    // the candidate: the scan of the last vertex against the sub-map anchored a lap earlier
    out.scan = kVertices - 1; out.anchor = out.scan - kLap;
    const auto c = graph.covariance({ { out.anchor, out.scan }, { out.scan - 1, out.scan } });
    if (c.status != VISFS_BA_OK) { std::fprintf(stderr, "covariance failed: %d (%s)\n", c.status, graph.lastError()); return 1; }
    out.cov = c.result;
    graph.covLastCounts(&out.launches, &out.copies, &out.waits);
    if (visfs_pose_graph_cov_search_window(c.relative.data(), kSigmas, &out.linear, &out.angular) != VISFS_BA_OK) return 1;
    if (visfs_pose_graph_cov_search_window(c.relative.data() + 9, kSigmas, &out.near_linear, &out.near_angular) != VISFS_BA_OK) return 1;
    double lin = 0.0, ang = 0.0;                                              // the container's one-call form gives the same window
    if (graph.searchWindow(out.anchor, out.scan, kSigmas, &lin, &ang) != VISFS_BA_OK || lin != out.linear || ang != out.angular) return 1;

    // how far the graph's relative pose of the pair is from the true one: what the window has to cover
    const double* pa = graph.pose(out.anchor);
    const double* pb = graph.pose(out.scan);
    const Pose have = between({ pa[0], pa[1], pa[2] }, { pb[0], pb[1], pb[2] });
    const Pose want = between(truth[(size_t)out.anchor], truth[(size_t)out.scan]);
    out.miss_m = std::hypot(have.x - want.x, have.y - want.y);
    out.miss_rad = std::fabs(have.yaw - want.yaw);
    return 0;
}

}  // namespace closure_gate_step

int main(int argc, char** argv) {
    bool host = false;
    for (int i = 1; i < argc; ++i) if (std::strcmp(argv[i], "host") == 0) host = true;
    closure_gate_step::Summary s;
    int rc;
    try {
        if (host) {
            rc = closure_gate_step::run(nullptr, s);
        } else {
            visfs_ba_params prm;
            visfs_ba_default_params(&prm);
            visfs_ba_handle* ba = nullptr;
            if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
            rc = closure_gate_step::run(ba, s);                                  // the graph goes before the handle
            visfs_ba_destroy(ba);
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"vertices\": %d, \"edges\": %d, \"closures\": %d, \"cost_before\": %.17g, \"cost_after\": %.17g, "
                "\"anchor\": %d, \"scan\": %d, \"sigmas\": %d, \"linear_window_m\": %.17g, \"angular_window_rad\": %.17g, "
                "\"neighbour_linear_window_m\": %.17g, \"neighbour_angular_window_rad\": %.17g, \"blanket_linear_m\": %.17g, "
                "\"blanket_angular_rad\": %.17g, \"miss_m\": %.17g, \"miss_rad\": %.17g, \"sources\": %d, \"columns\": %d, "
                "\"pcg_iterations_max\": %d, \"pcg_iterations_total\": %d, \"unconverged_columns\": %d, \"launches\": %d, \"copies\": %d, \"waits\": %d}\n",
                host ? "host" : "device", s.vertices, s.edges, s.closures, s.opt.initialCost, s.opt.finalCost, s.anchor, s.scan,
                closure_gate_step::kSigmas, s.linear, s.angular, s.near_linear, s.near_angular, closure_gate_step::kBlanketLinear,
                closure_gate_step::kBlanketAngular, s.miss_m, s.miss_rad, s.cov.sources, s.cov.columns, s.cov.pcg_iterations_max,
                s.cov.pcg_iterations_total, s.cov.unconverged_columns, s.launches, s.copies, s.waits);
    return 0;
}
