// pose_graph_step.cpp — what follows a loop closure: the constraints that visfs_scan_group_match_refine hands out go into a 2-D pose
// graph beside the odometry chain, and the graph is optimised in one call (VISFS::PoseGraph2D over include/visfs_pose_graph.h).
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/pose_graph_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o pose_graph_step && ./pose_graph_step [host]
//
// A robot drives two laps of a circle, 100 poses each.  Its odometry has noise and a small yaw bias, so the dead-reckoned second lap
// lies beside the first.  Every tenth pose of the second lap is matched against the sub-map around the pose a lap earlier; the
// refinement record (here made from the true relative pose and a little noise, expressed in the drifted frame of that sub-map, with
// an information matrix of the size the refinement returns) becomes an edge through visfs_pose_graph_edge_from_refine.  Pose 0 is
// held.  `host` runs the one-core twin.  Prints one JSON line; the device and the twin print the same numbers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "PoseGraph2D.h"
#include "visfs_ba.h"

namespace pose_graph_step {

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

constexpr int kLap = 100, kVertices = 2 * kLap, kEvery = 10;

struct Summary {
    int vertices = 0, edges = 0, closures = 0, launches = 0, copies = 0, waits = 0;
    VISFS::PoseGraph2D::Summary opt;
    double err_before = 0.0, err_after = 0.0, yaw_err_before = 0.0, yaw_err_after = 0.0;
};

inline void worst(const VISFS::PoseGraph2D& g, const std::vector<Pose>& truth, double* d, double* a) {
    *d = *a = 0.0;
    for (int i = 0; i < g.numVertices(); ++i) {
        const double* p = g.pose(i);
        *d = std::max(*d, std::hypot(p[0] - truth[(size_t)i].x, p[1] - truth[(size_t)i].y));
        *a = std::max(*a, std::fabs(p[2] - truth[(size_t)i].yaw));
    }
}

inline int run(visfs_ba_handle* ba, Summary& out) {
    Rng rng{ 2024 };
    const Pose step{ 0.25, 0.0, 6.283185307179586 / kLap };
    std::vector<Pose> truth(kVertices), dead(kVertices);
    truth[0] = dead[0] = { 0.0, 0.0, 0.0 };
    VISFS::PoseGraph2D graph(ba, kVertices, kVertices + kVertices / kEvery);
    graph.addVertex(0.0, 0.0, 0.0, true);
    const double odo_sigma[3] = { 0.004, 0.004, 0.002 };
    const double odo_information[9] = { 1.0 / (0.004 * 0.004), 0, 0, 0, 1.0 / (0.004 * 0.004), 0, 0, 0, 1.0 / (0.002 * 0.002) };
    for (int i = 1; i < kVertices; ++i) {
        truth[(size_t)i] = compose(truth[(size_t)i - 1], step);
        const Pose z{ step.x + odo_sigma[0] * rng.normal(), step.y + odo_sigma[1] * rng.normal(), step.yaw + 0.0008 + odo_sigma[2] * rng.normal() };
        dead[(size_t)i] = compose(dead[(size_t)i - 1], z);
        graph.addVertex(dead[(size_t)i].x, dead[(size_t)i].y, dead[(size_t)i].yaw);
        const double zz[3] = { z.x, z.y, z.yaw };
        graph.addEdge(i - 1, i, zz, odo_information);
    }
    for (int j = kLap + kEvery; j < kVertices; j += kEvery) {
        const int i = j - kLap;
        Pose rel = between(truth[(size_t)i], truth[(size_t)j]);                 // what the matcher sees: the second lap on top of the first
        rel.x += 0.002 * rng.normal(); rel.y += 0.002 * rng.normal(); rel.yaw += 0.001 * rng.normal();
        const Pose refined = compose(dead[(size_t)i], rel);                     // in the frame the sub-map around i was built in
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
    worst(graph, truth, &out.err_before, &out.yaw_err_before);
    out.opt = graph.optimize();
    if (out.opt.status != VISFS_BA_OK) { std::fprintf(stderr, "optimize failed: %d (%s)\n", out.opt.status, graph.lastError()); return 1; }
    graph.lastCounts(&out.launches, &out.copies, &out.waits);
    worst(graph, truth, &out.err_after, &out.yaw_err_after);
    return 0;
}

}  // namespace pose_graph_step

int main(int argc, char** argv) {
    bool host = false;
    for (int i = 1; i < argc; ++i) if (std::strcmp(argv[i], "host") == 0) host = true;
    pose_graph_step::Summary s;
    int rc;
    try {
        if (host) {
            rc = pose_graph_step::run(nullptr, s);
        } else {
            visfs_ba_params prm;
            visfs_ba_default_params(&prm);
            visfs_ba_handle* ba = nullptr;
            if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
            rc = pose_graph_step::run(ba, s);                                    // the graph goes before the handle
            visfs_ba_destroy(ba);
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"vertices\": %d, \"edges\": %d, \"closures\": %d, \"calls\": %d, \"iterations\": %d, \"trials\": %d, "
                "\"pcg_iterations\": %d, \"termination\": %d, \"cost_before\": %.17g, \"cost_after\": %.17g, \"err_before_m\": %.17g, "
                "\"err_after_m\": %.17g, \"yaw_err_before\": %.17g, \"yaw_err_after\": %.17g, \"launches\": %d, \"copies\": %d, \"waits\": %d}\n",
                host ? "host" : "device", s.vertices, s.edges, s.closures, s.opt.calls, s.opt.iterations, s.opt.trials, s.opt.pcgIterations,
                s.opt.termination, s.opt.initialCost, s.opt.finalCost, s.err_before, s.err_after, s.yaw_err_before, s.yaw_err_after, s.launches,
                s.copies, s.waits);
    return 0;
}
