// loop_closure_step.cpp — a robot that comes back to a mapped place does not know which sub-map it is in: its scan is matched against
// every finished sub-map in one call (VISFS::ScanStackGroup over include/visfs_scan_group.h), the best member's pose is settled by the
// weighted correlative match (include/visfs_scan_match.h) as relocalise_step.cpp does, and would then go to the window solve.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/loop_closure_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o loop_closure_step && ./loop_closure_step [host] [refine]
//
// The room and the pillar are those of relocalise_step.cpp.  With LocalMap/NumRangeDataLimit = 3 a sub-map is finished (and cropped)
// after six insertions and dropped at the next one; twelve frames along the arc finish three, each frozen while it is the front.
// `host` runs the insertions, the stacks, the group and the local match on the one-core host twins.  `refine` makes the group call
// visfs_scan_group_match_refine (include/visfs_scan_refine.h): every matched member's pose leaves the search lattice in the same call,
// and the best member's refined pose, its costs and the trace of its information matrix join the output.  Prints one JSON line.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <string>
#include <vector>

#include "ActiveSubmaps2D.h"
#include "ScanStack.h"
#include "visfs_ba.h"
#include "visfs_scan_group.h"
#include "visfs_scan_match.h"

namespace loop_closure_step {

struct Rng {                      // SplitMix64 -> uniform / normal
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
    double normal() { const double u = uni() + 1e-300, v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

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

// n returns on the walls of the room [-3, 3] x [-2, 2] and of the pillar [0.9, 1.4] x [-1.3, -0.8], in the robot frame of (x, y, yaw)
inline std::vector<double> scan(double x, double y, double yaw, int n, Rng& rng) {
    std::vector<double> out;
    for (int i = 0; i < n; ++i) {
        const double a = 6.283185307179586 * (i + 0.5) / n, dx = std::cos(a + yaw), dy = std::sin(a + yaw);
        const double tx = dx > 0 ? (3.0 - x) / dx : (-3.0 - x) / dx, ty = dy > 0 ? (2.0 - y) / dy : (-2.0 - y) / dy;
        double r = std::min(std::min(tx, ty), hit_box(x, y, dx, dy, 0.9, 1.4, -1.3, -0.8));
        r += 0.005 * rng.normal();
        out.insert(out.end(), { r * std::cos(a), r * std::sin(a), 0.0 });
    }
    return out;
}

constexpr int kLimit = 3;         // a sub-map is finished after 2 * kLimit insertions
constexpr int kFrames = 12;       // three finished sub-maps
constexpr int kDepth = 7;
inline void true_pose(int f, double p[3]) { p[0] = -0.6 + 0.15 * f; p[1] = 0.2 + 0.04 * f; p[2] = 0.1 * f; }
// the pose the robot believes on its return: off by (1.1 m, -0.7 m, 0.35 rad)
inline void drifted_guess(const double truth[3], double g[3]) { g[0] = truth[0] + 1.1; g[1] = truth[1] - 0.7; g[2] = truth[2] + 0.35; }

inline visfs_scan_stack_params wide_search() {
    visfs_scan_stack_params p;
    visfs_scan_stack_default_params(&p);
    p.linear_search_window = 1.5; p.angular_search_window = 0.5; p.min_score = 0.4;
    return p;
}

struct Summary {
    int inserted = 0, frozen = 0, best = -1, refined = 0, launches = 0, copies = 0, waits = 0, depth_used = 0, num_linear = 0;
    std::vector<double> scores;
    std::vector<int> matched, cells_x;
    double err_before = 0.0, err_closure = 0.0, yaw_err_closure = 0.0, err_refined = 0.0, yaw_err_refined = 0.0, angular_step = 0.0;
    // with `refine`: the members refined in the group call, and the best member's refinement
    std::vector<int> subcell;
    int subcell_iterations = 0;
    double err_subcell = 0.0, yaw_err_subcell = 0.0, cost_before = 0.0, cost_after = 0.0, information_trace = 0.0;
};

// What the two flavours differ in: inserting a frame, whether the front is finished, freezing it, and the local match on the front.
struct Map {
    std::function<int(const double T[12], const std::vector<double>& returns)> insert;
    std::function<bool(int* num_x_cells)> front_finished;
    std::function<VISFS::ScanStack()> freeze_front;
    std::function<int(const double g[3], const std::vector<double>& returns, visfs_scan_match_result* out)> local_match;
};

inline int run(const Map& map, Summary& out, bool refine) {
    Rng rng{ 99 };
    std::vector<VISFS::ScanStack> stacks;
    for (int f = 0; f < kFrames; ++f) {
        double p[3], T[12];
        true_pose(f, p); planar(p[0], p[1], p[2], T);
        if (map.insert(T, scan(p[0], p[1], p[2], 360, rng)) != VISFS_BA_OK) return 1;
        ++out.inserted;
        int nx = 0;
        if (map.front_finished(&nx)) {                                         // finished and cropped: frozen before the next insertion drops it
            stacks.push_back(map.freeze_front());
            out.cells_x.push_back(nx);
        }
    }
    out.frozen = (int)stacks.size();
    if (stacks.empty()) return 1;
    std::vector<const VISFS::ScanStack*> members;
    for (const VISFS::ScanStack& s : stacks) members.push_back(&s);
    const VISFS::ScanStackGroup group(members);
    double truth[3], guess[3];
    true_pose(kFrames, truth); drifted_guess(truth, guess);
    const std::vector<double> ret = scan(truth[0], truth[1], truth[2], 360, rng);
    std::vector<double> guesses;
    for (size_t i = 0; i < stacks.size(); ++i) guesses.insert(guesses.end(), guess, guess + 3);      // loop closure: one world pose for all
    const visfs_scan_stack_params wp = wide_search();
    std::vector<VISFS::ScanStackGroup::Match> ms;
    std::vector<visfs_scan_stack_result> full;
    std::vector<VISFS::RefinedPose> fp;
    // the group call refines towards each member's guess; a loop closure's guess has drifted by a metre, so it gets no weight here
    visfs_scan_refine_params rp;
    visfs_scan_refine_default_params(&rp);
    rp.translation_weight = 0.0;
    int rc = refine ? group.matchRefine(guesses, ret, &ms, &out.best, &fp, &wp, &rp, &full) : group.match(guesses, ret, &ms, &out.best, &wp, &full);
    if (rc != VISFS_BA_OK) { std::fprintf(stderr, "group match failed: %d (%s)\n", rc, group.lastError()); return 1; }
    group.lastCounts(&out.launches, &out.copies, &out.waits);
    for (const VISFS::ScanStackGroup::Match& m : ms) { out.scores.push_back(m.ok ? m.score : -1.0); out.matched.push_back(m.ok && m.matched ? 1 : 0); }
    out.err_before = std::hypot(guess[0] - truth[0], guess[1] - truth[1]);
    if (out.best < 0) return 0;
    const visfs_scan_stack_result& w = full[(size_t)out.best];
    out.depth_used = w.depth_used; out.num_linear = w.match.num_linear; out.angular_step = w.match.angular_step;
    out.err_closure = std::max(std::fabs(w.match.x - truth[0]), std::fabs(w.match.y - truth[1]));
    out.yaw_err_closure = std::fabs(w.match.yaw - truth[2]);
    if (refine) {
        for (const VISFS::RefinedPose& f : fp) out.subcell.push_back(f.refined ? 1 : 0);
        const VISFS::RefinedPose& f = fp[(size_t)out.best];
        out.subcell_iterations = f.iterations; out.cost_before = f.initialCost; out.cost_after = f.finalCost;
        out.information_trace = f.information[0] + f.information[4] + f.information[8];
        out.err_subcell = std::max(std::fabs(f.x - truth[0]), std::fabs(f.y - truth[1]));
        out.yaw_err_subcell = std::fabs(f.yaw - truth[2]);
    }
    const double g2[3] = { w.match.x, w.match.y, w.match.yaw };
    visfs_scan_match_result fine{};
    rc = map.local_match(g2, ret, &fine);
    if (rc != VISFS_BA_OK) { std::fprintf(stderr, "local match failed: %d\n", rc); return 1; }
    out.refined = fine.matched;
    out.err_refined = std::max(std::fabs(fine.x - truth[0]), std::fabs(fine.y - truth[1]));
    out.yaw_err_refined = std::fabs(fine.yaw - truth[2]);
    return 0;
}

// the one-core twins: host sub-maps over the C ABI, host stacks
inline int run_host(Summary& out, bool refine) {
    visfs_submap_params sp;
    visfs_submap_default_params(&sp);
    sp.num_range_data_limit = kLimit;
    visfs_submaps* s = nullptr;
    if (visfs_submaps_create_host(&sp, &s) != VISFS_BA_OK) return 1;
    Map map;
    map.insert = [s](const double T[12], const std::vector<double>& ret) {
        visfs_range_data rd{};
        rd.n_returns = (int32_t)(ret.size() / 3); rd.returns = ret.data();
        return visfs_submaps_insert(s, T, 1, &rd);
    };
    map.front_finished = [s](int* nx) {
        int32_t n = 0;
        visfs_submap_info info[2];
        visfs_submaps_describe(s, &n, info);
        if (n > 0) *nx = info[0].num_x_cells;
        return n > 0 && info[0].finished != 0;
    };
    map.freeze_front = [s]() {
        visfs_scan_stack* st = nullptr;
        if (visfs_scan_stack_create(s, 0, kDepth, &st) != VISFS_BA_OK) std::fprintf(stderr, "freeze failed: %s\n", visfs_submaps_last_error(s));
        return VISFS::ScanStack(st);
    };
    map.local_match = [s](const double g[3], const std::vector<double>& ret, visfs_scan_match_result* r) {
        visfs_scan_match_params lp;
        visfs_scan_match_default_params(&lp);                                  // Cartographer's real-time defaults: 0.1 m, 20 degrees, weighted
        return visfs_scan_match(s, 0, &lp, g, (int32_t)(ret.size() / 3), ret.data(), r);
    };
    const int rc = run(map, out, refine);                                              // the stacks and the group go inside
    visfs_submaps_destroy(s);
    return rc;
}

// the device: VISFS::Map::ActiveSubmaps2D, device stacks and the group's kernels on the handle's stream
inline int run_device(visfs_ba_handle* ba, Summary& out, bool refine) {
    VISFS::Map::ActiveSubmaps2D submaps(ba, kLimit);
    Map map;
    map.insert = [&submaps](const double T[12], const std::vector<double>& ret) {
        std::vector<VISFS::Map::ActiveSubmaps2D::RangeData> rds(1);
        rds[0].returns = ret;
        const int rc = submaps.insertRangeData(rds, T);
        if (rc != VISFS_BA_OK) std::fprintf(stderr, "insert failed: %s\n", submaps.lastError());
        return rc;
    };
    map.front_finished = [&submaps](int* nx) {
        const std::vector<visfs_submap_info> v = submaps.submaps();
        if (!v.empty()) *nx = v[0].num_x_cells;
        return !v.empty() && v[0].finished != 0;
    };
    map.freeze_front = [&submaps]() { return submaps.freeze(0, kDepth); };
    map.local_match = [&submaps](const double g[3], const std::vector<double>& ret, visfs_scan_match_result* r) {
        return submaps.match(g, ret, nullptr, nullptr, 0, r);
    };
    return run(map, out, refine);
}

template <class T> std::string list(const std::vector<T>& v, const char* fmt) {
    std::string s = "[";
    char buf[64];
    for (size_t i = 0; i < v.size(); ++i) { std::snprintf(buf, sizeof buf, fmt, v[i]); s += (i ? ", " : ""); s += buf; }
    return s + "]";
}

}  // namespace loop_closure_step

int main(int argc, char** argv) {
    bool host = false, refine = false;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "host") == 0) host = true;
        else if (std::strcmp(argv[i], "refine") == 0) refine = true;
    }
    loop_closure_step::Summary s;
    int rc;
    try {
    if (host) {
        rc = loop_closure_step::run_host(s, refine);
    } else {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        visfs_ba_handle* ba = nullptr;
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
        rc = loop_closure_step::run_device(ba, s, refine);                             // the group, the stacks and the sub-maps go before the handle
        visfs_ba_destroy(ba);
    }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"inserted\": %d, \"frozen\": %d, \"cells_x\": %s, \"scores\": %s, \"matched\": %s, \"best_member\": %d, "
                "\"depth_used\": %d, \"num_linear\": %d, \"angular_step\": %.6g, \"err_before_m\": %.4g, \"err_closure_m\": %.17g, "
                "\"yaw_err_closure\": %.17g, \"refined\": %d, \"err_refined_m\": %.17g, \"yaw_err_refined\": %.17g, \"launches\": %d, "
                "\"copies\": %d, \"waits\": %d",
                host ? "host" : "device", s.inserted, s.frozen, loop_closure_step::list(s.cells_x, "%d").c_str(),
                loop_closure_step::list(s.scores, "%.17g").c_str(), loop_closure_step::list(s.matched, "%d").c_str(), s.best, s.depth_used,
                s.num_linear, s.angular_step, s.err_before, s.err_closure, s.yaw_err_closure, s.refined, s.err_refined, s.yaw_err_refined,
                s.launches, s.copies, s.waits);
    if (refine)
        std::printf(", \"subcell\": %s, \"subcell_iterations\": %d, \"cost_before\": %.17g, \"cost_after\": %.17g, \"information_trace\": %.17g, "
                    "\"err_subcell_m\": %.17g, \"yaw_err_subcell\": %.17g", loop_closure_step::list(s.subcell, "%d").c_str(), s.subcell_iterations,
                    s.cost_before, s.cost_after, s.information_trace, s.err_subcell, s.yaw_err_subcell);
    std::printf("}\n");
    return 0;
}
