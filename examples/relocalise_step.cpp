// relocalise_step.cpp — a robot that has lost its pose finds it again in the map it built: the matching sub-map is frozen as a grid
// stack (include/visfs_scan_fast.h), the branch-and-bound search recovers the pose from a guess that is off by more than a metre and
// a third of a radian, the weighted correlative match (include/visfs_scan_match.h) settles it locally, and the window solve takes it.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/relocalise_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o relocalise_step && ./relocalise_step [host] [refine]
//
// The room, the pillar and the five inserted frames are those of scan_match_step.cpp.  `host` runs the insertions, the stack and both
// matches on the one-core host twins (no device, no window solve).  `refine` adds the sub-cell refinement of the settled pose on the live
// sub-map (include/visfs_scan_refine.h) and its fields to the output.  Prints one JSON line.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ActiveSubmaps2D.h"
#include "ScanStack.h"
#include "visfs_ba.h"
#include "visfs_scan_fast.h"
#include "visfs_scan_match.h"
#include "visfs_scan_refine.h"

namespace relocalise_step {

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

struct Summary {
    int inserted = 0, matched = 0, refined = 0, solved = 0, num_scans = 0, num_linear = 0, depth_used = 0;
    double err_before = 0.0, err_reloc = 0.0, yaw_err_reloc = 0.0, err_refined = 0.0, yaw_err_refined = 0.0, angular_step = 0.0, score = 0.0,
           solve_err = -1.0;
    // with `refine`: the sub-cell refinement of the settled pose
    int subcell = 0, subcell_iterations = 0;
    double err_subcell = 0.0, yaw_err_subcell = 0.0, cost_before = 0.0, cost_after = 0.0;
};

inline void report_subcell(const double truth[3], const visfs_scan_refine_result& f, Summary& out) {
    out.subcell = f.refined; out.subcell_iterations = f.iterations; out.cost_before = f.initial_cost; out.cost_after = f.final_cost;
    out.err_subcell = std::max(std::fabs(f.x - truth[0]), std::fabs(f.y - truth[1]));
    out.yaw_err_subcell = std::fabs(f.yaw - truth[2]);
}

constexpr int kFrames = 5;
constexpr int kDepth = 7;
inline void true_pose(int f, double p[3]) { p[0] = -0.6 + 0.15 * f; p[1] = 0.2 + 0.04 * f; p[2] = 0.1 * f; }
// the pose is thrown away: what is left is off by (1.1 m, -0.7 m, 0.35 rad)
inline void lost_guess(const double truth[3], double g[3]) { g[0] = truth[0] + 1.1; g[1] = truth[1] - 0.7; g[2] = truth[2] + 0.35; }

inline visfs_scan_stack_params wide_search() {
    visfs_scan_stack_params p;
    visfs_scan_stack_default_params(&p);
    p.linear_search_window = 1.5; p.angular_search_window = 0.5; p.min_score = 0.4;
    return p;
}

inline visfs_scan_match_params local_search() {                                // Cartographer's real-time defaults: 0.1 m, 20 degrees, weighted
    visfs_scan_match_params p;
    visfs_scan_match_default_params(&p);
    return p;
}

inline void report(const double truth[3], const double guess[3], const visfs_scan_stack_result& r, const visfs_scan_match_result& fine, Summary& out) {
    out.matched = r.match.matched; out.score = r.match.score; out.num_scans = r.match.num_scans; out.num_linear = r.match.num_linear;
    out.angular_step = r.match.angular_step; out.depth_used = r.depth_used;
    out.err_before = std::hypot(guess[0] - truth[0], guess[1] - truth[1]);
    out.err_reloc = std::max(std::fabs(r.match.x - truth[0]), std::fabs(r.match.y - truth[1]));
    out.yaw_err_reloc = std::fabs(r.match.yaw - truth[2]);
    out.refined = fine.matched;
    out.err_refined = std::max(std::fabs(fine.x - truth[0]), std::fabs(fine.y - truth[1]));
    out.yaw_err_refined = std::fabs(fine.yaw - truth[2]);
}

// the one-core twins: host sub-maps and a host stack over the C ABI
inline int run_host(Summary& out, bool refine) {
    visfs_submap_params sp;
    visfs_submap_default_params(&sp);
    visfs_submaps* s = nullptr;
    if (visfs_submaps_create_host(&sp, &s) != VISFS_BA_OK) return 1;
    Rng rng{ 99 };
    for (int f = 0; f < kFrames; ++f) {
        double p[3], T[12];
        true_pose(f, p); planar(p[0], p[1], p[2], T);
        const std::vector<double> ret = scan(p[0], p[1], p[2], 360, rng);
        visfs_range_data rd{};
        rd.n_returns = (int32_t)(ret.size() / 3); rd.returns = ret.data();
        if (visfs_submaps_insert(s, T, 1, &rd) != VISFS_BA_OK) { visfs_submaps_destroy(s); return 1; }
        ++out.inserted;
    }
    visfs_scan_stack* st = nullptr;
    if (visfs_scan_stack_create(s, 0, kDepth, &st) != VISFS_BA_OK) { std::fprintf(stderr, "freeze failed: %s\n", visfs_submaps_last_error(s)); visfs_submaps_destroy(s); return 1; }
    double truth[3], guess[3];
    true_pose(kFrames, truth); lost_guess(truth, guess);
    const std::vector<double> ret = scan(truth[0], truth[1], truth[2], 360, rng);
    const int32_t n = (int32_t)(ret.size() / 3);
    const visfs_scan_stack_params wp = wide_search();
    visfs_scan_stack_result r;
    int rc = visfs_scan_stack_match(st, &wp, guess, n, ret.data(), &r);
    if (rc != VISFS_BA_OK) std::fprintf(stderr, "relocalisation failed: %d (%s)\n", rc, visfs_scan_stack_last_error(st));
    visfs_scan_match_result fine{};
    if (rc == VISFS_BA_OK) {
        const visfs_scan_match_params lp = local_search();
        const double g2[3] = { r.match.x, r.match.y, r.match.yaw };
        rc = visfs_scan_match(s, 0, &lp, g2, n, ret.data(), &fine);
        if (rc != VISFS_BA_OK) std::fprintf(stderr, "local match failed: %d (%s)\n", rc, visfs_submaps_last_error(s));
    }
    if (rc == VISFS_BA_OK) report(truth, guess, r, fine, out);
    if (rc == VISFS_BA_OK && refine) {                                         // from the settled pose, held to its translation
        visfs_scan_refine_params rp;
        visfs_scan_refine_default_params(&rp);
        const double a[3] = { fine.x, fine.y, fine.yaw };
        visfs_scan_refine_result f;
        rc = visfs_scan_refine(s, 0, &rp, a, a, n, ret.data(), &f);
        if (rc != VISFS_BA_OK) std::fprintf(stderr, "refinement failed: %d (%s)\n", rc, visfs_submaps_last_error(s));
        else report_subcell(truth, f, out);
    }
    visfs_scan_stack_destroy(st);
    visfs_submaps_destroy(s);
    return rc == VISFS_BA_OK ? 0 : 1;
}

// relative transform A^-1 B of two 3x4 poses
inline void rel(const double A[12], const double B[12], double out[12]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = A[r] * B[c] + A[4 + r] * B[4 + c] + A[8 + r] * B[8 + c];
        out[4 * r + 3] = A[r] * (B[3] - A[3]) + A[4 + r] * (B[7] - A[7]) + A[8 + r] * (B[11] - A[11]);
    }
}

// the device: VISFS::Map::ActiveSubmaps2D and VISFS::ScanStack on the handle's stream, the recovered pose handed to the window solve
inline int run_device(visfs_ba_handle* ba, Summary& out, bool refine) {
    VISFS::Map::ActiveSubmaps2D submaps(ba);
    Rng rng{ 99 };
    std::vector<uint64_t> ids;
    std::vector<double> est, truthT;                                           // [pose][12]
    for (int f = 0; f < kFrames; ++f) {
        double p[3], T[12];
        true_pose(f, p); planar(p[0], p[1], p[2], T);
        std::vector<VISFS::Map::ActiveSubmaps2D::RangeData> rds(1);
        rds[0].returns = scan(p[0], p[1], p[2], 360, rng);
        if (submaps.insertRangeData(rds, T) != VISFS_BA_OK) { std::fprintf(stderr, "insert failed: %s\n", submaps.lastError()); return 1; }
        ++out.inserted;
        if (f >= kFrames - 2) { ids.push_back((uint64_t)f + 1); est.insert(est.end(), T, T + 12); truthT.insert(truthT.end(), T, T + 12); }
    }
    const VISFS::ScanStack stack = submaps.freeze(0, kDepth);                  // right after the insertions: device to device
    double truth[3], guess[3], Tt[12];
    true_pose(kFrames, truth); planar(truth[0], truth[1], truth[2], Tt); lost_guess(truth, guess);
    const std::vector<double> ret = scan(truth[0], truth[1], truth[2], 360, rng);
    const visfs_scan_stack_params wp = wide_search();
    VISFS::ScanStack::Match wide;
    visfs_scan_stack_result r;
    int rc = stack.match(guess, ret, &wide, &wp, &r);
    if (rc != VISFS_BA_OK) { std::fprintf(stderr, "relocalisation failed: %d (%s)\n", rc, stack.lastError()); return 1; }
    const visfs_scan_match_params lp = local_search();
    const double g2[3] = { wide.x, wide.y, wide.yaw };
    VISFS::Map::ActiveSubmaps2D::Match m;
    visfs_scan_match_result fine;
    rc = submaps.match(g2, ret, &m, &lp, 0, &fine);
    if (rc != VISFS_BA_OK) { std::fprintf(stderr, "local match failed: %d (%s)\n", rc, submaps.lastError()); return 1; }
    report(truth, guess, r, fine, out);
    if (refine) {
        const double a[3] = { m.x, m.y, m.yaw };
        visfs_scan_refine_result f;
        rc = submaps.refine(a, a, ret, nullptr, nullptr, 0, &f);
        if (rc != VISFS_BA_OK) { std::fprintf(stderr, "refinement failed: %d (%s)\n", rc, submaps.lastError()); return 1; }
        report_subcell(truth, f, out);
    }
    // the window: the last two inserted poses and the new one at the recovered pose, odometry links from the true motion
    double Tn[12];
    planar(m.x, m.y, m.yaw, Tn);
    ids.push_back((uint64_t)kFrames + 1); est.insert(est.end(), Tn, Tn + 12); truthT.insert(truthT.end(), Tt, Tt + 12);
    const int n = (int)ids.size();
    std::vector<uint64_t> lf, lt;
    std::vector<double> lT;
    for (int i = 0; i + 1 < n; ++i) {
        double d[12];
        rel(&truthT[12 * i], &truthT[12 * (i + 1)], d);
        lf.push_back(ids[i]); lt.push_back(ids[i + 1]); lT.insert(lT.end(), d, d + 12);
    }
    visfs_ba_window w{};
    w.root_id = ids.front();
    w.n_poses = n; w.pose_ids = ids.data(); w.pose_Twr = est.data();
    w.n_links = (int32_t)lf.size(); w.link_from = lf.data(); w.link_to = lt.data(); w.link_T = lT.data();
    w.n_cameras = 1; w.fx = w.fy = 400; w.cx = 320; w.cy = 240;
    const double Trc[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };
    for (int i = 0; i < 12; ++i) w.Trc[i] = Trc[i];
    w.n_laser_points = (int32_t)(ret.size() / 3); w.laser_xyz = ret.data();
    std::vector<uint64_t> pid(n);
    std::vector<double> pT(12 * (size_t)n);
    visfs_ba_result res{};
    res.pose_ids_out = pid.data(); res.pose_Twr_out = pT.data();
    const int rs = submaps.solveWindow(&w, &res);
    if (rs != VISFS_BA_OK && rs != VISFS_BA_PASSTHROUGH) { std::fprintf(stderr, "solve failed: %d\n", rs); return 1; }
    if (rs == VISFS_BA_OK && res.n_poses_out == n) {
        out.solved = 1;
        const double* Tl = &pT[12 * (size_t)(n - 1)];
        out.solve_err = std::hypot(Tl[3] - truth[0], Tl[7] - truth[1]);
    }
    return 0;
}

}  // namespace relocalise_step

int main(int argc, char** argv) {
    bool host = false, refine = false;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "host") == 0) host = true;
        else if (std::strcmp(argv[i], "refine") == 0) refine = true;
    }
    relocalise_step::Summary s;
    int rc;
    if (host) {
        rc = relocalise_step::run_host(s, refine);
    } else {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        visfs_ba_handle* ba = nullptr;
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
        rc = relocalise_step::run_device(ba, s, refine);                               // the stack and the sub-maps go before the handle
        visfs_ba_destroy(ba);
    }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"inserted\": %d, \"matched\": %d, \"depth_used\": %d, \"num_scans\": %d, \"num_linear\": %d, \"angular_step\": %.6g, "
                "\"score\": %.17g, \"err_before_m\": %.4g, \"err_reloc_m\": %.17g, \"yaw_err_reloc\": %.17g, \"refined\": %d, \"err_refined_m\": %.17g, "
                "\"yaw_err_refined\": %.17g, \"solved\": %d, \"solve_err_m\": %.4g",
                host ? "host" : "device", s.inserted, s.matched, s.depth_used, s.num_scans, s.num_linear, s.angular_step, s.score, s.err_before,
                s.err_reloc, s.yaw_err_reloc, s.refined, s.err_refined, s.yaw_err_refined, s.solved, s.solve_err);
    if (refine)
        std::printf(", \"subcell\": %d, \"subcell_iterations\": %d, \"cost_before\": %.17g, \"cost_after\": %.17g, \"err_subcell_m\": %.17g, "
                    "\"yaw_err_subcell\": %.17g", s.subcell, s.subcell_iterations, s.cost_before, s.cost_after, s.err_subcell, s.yaw_err_subcell);
    std::printf("}\n");
    return 0;
}
