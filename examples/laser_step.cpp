// laser_step.cpp — one frame of the laser sensor strategies (4/5) of VISFS's estimator on the C ABIs of this repository: the
// sliding-window BA reads the matching sub-map resident on the GPU (Estimator.cpp:247-250), then the frame's range data go into the
// sub-maps at the optimised pose (Estimator.cpp:377-388 -> LocalMap::insertMatchingSubMap2d).
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/laser_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o laser_step && ./laser_step 20
//
// A robot drives through a 20 m x 12 m room with a planar laser (720 returns per scan, two range data per frame) and noisy wheel
// odometry; the window holds the last six poses (the newest one free, anchored to the laser).  Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ActiveSubmaps2D.h"
#include "visfs_ba.h"

namespace laser_step {

struct Rng {                      // SplitMix64 -> uniform / normal
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
    double normal() { const double u = uni() + 1e-300, v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

struct Summary { int frames = 0, solved = 0, submaps = 0, front_range_data = 0; double last_chi2 = 0.0, max_err = 0.0, ms = 0.0; };

inline void planar(double x, double y, double yaw, double T[12]) {
    const double c = std::cos(yaw), s = std::sin(yaw);
    const double v[12] = { c, -s, 0, x, s, c, 0, y, 0, 0, 1, 0 };
    for (int i = 0; i < 12; ++i) T[i] = v[i];
}

// returns on the walls of the room [x0, x1] x [y0, y1], in the robot frame of the planar pose (x, y, yaw)
inline VISFS::Map::ActiveSubmaps2D::RangeData scan(double x, double y, double yaw, int n, double phase, Rng& rng) {
    const double x0 = -10, x1 = 10, y0 = -6, y1 = 6;
    VISFS::Map::ActiveSubmaps2D::RangeData rd;
    for (int i = 0; i < n; ++i) {
        const double a = 6.283185307179586 * (i + phase) / n, dx = std::cos(a), dy = std::sin(a);
        const double tx = dx > 0 ? (x1 - x) / dx : (x0 - x) / dx, ty = dy > 0 ? (y1 - y) / dy : (y0 - y) / dy;
        const double r = std::min(std::min(tx, ty) + 0.005 * rng.normal(), 30.0);
        const double wx = r * dx, wy = r * dy, c = std::cos(yaw), s = std::sin(yaw);
        rd.returns.insert(rd.returns.end(), { c * wx + s * wy, -s * wx + c * wy, 0.0 });
    }
    return rd;
}

// relative transform A^-1 B of two 3x4 poses
inline void rel(const double A[12], const double B[12], double out[12]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * r + c] = A[r] * B[c] + A[4 + r] * B[4 + c] + A[8 + r] * B[8 + c];
        out[4 * r + 3] = A[r] * (B[3] - A[3]) + A[4 + r] * (B[7] - A[7]) + A[8 + r] * (B[11] - A[11]);
    }
}

inline int run(int frames, visfs_ba_handle* ba, Summary& out) {
    VISFS::Map::ActiveSubmaps2D submaps(ba, 10);                               // LocalMap/NumRangeDataLimit 10: the life cycle within a short run
    Rng rng{ 777 };
    std::vector<uint64_t> ids;
    std::vector<double> est, truth;                                            // [pose][12]
    const auto t0 = std::chrono::steady_clock::now();
    for (int f = 1; f <= frames; ++f) {
        const double a = 0.15 * f, x = 5.0 * std::cos(a), y = 3.0 * std::sin(a), yaw = a + 1.5707963267948966;
        double T[12], Tn[12];
        planar(x, y, yaw, T);
        planar(x + 0.03 * rng.normal(), y + 0.03 * rng.normal(), yaw + 0.01 * rng.normal(), Tn);   // odometry-propagated guess
        ids.push_back((uint64_t)f);
        truth.insert(truth.end(), T, T + 12);
        est.insert(est.end(), Tn, Tn + 12);
        if (ids.size() > 6) { ids.erase(ids.begin()); est.erase(est.begin(), est.begin() + 12); truth.erase(truth.begin(), truth.begin() + 12); }
        std::vector<VISFS::Map::ActiveSubmaps2D::RangeData> rds = { scan(x, y, yaw, 720, 0.25, rng), scan(x, y, yaw, 720, 0.75, rng) };
        const int n = (int)ids.size();
        // the window: poses, odometry links between neighbours (from the true motion), the newest scan's returns
        std::vector<uint64_t> lf, lt;
        std::vector<double> lT;
        for (int i = 0; i + 1 < n; ++i) {
            double d[12];
            rel(&truth[12 * i], &truth[12 * (i + 1)], d);
            lf.push_back(ids[i]); lt.push_back(ids[i + 1]); lT.insert(lT.end(), d, d + 12);
        }
        std::vector<double> pts;
        for (const auto& rd : rds) pts.insert(pts.end(), rd.returns.begin(), rd.returns.end());
        visfs_ba_window w{};
        w.root_id = ids.front();
        w.n_poses = n; w.pose_ids = ids.data(); w.pose_Twr = est.data();
        w.n_links = (int32_t)lf.size(); w.link_from = lf.data(); w.link_to = lt.data(); w.link_T = lT.data();
        w.n_cameras = 1; w.fx = w.fy = 400; w.cx = 320; w.cy = 240;
        const double Trc[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };
        for (int i = 0; i < 12; ++i) w.Trc[i] = Trc[i];
        w.n_laser_points = (int32_t)(pts.size() / 3); w.laser_xyz = pts.data();
        std::vector<uint64_t> pid(n);
        std::vector<double> pT(12 * (size_t)n);
        visfs_ba_result r{};
        r.pose_ids_out = pid.data(); r.pose_Twr_out = pT.data();
        const double* Tins = Tn;
        if (n >= 2) {
            const int rc = submaps.solveWindow(&w, &r);                        // reads getMatchingSubmap2D() on the device
            if (rc != VISFS_BA_OK && rc != VISFS_BA_PASSTHROUGH) { std::fprintf(stderr, "solve failed: %d\n", rc); return rc; }
            if (rc == VISFS_BA_OK && r.n_poses_out == n) {
                ++out.solved;
                out.last_chi2 = r.chi2_final;
                for (int i = 0; i < 12 * n; ++i) est[i] = pT[i];
                Tins = &est[12 * (n - 1)];
                out.max_err = std::max(out.max_err, std::hypot(Tins[3] - x, Tins[7] - y));
            }
        }
        const int rc = submaps.insertRangeData(rds, Tins);                     // at the optimised pose
        if (rc != VISFS_BA_OK) { std::fprintf(stderr, "insert failed: %d (%s)\n", rc, submaps.lastError()); return rc; }
        ++out.frames;
    }
    out.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    const auto s = submaps.submaps();
    out.submaps = (int)s.size();
    out.front_range_data = s.empty() ? 0 : s.front().num_range_data;
    return 0;
}

}  // namespace laser_step

#ifndef LASER_STEP_NO_MAIN
int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 20;
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    laser_step::Summary s;
    const int rc = laser_step::run(frames, ba, s);
    visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::printf("{\"frames\": %d, \"solved\": %d, \"submaps\": %d, \"front_range_data\": %d, \"last_chi2\": %.6g, \"max_err_m\": %.4g, \"ms\": %.2f}\n",
                s.frames, s.solved, s.submaps, s.front_range_data, s.last_chi2, s.max_err, s.ms);
    return 0;
}
#endif
