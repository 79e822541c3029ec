// pnp_step.cpp — the pose guess of a VISFS frame on the C ABIs of this repository: per frame, VISFS::estimateMotion3DTo2D
// (visfs_amd/host/MotionEstimator.h over include/visfs_pnp.h) from the 3-D words of the frame before and the key-points of this
// frame, as Estimator::process calls it without wheel odometry (Estimator.cpp:187-190); the pose it gives is chained and handed to the
// sliding-window container (visfs_window_insert) with the frame's words.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/pnp_step.cpp -Lvisfs_amd/lib -lvisfs_window -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o pnp_step && ./pnp_step 5 [prefix]
//
// Words only, no images: a cloud of landmarks in front of a robot that drives forward on a gentle curve; every frame sees the
// landmarks in its image with 0.3 px of pixel noise, and one word in seven is a wrong match 30 px away.  With a prefix, the words
// of every frame are also written as <prefix>_<frame>.txt (id, then u v u_right v_right x y z), so a test can run the same frames
// elsewhere.  Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "MotionEstimator.h"
#include "visfs_window.h"

namespace pnp_step {

struct Lcg {                                             // a tiny generator, so the scene is the same everywhere
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double range(double a, double b) { return a + (b - a) * next(); }
};

struct Word { float u, v, ur, vr, x, y, z; };

struct WindowGuard {
    visfs_window_map* map = nullptr;
    WindowGuard() = default;
    WindowGuard(const WindowGuard&) = delete;
    WindowGuard& operator=(const WindowGuard&) = delete;
    ~WindowGuard() { if (map) visfs_window_destroy(map); }
};

struct Summary {
    int frames = 0, inserted = 0;
    std::vector<int> matches;
    std::vector<std::vector<std::size_t>> inliers;
    std::vector<VISFS::PnpTransform> transforms;
    double max_rot_err = 0.0, max_trans_err = 0.0, ms = 0.0;
};

// The true pose of frame f in the world, 3x4 row-major: forward along x with a slow yaw and a little sway.
inline void truePose(int f, double T[12]) {
    const double yaw = 0.03 * f, c = std::cos(yaw), s = std::sin(yaw);
    const double t[3] = { 0.25 * f, 0.04 * f * f, 0.01 * f };
    const double R[9] = { c, -s, 0, s, c, 0, 0, 0, 1 };
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) T[4 * r + k] = R[3 * r + k]; T[4 * r + 3] = t[r]; }
}
inline void invert(const double A[12], double C[12]) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[4 * r + c] = A[4 * c + r];
    for (int r = 0; r < 3; ++r) C[4 * r + 3] = -(C[4 * r] * A[3] + C[4 * r + 1] * A[7] + C[4 * r + 2] * A[11]);
}
inline void mul(const double A[12], const double B[12], double C[12]) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) C[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c];
        C[4 * r + 3] = A[4 * r] * B[3] + A[4 * r + 1] * B[7] + A[4 * r + 2] * B[11] + A[4 * r + 3];
    }
}
inline void apply(const double A[12], const double p[3], double o[3]) {
    for (int r = 0; r < 3; ++r) o[r] = A[4 * r] * p[0] + A[4 * r + 1] * p[1] + A[4 * r + 2] * p[2] + A[4 * r + 3];
}

inline int run(int frames, visfs_ba_handle* ba, const std::string& dump, Summary& out) {
    const int W = 752, H = 480, nLandmarks = 400;
    const double fx = 435.2, fy = 435.2, cx = 367.4, cy = 252.2, baseline = 0.11;
    const int minInliers = 12, iterations = 50, refineIterations = 5;       // Estimator/MinInliers, PnPIterations, RefineIterations
    const double reProjError = 2.0;                                          // Estimator/PnPReprojError
    visfs_pnp_camera cam{};
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    const double Tir[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };
    for (int i = 0; i < 12; ++i) cam.Tir[i] = Tir[i];
    double Tri[12];
    invert(Tir, Tri);
    VISFS::MotionEstimator estimator(ba, 1024);
    WindowGuard guard;
    if (visfs_window_create(0, nullptr, nullptr, &guard.map) != VISFS_BA_OK) return 2;
    Lcg rng{ 2024 };
    std::vector<double> landmarks;
    for (int i = 0; i < nLandmarks; ++i) {
        landmarks.push_back(rng.range(2.0, 11.0)); landmarks.push_back(rng.range(-5.0, 5.0)); landmarks.push_back(rng.range(-2.0, 2.5));
    }
    std::map<std::size_t, VISFS::PnpPoint3f> words3dBefore;
    double pose[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 }, truthBefore[12];
    truePose(0, truthBefore);
    for (int f = 0; f < frames; ++f) {
        double Twr[12], Trw[12];
        truePose(f, Twr);
        invert(Twr, Trw);
        std::map<std::size_t, Word> words;
        for (int i = 0; i < nLandmarks; ++i) {
            double pr[3], pc[3];
            apply(Trw, &landmarks[3 * (size_t)i], pr);
            apply(Tri, pr, pc);
            if (pc[2] < 0.5) continue;
            double u = fx * pc[0] / pc[2] + cx + rng.range(-0.5, 0.5), v = fy * pc[1] / pc[2] + cy + rng.range(-0.5, 0.5);
            if ((i + f) % 7 == 3) { const double a = rng.range(0.0, 6.2831853); u += 30.0 * std::cos(a); v += 30.0 * std::sin(a); }
            if (!(u >= 0 && u < W && v >= 0 && v < H)) continue;
            const double disparity = fx * baseline / pc[2];
            words[(std::size_t)i + 1] = Word{ (float)u, (float)v, (float)(u - disparity), (float)v, (float)pr[0], (float)pr[1], (float)pr[2] };
        }
        if (!dump.empty()) {
            std::FILE* fp = std::fopen((dump + "_" + std::to_string(f) + ".txt").c_str(), "w");
            if (!fp) { std::fprintf(stderr, "cannot write the words\n"); return 5; }
            for (const auto& kv : words)
                std::fprintf(fp, "%zu %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", kv.first, kv.second.u, kv.second.v, kv.second.ur, kv.second.vr,
                             kv.second.x, kv.second.y, kv.second.z);
            if (std::fclose(fp) != 0) return 5;
        }
        std::map<std::size_t, VISFS::PnpKeyPoint> words2d;
        std::map<std::size_t, VISFS::PnpPoint3f> words3d;
        for (const auto& kv : words) {
            words2d[kv.first] = VISFS::PnpKeyPoint{ { kv.second.u, kv.second.v } };
            words3d[kv.first] = VISFS::PnpPoint3f{ kv.second.x, kv.second.y, kv.second.z };
        }
        double translation[3] = { 0, 0, 0 };
        if (f > 0) {                                                          // Estimator.cpp:187-190
            VISFS::PnpCovariance covariance;
            std::vector<std::size_t> matches, inliers;
            const auto t0 = std::chrono::steady_clock::now();
            const VISFS::PnpTransform T = VISFS::estimateMotion3DTo2D(estimator.get(), words3dBefore, words2d, cam, minInliers, iterations,
                                                                      reProjError, 0, refineIterations, words3d, covariance, matches, inliers);
            out.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (T[15] == 0.0) { std::fprintf(stderr, "frame %d: no motion found\n", f); return 4; }
            out.matches.push_back((int)matches.size());
            out.inliers.push_back(inliers);
            out.transforms.push_back(T);
            double truth[12], inv[12], next[12];                              // the true motion: frame f seen from frame f - 1
            invert(truthBefore, inv);
            mul(inv, Twr, truth);
            double tr = 0.0, dt = 0.0;
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) tr += truth[4 * r + c] * T[4 * (size_t)r + c];
                dt += (truth[4 * r + 3] - T[4 * (size_t)r + 3]) * (truth[4 * r + 3] - T[4 * (size_t)r + 3]);
                translation[r] = T[4 * (size_t)r + 3];
            }
            out.max_rot_err = std::fmax(out.max_rot_err, std::acos(std::fmin(1.0, std::fmax(-1.0, 0.5 * (tr - 1.0)))));
            out.max_trans_err = std::fmax(out.max_trans_err, std::sqrt(dt));
            mul(pose, T.data(), next);
            for (int i = 0; i < 12; ++i) pose[i] = next[i];
        }
        std::vector<uint64_t> wid;
        std::vector<float> uv, p3;
        std::vector<uint8_t> has3d;
        for (const auto& kv : words) {
            wid.push_back((uint64_t)kv.first);
            uv.insert(uv.end(), { kv.second.u, kv.second.v, kv.second.ur, kv.second.vr });
            p3.insert(p3.end(), { kv.second.x, kv.second.y, kv.second.z });
            has3d.push_back(1);
        }
        const double wheel[12] = { 0 };
        const int rc = visfs_window_insert(guard.map, (uint64_t)f + 1, pose, wheel, translation, (int32_t)wid.size(), wid.data(), uv.data(),
                                           p3.data(), has3d.data(), 0, nullptr, nullptr);
        if (rc != 1) { std::fprintf(stderr, "insert refused: %d\n", rc); return 4; }
        ++out.inserted;
        ++out.frames;
        words3dBefore.swap(words3d);
        for (int i = 0; i < 12; ++i) truthBefore[i] = Twr[i];
    }
    return 0;
}

}  // namespace pnp_step

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 5;
    const std::string dump = argc > 2 ? argv[2] : "";
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    pnp_step::Summary s;
    int rc;
    try { rc = pnp_step::run(frames, ba, dump, s); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::string matches = "[", inliers = "[", transforms = "[";
    for (size_t k = 0; k < s.matches.size(); ++k) {
        matches += (k ? ", " : "") + std::to_string(s.matches[k]);
        inliers += k ? ", [" : "[";
        for (size_t i = 0; i < s.inliers[k].size(); ++i) inliers += (i ? ", " : "") + std::to_string(s.inliers[k][i]);
        inliers += "]";
        transforms += k ? ", [" : "[";
        for (size_t i = 0; i < 16; ++i) { char buf[40]; std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", s.transforms[k][i]); transforms += buf; }
        transforms += "]";
    }
    std::printf("{\"frames\": %d, \"inserted\": %d, \"matches\": %s], \"inliers\": %s], \"transforms\": %s], \"max_rot_err_rad\": %.4g, "
                "\"max_trans_err_m\": %.4g, \"pnp_ms\": %.3f}\n",
                s.frames, s.inserted, matches.c_str(), inliers.c_str(), transforms.c_str(), s.max_rot_err, s.max_trans_err, s.ms);
    return 0;
}
