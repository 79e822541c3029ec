// tracker_step.cpp — the image front end of one VISFS frame on the C ABIs of this repository: synthetic stereo frames go through
// VISFS::FlowTracker (Tracker::imageProcess's optical flow and triangulation, Tracker.cpp:233-388) and the words that survive go into
// the sliding-window container (visfs_window_insert), which is what Estimator hands to the BA.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/tracker_step.cpp -Lvisfs_amd/lib -lvisfs_window -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o tracker_step && ./tracker_step 4
//
// A stereo camera slides sideways in front of a textured wall 5 m away (a sum of sinusoids, sampled analytically), so the true flow
// and disparity are known.  Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "FlowTracker.h"
#include "visfs_ba.h"
#include "visfs_window.h"

namespace tracker_step {

struct Rng {                      // SplitMix64 -> uniform
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct Texture {
    std::vector<double> kx, ky, ph, amp;
    explicit Texture(uint64_t seed, int n = 48) {
        Rng rng{ seed };
        double power = 0.0;
        for (int i = 0; i < n; ++i) {
            const double lam = std::exp(std::log(6.0) + rng.uni() * (std::log(60.0) - std::log(6.0))), th = 6.283185307179586 * rng.uni();
            kx.push_back(6.283185307179586 / lam * std::cos(th)); ky.push_back(6.283185307179586 / lam * std::sin(th));
            ph.push_back(6.283185307179586 * rng.uni()); amp.push_back(lam);
            power += 0.5 * lam * lam;
        }
        for (double& a : amp) a *= 40.0 / std::sqrt(power);
    }
    // the image whose pixel (x, y) shows the wall at (x + dx, y)
    std::vector<uint8_t> image(int w, int h, double dx) const {
        std::vector<uint8_t> img((size_t)w * h);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                double v = 128.0;
                for (size_t k = 0; k < kx.size(); ++k) v += amp[k] * std::cos(kx[k] * (x + dx) + ky[k] * y + ph[k]);
                img[(size_t)y * w + x] = (uint8_t)std::lround(std::fmin(std::fmax(v, 0.0), 255.0));
            }
        return img;
    }
};

struct Summary { int frames = 0, words = 0, tracked = 0, inserted = 0; double max_flow_err = 0.0, max_depth_err = 0.0, ms = 0.0; };

inline int run(int frames, visfs_ba_handle* ba, Summary& out) {
    const int W = 640, H = 400;
    const float fx = 435.2f, baseline = 0.11f;
    const double depth = 5.0, step = 0.06;                                      // metres per frame to the right: flow = -fx * step / depth
    const double disparity = (double)fx * baseline / depth, flow = -(double)fx * step / depth;
    visfs_flow_camera cam{};
    cam.fx = cam.fy = fx; cam.cx = cam.cx_right = 0.5f * W; cam.cy = 0.5f * H; cam.baseline = baseline;
    const double Tir[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };            // image -> robot
    for (int i = 0; i < 12; ++i) cam.Tir[i] = Tir[i];
    VISFS::FlowTracker tracker(ba, W, H);
    visfs_window_map* window = nullptr;
    if (visfs_window_create(0, nullptr, nullptr, &window) != VISFS_BA_OK) return 2;
    const Texture wall(2024);
    using P2 = VISFS::FlowTracker::Point2f;
    std::vector<P2> corners;                                                    // the words' key-points in the newest left image
    std::vector<uint64_t> ids;
    for (int j = 0; j < 15; ++j)
        for (int i = 0; i < 20; ++i) { corners.push_back(P2{ 60.0f + 27.5f * i, 50.0f + 21.25f * j }); ids.push_back(ids.size() + 1); }
    double ms = 0.0;
    for (int f = 1; f <= frames; ++f) {
        // the wall slides by `flow` px per frame in the left image; the right camera sees it `disparity` px further left
        const std::vector<uint8_t> left = wall.image(W, H, -flow * (f - 1)), right = wall.image(W, H, -flow * (f - 1) + disparity);
        const auto t0 = std::chrono::steady_clock::now();
        if (tracker.pushFrame(left.data(), right.data(), W) != VISFS_BA_OK) { std::fprintf(stderr, "push failed: %s\n", tracker.lastError()); return 1; }
        std::vector<uint64_t> covIds;
        std::vector<float> covUv;
        if (f > 1) {                                                            // Tracker.cpp:257-301
            std::vector<P2> to;
            std::vector<unsigned char> status;
            if (tracker.track(corners, to, status) != VISFS_BA_OK) { std::fprintf(stderr, "track failed: %s\n", tracker.lastError()); return 1; }
            std::vector<P2> kept;
            std::vector<uint64_t> keptIds;
            for (size_t i = 0; i < to.size(); ++i) {
                if (!status[i] || !(to[i].x >= 0.f && to[i].x < (float)W && to[i].y >= 0.f && to[i].y < (float)H)) continue;
                out.max_flow_err = std::fmax(out.max_flow_err, std::hypot(to[i].x - (corners[i].x + flow), to[i].y - corners[i].y));
                covIds.push_back(ids[i]); covUv.push_back(corners[i].x); covUv.push_back(corners[i].y);
                kept.push_back(to[i]); keptIds.push_back(ids[i]);
            }
            out.tracked += (int)kept.size();
            corners.swap(kept); ids.swap(keptIds);
        }
        std::vector<P2> rightPts;                                               // Tracker.cpp:354-388
        std::vector<unsigned char> status;
        std::vector<VISFS::FlowTracker::Point3f> xyz;
        if (tracker.stereo(corners, cam, rightPts, status, xyz) != VISFS_BA_OK) { std::fprintf(stderr, "stereo failed: %s\n", tracker.lastError()); return 1; }
        ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::vector<uint64_t> wid;
        std::vector<float> uv, p3;
        std::vector<uint8_t> has3d;
        for (size_t i = 0; i < corners.size(); ++i) {
            if (!status[i] || !(rightPts[i].x >= 0.f && rightPts[i].x < (float)W)) continue;
            wid.push_back(ids[i]);
            uv.insert(uv.end(), { corners[i].x, corners[i].y, rightPts[i].x, rightPts[i].y });
            p3.insert(p3.end(), { xyz[i].x, xyz[i].y, xyz[i].z });
            has3d.push_back(std::isfinite(xyz[i].x) ? 1 : 0);
            if (has3d.back()) out.max_depth_err = std::fmax(out.max_depth_err, std::fabs(xyz[i].x - depth));
        }
        out.words += (int)wid.size();
        const double Twr[12] = { 1, 0, 0, 0, 0, 1, 0, -step * (f - 1), 0, 0, 1, 0 };   // sideways: the robot's -y is the image's +x
        const double wheel[12] = { 0 }, translation[3] = { 0, -step, 0 };
        const int rc = visfs_window_insert(window, (uint64_t)f, Twr, wheel, translation, (int32_t)wid.size(), wid.data(), uv.data(), p3.data(),
                                           has3d.data(), (int32_t)covIds.size(), covIds.data(), covUv.data());
        if (rc != 1) { std::fprintf(stderr, "insert refused: %d\n", rc); return 4; }
        ++out.inserted;
        ++out.frames;
    }
    out.ms = ms;
    visfs_window_destroy(window);
    return 0;
}

}  // namespace tracker_step

#ifndef TRACKER_STEP_NO_MAIN
int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 4;
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    tracker_step::Summary s;
    int rc;
    try { rc = tracker_step::run(frames, ba, s); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::printf("{\"frames\": %d, \"words\": %d, \"tracked\": %d, \"inserted\": %d, \"max_flow_err_px\": %.4g, \"max_depth_err_m\": %.4g, \"flow_ms\": %.2f}\n",
                s.frames, s.words, s.tracked, s.inserted, s.max_flow_err, s.max_depth_err, s.ms);
    return 0;
}
#endif
