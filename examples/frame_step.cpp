// frame_step.cpp — one VISFS frame from the images to the window on the C ABIs of this repository: synthetic stereo frames go
// through VISFS::ResidentTracker (Tracker::pretreatment + Tracker::imageProcess in one call, include/visfs_tracker.h), the covisible
// rows go to visfs_pnp_solve (the pose guess of Estimator::process) and the words into the sliding-window container
// (visfs_window_insert), which is what Estimator hands to the BA.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/frame_step.cpp -Lvisfs_amd/lib -lvisfs_window -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o frame_step && ./frame_step 5          (./frame_step 5 host: the one-core twins, no GPU)
//   ./frame_step 5 cull (or: 5 host cull): the configuration of the launch files that set Tracker/FlowBack to false: no reverse
//   passes, and Tracker/CullByFundationMatrix inside the resident call in their place.
//   ./frame_step 5 pnp (or: 5 host pnp): the pose guess runs inside the resident call too (include/visfs_tracker_pnp.h, DESIGN.md
//   section 9k): the pose comes from VISFS::ResidentTracker::poseGuess() and no visfs_pnp object is created.
//
// A stereo camera slides sideways in front of a textured wall 5 m away, so the true motion and depth are known.  The pose PnP finds
// in one frame is the guess of the next; the first guess is the identity, which the wrapper treats as "not set" (Tracker.cpp:237).
// Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ResidentTracker.h"
#include "visfs_ba.h"
#include "visfs_pnp.h"
#include "visfs_window.h"

namespace frame_step {

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

struct Summary {
    int frames = 0, inserted = 0, words = 0, covisible = 0, new_words = 0, min_pnp_inliers = 1 << 30, bootstrapped = 0, identity_guesses = 0;
    double max_translation_err = 0.0, max_depth_err = 0.0, ms = 0.0;
};

// cull: Tracker/CullByFundationMatrix; the flow object must then have been made with flow_back off
// resident_pnp: the pose guess inside the tracker call; pnp is not used then and may be NULL
inline int run(int frames, visfs_flow* flow, visfs_pnp* pnp, Summary& out, bool cull = false, bool resident_pnp = false) {
    const int W = 640, H = 400;
    const float fx = 435.2f, baseline = 0.11f;
    const double depth = 5.0, step = 0.06;                                      // metres per frame to the right: flow = -fx * step / depth
    const double disparity = (double)fx * baseline / depth, shift = -(double)fx * step / depth;
    const double Tir[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };            // image -> robot
    visfs_flow_camera cam{};
    cam.fx = cam.fy = fx; cam.cx = cam.cx_right = 0.5f * W; cam.cy = 0.5f * H; cam.baseline = baseline;
    visfs_pnp_camera pcam{};
    pcam.fx = pcam.fy = fx; pcam.cx = 0.5 * W; pcam.cy = 0.5 * H;
    for (int i = 0; i < 12; ++i) { cam.Tir[i] = Tir[i]; pcam.Tir[i] = Tir[i]; }
    VISFS::ResidentTracker tracker(flow, cam, 300, 0.01, 20, 10, false, 3.0, 8, 8, cull, 1.0f);
    visfs_pnp_params pp;
    visfs_pnp_default_params(&pp);
    if (resident_pnp) tracker.enablePnP(pp.min_inliers, pp.iterations, (double)pp.reproj_error, pp.refine_iterations, pp.seed);
    visfs_window_map* window = nullptr;
    if (visfs_window_create(0, nullptr, nullptr, &window) != VISFS_BA_OK) return 2;
    const Texture wall(2024);
    double guess[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };     // getDeltaPoseGuess(): the motion PnP found last
    for (int f = 1; f <= frames; ++f) {
        const std::vector<uint8_t> left = wall.image(W, H, -shift * (f - 1)), right = wall.image(W, H, -shift * (f - 1) + disparity);
        const auto t0 = std::chrono::steady_clock::now();
        VISFS::ResidentTracker::Frame fr;
        out.identity_guesses += VISFS::ResidentTracker::isIdentity(guess) ? 1 : 0;
        tracker.pretreatment({});                                               // no BA in this example: no outliers come back
        if (tracker.imageProcess(left.data(), right.data(), W, guess, fr) != VISFS_BA_OK) {
            std::fprintf(stderr, "imageProcess failed: %s\n", tracker.lastError());
            return 1;
        }
        ++out.frames;
        if (fr.noPrevious) { out.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); continue; }
        if (fr.lost) { std::fprintf(stderr, "lost tracking in frame %d\n", f); return 5; }
        out.bootstrapped += fr.bootstrapped ? 1 : 0;
        // Estimator::process's guess (estimateMotion3DTo2D): the covisible rows as they come
        std::vector<float> from3, to2, covUv;
        std::vector<uint64_t> covIds;
        for (const auto& kv : fr.covisibleWords3d) {
            const auto& px = fr.keyPointsMatchesFormer.at(kv.first);
            const auto& fp = fr.covisibleWords.at(kv.first);
            from3.insert(from3.end(), { kv.second.x, kv.second.y, kv.second.z });
            to2.insert(to2.end(), { px.x, px.y });
            covIds.push_back(kv.first); covUv.insert(covUv.end(), { fp.x, fp.y });
        }
        const int32_t n = (int32_t)covIds.size();
        double T[16], cov[36];
        std::vector<int32_t> matches((size_t)n + 1), inliers((size_t)n + 1);
        int32_t nm = 0, ni = 0;
        if (resident_pnp) {                                                     // it came down with the tracker call
            VISFS::ResidentTracker::PoseGuess pg;
            if (tracker.poseGuess(pg) != VISFS_BA_OK || !pg.ran) { std::fprintf(stderr, "no pose guess in frame %d\n", f); return 1; }
            std::memcpy(T, pg.transform.data(), sizeof(T));
            std::memcpy(cov, pg.covariance.data(), sizeof(cov));
            nm = (int32_t)pg.matches.size(); ni = (int32_t)pg.inliers.size();
        } else if (visfs_pnp_solve(pnp, &pp, &pcam, n, from3.data(), to2.data(), nullptr, T, cov, matches.data(), &nm, inliers.data(), &ni) != VISFS_BA_OK) {
            std::fprintf(stderr, "pnp failed: %s\n", visfs_pnp_last_error(pnp));
            return 1;
        }
        out.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        out.covisible += n; out.new_words += (int)fr.keyPointsNewExtract.size();
        out.min_pnp_inliers = ni < out.min_pnp_inliers ? ni : out.min_pnp_inliers;
        // the robot moved by (0, -step, 0): sideways, the robot's -y is the image's +x
        out.max_translation_err = std::fmax(out.max_translation_err, std::sqrt(T[3] * T[3] + (T[7] + step) * (T[7] + step) + T[11] * T[11]));
        std::memcpy(guess, T, sizeof(guess));
        std::vector<uint64_t> wid;
        std::vector<float> uv, p3;
        std::vector<uint8_t> has3d;
        for (const auto& kv : fr.words) {
            const auto& r = fr.keyPointMatchesImageRight.at(kv.first);
            const auto& p = fr.words3d.at(kv.first);
            wid.push_back(kv.first);
            uv.insert(uv.end(), { kv.second.x, kv.second.y, r.x, r.y });
            p3.insert(p3.end(), { p.x, p.y, p.z });
            has3d.push_back(1);
            out.max_depth_err = std::fmax(out.max_depth_err, std::fabs(p.x - depth));
        }
        out.words += (int)wid.size();
        const double Twr[12] = { 1, 0, 0, 0, 0, 1, 0, -step * (f - 1), 0, 0, 1, 0 };
        const double wheel[12] = { 0 }, translation[3] = { 0, -step, 0 };
        const int rc = visfs_window_insert(window, (uint64_t)f, Twr, wheel, translation, (int32_t)wid.size(), wid.data(), uv.data(), p3.data(),
                                           has3d.data(), n, covIds.data(), covUv.data());
        if (rc != 1) { std::fprintf(stderr, "insert refused: %d\n", rc); return 4; }
        ++out.inserted;
    }
    visfs_window_destroy(window);
    return 0;
}

}  // namespace frame_step

#ifndef FRAME_STEP_NO_MAIN
int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 5;
    bool host = false, cull = false, resident_pnp = false;
    for (int i = 2; i < argc; ++i) {
        host = host || std::strcmp(argv[i], "host") == 0;
        cull = cull || std::strcmp(argv[i], "cull") == 0;
        resident_pnp = resident_pnp || std::strcmp(argv[i], "pnp") == 0;
    }
    visfs_ba_handle* ba = nullptr;
    visfs_flow* flow = nullptr;
    visfs_pnp* pnp = nullptr;
    visfs_flow_params fp;
    visfs_flow_default_params(&fp);
    if (cull) fp.flow_back = 0;
    if (host) {
        if (visfs_flow_create_host(&fp, 640, 400, &flow) != VISFS_BA_OK) return 3;
        if (!resident_pnp && visfs_pnp_create_host(4096, &pnp) != VISFS_BA_OK) return 3;
    } else {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
        if (visfs_flow_create(ba, &fp, 640, 400, &flow) != VISFS_BA_OK) return 3;
        if (!resident_pnp && visfs_pnp_create(ba, 4096, &pnp) != VISFS_BA_OK) return 3;
    }
    frame_step::Summary s;
    int rc;
    try { rc = frame_step::run(frames, flow, pnp, s, cull, resident_pnp); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    visfs_pnp_destroy(pnp);
    visfs_flow_destroy(flow);
    if (ba) visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::printf("{\"frames\": %d, \"inserted\": %d, \"words\": %d, \"covisible\": %d, \"new_words\": %d, \"bootstrapped\": %d, "
                "\"identity_guesses\": %d, \"min_pnp_inliers\": %d, \"max_translation_err_m\": %.4g, \"max_depth_err_m\": %.4g, \"frame_ms\": %.2f, \"cull\": %d}\n",
                s.frames, s.inserted, s.words, s.covisible, s.new_words, s.bootstrapped, s.identity_guesses, s.min_pnp_inliers,
                s.max_translation_err, s.max_depth_err, s.ms, cull ? 1 : 0);
    return 0;
}
#endif
