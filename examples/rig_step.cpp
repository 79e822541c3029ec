// rig_step.cpp — a rig of four stereo cameras from the images to the BA on the C ABIs of this repository: per frame ONE call of
// VISFS::ResidentTrackerGroup (include/visfs_tracker_group.h) runs Tracker::pretreatment + Tracker::imageProcess of all four cameras,
// each camera's words go into a sliding-window container of its own (visfs_window_insert), and at the end one visfs_ba_solve_batch
// solves the four windows together.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/rig_step.cpp -Lvisfs_amd/lib -lvisfs_window -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o rig_step && ./rig_step 5            (./rig_step 3 host: the one-core twins, no GPU and no BA)
//
// The rig slides sideways in front of textured walls 5 m away, a different wall per camera, so the true motion and depth are known.
// Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define FRAME_STEP_NO_MAIN
#include "frame_step.cpp"                      // the generated wall (frame_step::Texture)

#include "ResidentTracker.h"
#include "visfs_ba.h"
#include "visfs_window.h"

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 5;
    const bool host = argc > 2 && std::strcmp(argv[2], "host") == 0;
    // ./rig_step N [host] pnp: the pose guess of every camera inside the one call too (include/visfs_tracker_pnp.h)
    const bool resident_pnp = std::strcmp(argv[argc - 1], "pnp") == 0;
    constexpr int kCams = 4;
    const int W = 640, H = 400;
    const float fx = 435.2f, baseline = 0.11f;
    const double depth = 5.0, step = 0.06;
    const double disparity = (double)fx * baseline / depth, shift = -(double)fx * step / depth;
    const double Tir[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };
    visfs_flow_camera cam{};
    cam.fx = cam.fy = fx; cam.cx = cam.cx_right = 0.5f * W; cam.cy = 0.5f * H; cam.baseline = baseline;
    for (int i = 0; i < 12; ++i) cam.Tir[i] = Tir[i];

    visfs_ba_handle* ba = nullptr;
    visfs_flow_params fp;
    visfs_flow_default_params(&fp);
    if (!host) {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    }
    visfs_flow* flows[kCams] = {};
    visfs_window_map* windows[kCams] = {};
    for (int c = 0; c < kCams; ++c) {
        const int rc = host ? visfs_flow_create_host(&fp, W, H, &flows[c]) : visfs_flow_create(ba, &fp, W, H, &flows[c]);
        if (rc != VISFS_BA_OK || visfs_window_create(0, nullptr, nullptr, &windows[c]) != VISFS_BA_OK) return 3;
    }
    int status = 0, inserted = 0, words = 0, bootstrapped = 0, launches = 0, copies = 0, syncs = 0, solved = 0, max_launches = 0;
    double max_depth_err = 0.0, group_ms = 0.0, max_pose_shift = 0.0, max_translation_err = 0.0;
    int min_pnp_inliers = 1 << 30;
    try {
        std::vector<std::unique_ptr<VISFS::ResidentTracker>> trackers;
        std::vector<VISFS::ResidentTracker*> members;
        std::vector<frame_step::Texture> walls;
        for (int c = 0; c < kCams; ++c) {
            trackers.emplace_back(new VISFS::ResidentTracker(flows[c], cam, 300, 0.01, 20, 10));
            if (resident_pnp) trackers.back()->enablePnP();
            members.push_back(trackers.back().get());
            walls.emplace_back(2024 + 17 * c);
        }
        VISFS::ResidentTrackerGroup rig(members);
        for (int f = 1; f <= frames && status == 0; ++f) {
            std::vector<std::vector<uint8_t>> left, right;
            std::vector<VISFS::ResidentTrackerGroup::Input> in;
            for (int c = 0; c < kCams; ++c) {
                left.push_back(walls[c].image(W, H, -shift * (f - 1)));
                right.push_back(walls[c].image(W, H, -shift * (f - 1) + disparity));
            }
            for (int c = 0; c < kCams; ++c) in.push_back({ left[c].data(), right[c].data(), W, nullptr });
            std::vector<VISFS::ResidentTracker::Frame> out;
            const auto t0 = std::chrono::steady_clock::now();
            if (rig.imageProcess(in, out) != VISFS_BA_OK) { std::fprintf(stderr, "group call failed: %s\n", rig.lastError()); status = 1; break; }
            group_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            rig.lastCounts(launches, copies, syncs);
            max_launches = launches > max_launches ? launches : max_launches;
            for (int c = 0; c < kCams; ++c) {
                const VISFS::ResidentTracker::Frame& fr = out[c];
                if (fr.noPrevious) continue;
                if (fr.lost) { std::fprintf(stderr, "camera %d lost tracking in frame %d\n", c, f); status = 5; break; }
                bootstrapped += fr.bootstrapped ? 1 : 0;
                if (resident_pnp) {                                     // the robot moved by (0, -step, 0), as in frame_step.cpp
                    VISFS::ResidentTracker::PoseGuess pg;
                    if (trackers[c]->poseGuess(pg) != VISFS_BA_OK || !pg.ran) { std::fprintf(stderr, "camera %d: no pose guess\n", c); status = 8; break; }
                    const double* T = pg.transform.data();
                    max_translation_err = std::fmax(max_translation_err, std::sqrt(T[3] * T[3] + (T[7] + step) * (T[7] + step) + T[11] * T[11]));
                    min_pnp_inliers = (int)pg.inliers.size() < min_pnp_inliers ? (int)pg.inliers.size() : min_pnp_inliers;
                }
                std::vector<uint64_t> wid, covIds;
                std::vector<float> uv, p3, covUv;
                std::vector<uint8_t> has3d;
                for (const auto& kv : fr.covisibleWords) { covIds.push_back(kv.first); covUv.insert(covUv.end(), { kv.second.x, kv.second.y }); }
                for (const auto& kv : fr.words) {
                    const auto& r = fr.keyPointMatchesImageRight.at(kv.first);
                    const auto& p = fr.words3d.at(kv.first);
                    wid.push_back(kv.first);
                    uv.insert(uv.end(), { kv.second.x, kv.second.y, r.x, r.y });
                    p3.insert(p3.end(), { p.x, p.y, p.z });
                    has3d.push_back(1);
                    max_depth_err = std::fmax(max_depth_err, std::fabs(p.x - depth));
                }
                words += (int)wid.size();
                const double Twr[12] = { 1, 0, 0, 0, 0, 1, 0, -step * (f - 1), 0, 0, 1, 0 };
                const double wheel[12] = { 0 }, translation[3] = { 0, -step, 0 };
                if (visfs_window_insert(windows[c], (uint64_t)f, Twr, wheel, translation, (int32_t)wid.size(), wid.data(), uv.data(), p3.data(),
                                        has3d.data(), (int32_t)covIds.size(), covIds.data(), covUv.data()) != 1) { status = 4; break; }
                ++inserted;
            }
        }
        // the four windows in one batched solve (the BA needs the device)
        if (status == 0 && !host) {
            visfs_ba_window w[kCams];
            const visfs_ba_window* wp[kCams];
            visfs_ba_result r[kCams];
            visfs_ba_result* rp[kCams];
            std::vector<uint64_t> ids[kCams], outF[kCams], outP[kCams];
            std::vector<double> poses[kCams];
            bool ready = true;
            for (int c = 0; c < kCams; ++c) {
                ready = ready && visfs_window_available(windows[c]) &&
                        visfs_window_build(windows[c], Tir, fx, fx, 0.5 * W, 0.5 * H, baseline, 2, 0, &w[c]) == VISFS_BA_OK;
                if (!ready) break;
                ids[c].resize(w[c].n_poses + 1); poses[c].resize((size_t)(w[c].n_poses + 1) * 12);
                outF[c].resize(w[c].n_refs + 1); outP[c].resize(w[c].n_refs + 1);
                std::memset(&r[c], 0, sizeof(r[c]));
                r[c].pose_ids_out = ids[c].data(); r[c].pose_Twr_out = poses[c].data();
                r[c].outlier_capacity = w[c].n_refs + 1; r[c].outlier_feature = outF[c].data(); r[c].outlier_pose = outP[c].data();
                wp[c] = &w[c]; rp[c] = &r[c];
            }
            if (!ready) { std::fprintf(stderr, "a window is not available\n"); status = 6; }
            else if (visfs_ba_solve_batch(ba, kCams, wp, rp) != VISFS_BA_OK) { std::fprintf(stderr, "batch solve: %s\n", visfs_ba_last_error(ba)); status = 7; }
            else
                for (int c = 0; c < kCams; ++c) {
                    solved += r[c].n_poses_out > 0 ? 1 : 0;
                    for (int32_t p = 0; p < r[c].n_poses_out; ++p) {       // the poses given are the true ones: the BA leaves them where they are
                        const double* T = poses[c].data() + 12 * p;
                        const double want = -step * ((double)ids[c][p] - 1.0);
                        max_pose_shift = std::fmax(max_pose_shift, std::sqrt(T[3] * T[3] + (T[7] - want) * (T[7] - want) + T[11] * T[11]));
                    }
                }
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); status = 1; }
    for (int c = 0; c < kCams; ++c) { visfs_window_destroy(windows[c]); visfs_flow_destroy(flows[c]); }
    if (ba) visfs_ba_destroy(ba);
    if (status != 0) return status;
    std::printf("{\"cameras\": %d, \"frames\": %d, \"inserted\": %d, \"words\": %d, \"bootstrapped\": %d, \"max_depth_err_m\": %.4g, "
                "\"windows_solved\": %d, \"max_pose_shift_m\": %.4g, \"kernel_launches_last\": %d, \"kernel_launches_max\": %d, "
                "\"copies_last\": %d, \"synchronisations_last\": %d, \"group_ms\": %.2f",
                kCams, frames, inserted, words, bootstrapped, max_depth_err, solved, max_pose_shift, launches, max_launches, copies, syncs, group_ms);
    if (resident_pnp) std::printf(", \"min_pnp_inliers\": %d, \"max_translation_err_m\": %.4g", min_pnp_inliers, max_translation_err);
    std::printf("}\n");
    return 0;
}
