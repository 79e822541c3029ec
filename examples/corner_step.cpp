// corner_step.cpp — the whole pixel path of one VISFS frame on the C ABIs of this repository, corners included: the tracker finds
// its own corners on the first frame (cv::goodFeaturesToTrack, Tracker.cpp:181), tracks them (:257-301), tops the words up to
// Tracker/MaxFeatures behind the mask of the tracked points on every following frame (getMask and :322-336), triangulates (:354-388)
// and hands the words to the sliding-window container (visfs_window_insert).  The images never leave the device once pushed.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/corner_step.cpp -Lvisfs_amd/lib -lvisfs_window -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o corner_step && ./corner_step 4 [prefix]
//
// The scene is tracker_step's: a stereo camera slides sideways in front of a textured wall 5 m away, so the true flow and disparity
// are known.  With a prefix, every generated image is also written as <prefix>_<frame>_<left|right>.pgm.  Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#define TRACKER_STEP_NO_MAIN
#include "tracker_step.cpp"

namespace corner_step {

struct Summary {
    int frames = 0, words = 0, tracked = 0, inserted = 0;
    std::vector<int> newCorners, wordsBefore;                                  // per frame: corners added, words before the top-up
    double max_flow_err = 0.0, max_depth_err = 0.0, ms = 0.0;
};

struct WindowGuard {
    visfs_window_map* map = nullptr;
    WindowGuard() = default;
    WindowGuard(const WindowGuard&) = delete;
    WindowGuard& operator=(const WindowGuard&) = delete;
    ~WindowGuard() { if (map) visfs_window_destroy(map); }
};

inline bool writePgm(const std::string& path, const std::vector<uint8_t>& img, int w, int h) {
    std::FILE* fp = std::fopen(path.c_str(), "wb");
    if (!fp) return false;
    std::fprintf(fp, "P5\n%d %d\n255\n", w, h);
    const bool ok = std::fwrite(img.data(), 1, img.size(), fp) == img.size();
    return std::fclose(fp) == 0 && ok;
}

inline int run(int frames, visfs_ba_handle* ba, const std::string& dump, Summary& out) {
    const int W = 640, H = 400;
    const int maxFeatures = 300, minDistance = 40;                              // Tracker/MaxFeatures, Tracker/MinDistance
    const double qualityLevel = 0.01;                                           // Tracker/QualityLevel
    const float fx = 435.2f, baseline = 0.11f;
    const double depth = 5.0, step = 0.06;
    const double disparity = (double)fx * baseline / depth, flow = -(double)fx * step / depth;
    visfs_flow_camera cam{};
    cam.fx = cam.fy = fx; cam.cx = cam.cx_right = 0.5f * W; cam.cy = 0.5f * H; cam.baseline = baseline;
    const double Tir[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };
    for (int i = 0; i < 12; ++i) cam.Tir[i] = Tir[i];
    VISFS::FlowTracker tracker(ba, W, H);
    WindowGuard guard;                                                          // destroys the container on every way out
    if (visfs_window_create(0, nullptr, nullptr, &guard.map) != VISFS_BA_OK) return 2;
    visfs_window_map* window = guard.map;
    const tracker_step::Texture wall(2024);
    using P2 = VISFS::FlowTracker::Point2f;
    std::vector<P2> corners;                                                    // the words' key-points in the newest left image
    std::vector<uint64_t> ids;
    std::vector<int> trackCnt;                                                  // frames a word has been seen in
    uint64_t nextId = 1;
    double ms = 0.0;
    for (int f = 1; f <= frames; ++f) {
        const std::vector<uint8_t> left = wall.image(W, H, -flow * (f - 1)), right = wall.image(W, H, -flow * (f - 1) + disparity);
        if (!dump.empty() && (!writePgm(dump + "_" + std::to_string(f) + "_left.pgm", left, W, H) ||
                              !writePgm(dump + "_" + std::to_string(f) + "_right.pgm", right, W, H))) {
            std::fprintf(stderr, "cannot write the images\n");
            return 5;
        }
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
            std::vector<int> keptCnt;
            for (size_t i = 0; i < to.size(); ++i) {
                if (!status[i] || !(to[i].x >= 0.f && to[i].x < (float)W && to[i].y >= 0.f && to[i].y < (float)H)) continue;
                out.max_flow_err = std::fmax(out.max_flow_err, std::hypot(to[i].x - (corners[i].x + flow), to[i].y - corners[i].y));
                covIds.push_back(ids[i]); covUv.push_back(corners[i].x); covUv.push_back(corners[i].y);
                kept.push_back(to[i]); keptIds.push_back(ids[i]); keptCnt.push_back(trackCnt[i] + 1);
            }
            out.tracked += (int)kept.size();
            corners.swap(kept); ids.swap(keptIds); trackCnt.swap(keptCnt);
        }
        out.wordsBefore.push_back((int)corners.size());
        const int backUp = maxFeatures - (int)corners.size();                   // Tracker.cpp:181 (first frame), :322-336 (top-up)
        int added = 0;
        if (backUp > 0) {
            std::vector<std::pair<int, P2>> counted;
            for (size_t i = 0; i < corners.size(); ++i) counted.emplace_back(trackCnt[i], corners[i]);
            const std::vector<visfs_corners_disc> discs = VISFS::FlowTracker::maskDiscs(counted, {}, minDistance);
            std::vector<P2> fresh;
            if (tracker.corners(fresh, backUp, qualityLevel, (double)minDistance, discs) != VISFS_BA_OK) {
                std::fprintf(stderr, "corners failed: %s\n", tracker.lastError());
                return 1;
            }
            for (const P2& c : fresh) { corners.push_back(c); ids.push_back(nextId++); trackCnt.push_back(1); }
            added = (int)fresh.size();
        }
        out.newCorners.push_back(added);
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
        const double Twr[12] = { 1, 0, 0, 0, 0, 1, 0, -step * (f - 1), 0, 0, 1, 0 };
        const double wheel[12] = { 0 }, translation[3] = { 0, -step, 0 };
        const int rc = visfs_window_insert(window, (uint64_t)f, Twr, wheel, translation, (int32_t)wid.size(), wid.data(), uv.data(), p3.data(),
                                           has3d.data(), (int32_t)covIds.size(), covIds.data(), covUv.data());
        if (rc != 1) { std::fprintf(stderr, "insert refused: %d\n", rc); return 4; }
        ++out.inserted;
        ++out.frames;
    }
    out.ms = ms;
    return 0;
}

inline std::string list(const std::vector<int>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

}  // namespace corner_step

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 4;
    const std::string dump = argc > 2 ? argv[2] : "";
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    corner_step::Summary s;
    int rc;
    try { rc = corner_step::run(frames, ba, dump, s); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::printf("{\"frames\": %d, \"words\": %d, \"tracked\": %d, \"inserted\": %d, \"words_before_top_up\": %s, \"new_corners\": %s, "
                "\"max_flow_err_px\": %.4g, \"max_depth_err_m\": %.4g, \"pixel_path_ms\": %.2f}\n",
                s.frames, s.words, s.tracked, s.inserted, corner_step::list(s.wordsBefore).c_str(), corner_step::list(s.newCorners).c_str(),
                s.max_flow_err, s.max_depth_err, s.ms);
    return 0;
}
