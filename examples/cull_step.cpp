// cull_step.cpp — the outlier cull of a tracked VISFS frame on the C ABIs of this repository, for a caller that runs with
// Tracker/FlowBack off: per frame, the corners of the frame before and where the forward Lucas-Kanade pass put them go through
// VISFS::rejectOutlierWithFundationMatrix (visfs_amd/host/EpipolarCull.h over include/visfs_fund.h), as Tracker::imageProcess calls it
// (Tracker.cpp:275-277), and then through the compaction of :285-301 (status set and the corner inside the image).
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/cull_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o cull_step && ./cull_step 5 [prefix]
//
// Corners only, no images: the tracker's output is synthetic.  A cloud of landmarks in front of a robot that drives forward on a
// gentle curve; a corner of the frame before is the landmark's pixel there, cornersTo its pixel now with 0.3 px of noise; one corner
// in five is a mistrack 20 .. 60 px away that the tracker still reports with status 1, and one in eleven has status 0.  With a
// prefix, the rows of every frame are also written as <prefix>_<frame>.txt (id, from x y, to x y, status), so a test can run the
// same frames elsewhere.  Prints one JSON line.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "EpipolarCull.h"

namespace cull_step {

struct Lcg {                                             // a tiny generator, so the scene is the same everywhere
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double range(double a, double b) { return a + (b - a) * next(); }
};

struct Point2f { float x, y; };

struct Summary {
    int frames = 0;
    std::vector<int> tracked, kept, mistracksIn, mistracksKept;
    std::vector<std::vector<std::size_t>> keptIds;
    double ms = 0.0;
};

// The pose of frame f in the world seen from the camera: forward along z with a slow yaw and a little sway.
inline void project(int f, const double p[3], double fx, double fy, double cx, double cy, double& u, double& v, double& depth) {
    const double yaw = 0.02 * f, c = std::cos(yaw), s = std::sin(yaw);
    const double t[3] = { 0.03 * f * f, 0.01 * f, 0.25 * f };
    const double d[3] = { p[0] - t[0], p[1] - t[1], p[2] - t[2] };
    const double x = c * d[0] - s * d[2], y = d[1], z = s * d[0] + c * d[2];
    depth = z;
    u = fx * x / z + cx; v = fy * y / z + cy;
}

inline bool inBounds(float v, float lo, float hi) { return v >= lo && v < hi; }      // uIsInBounds

inline int run(int frames, visfs_ba_handle* ba, const std::string& dump, Summary& out) {
    const int W = 752, H = 480, nLandmarks = 400;
    const double fx = 435.2, fy = 435.2, cx = 367.4, cy = 252.2;
    const float fundationPixelError = 1.0f;                                  // Tracker/FundationPixelError
    VISFS::EpipolarCull cull(ba, 1024);
    Lcg rng{ 4242 };
    std::vector<double> landmarks;
    for (int i = 0; i < nLandmarks; ++i) {
        landmarks.push_back(rng.range(-6.0, 6.0)); landmarks.push_back(rng.range(-3.0, 3.0)); landmarks.push_back(rng.range(3.0, 12.0));
    }
    for (int f = 1; f <= frames; ++f) {
        std::vector<std::size_t> orignalWordsFromIds;
        std::vector<Point2f> cornersFrom, cornersTo;
        std::vector<unsigned char> status;
        std::vector<char> mistrack;
        for (int i = 0; i < nLandmarks; ++i) {
            double u0, v0, z0, u1, v1, z1;
            project(f - 1, &landmarks[3 * (size_t)i], fx, fy, cx, cy, u0, v0, z0);
            project(f, &landmarks[3 * (size_t)i], fx, fy, cx, cy, u1, v1, z1);
            if (z0 < 0.5 || z1 < 0.5 || !(u0 >= 0 && u0 < W && v0 >= 0 && v0 < H)) continue;
            u1 += rng.range(-0.5, 0.5); v1 += rng.range(-0.5, 0.5);
            const bool wrong = (i + f) % 5 == 2;
            if (wrong) { const double a = rng.range(0.0, 6.2831853), r = rng.range(20.0, 60.0); u1 += r * std::cos(a); v1 += r * std::sin(a); }
            orignalWordsFromIds.push_back((std::size_t)i + 1);
            cornersFrom.push_back(Point2f{ (float)u0, (float)v0 });
            cornersTo.push_back(Point2f{ (float)u1, (float)v1 });
            status.push_back((i + 3 * f) % 11 == 4 ? 0 : 1);
            mistrack.push_back(wrong ? 1 : 0);
        }
        if (!dump.empty()) {
            std::FILE* fp = std::fopen((dump + "_" + std::to_string(f) + ".txt").c_str(), "w");
            if (!fp) { std::fprintf(stderr, "cannot write the corners\n"); return 5; }
            for (size_t i = 0; i < cornersFrom.size(); ++i)
                std::fprintf(fp, "%zu %.9g %.9g %.9g %.9g %d\n", orignalWordsFromIds[i], cornersFrom[i].x, cornersFrom[i].y, cornersTo[i].x,
                             cornersTo[i].y, (int)status[i]);
            if (std::fclose(fp) != 0) return 5;
        }
        int wrongIn = 0;
        for (size_t i = 0; i < status.size(); ++i) wrongIn += status[i] && mistrack[i];
        // Tracker.cpp:275-277 with flowBack_ off and cullByFundationMatrix_ on
        const auto t0 = std::chrono::steady_clock::now();
        const int kept = VISFS::rejectOutlierWithFundationMatrix(cull.get(), cornersFrom, cornersTo, status, fundationPixelError);
        out.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (kept < 0) { std::fprintf(stderr, "frame %d: fewer than seven corners\n", f); return 4; }
        // Reduce feature vector (:285-301)
        std::vector<std::size_t> orignalWordsFromIdsCpy = orignalWordsFromIds;
        std::vector<Point2f> cornersToKept(cornersTo.size());
        std::size_t index = 0;
        int wrongKept = 0;
        for (std::size_t i = 0; i < status.size(); ++i) {
            if (status[i] && inBounds(cornersTo[i].x, 0.f, (float)W) && inBounds(cornersTo[i].y, 0.f, (float)H)) {
                orignalWordsFromIds[index] = orignalWordsFromIdsCpy[i];
                cornersToKept[index++] = cornersTo[i];
                wrongKept += mistrack[i];
            }
        }
        orignalWordsFromIds.resize(index);
        cornersToKept.resize(index);
        out.tracked.push_back((int)status.size());
        out.kept.push_back((int)index);
        out.mistracksIn.push_back(wrongIn);
        out.mistracksKept.push_back(wrongKept);
        out.keptIds.push_back(orignalWordsFromIds);
        ++out.frames;
    }
    return 0;
}

}  // namespace cull_step

int main(int argc, char** argv) {
    const int frames = argc > 1 ? std::atoi(argv[1]) : 5;
    const std::string dump = argc > 2 ? argv[2] : "";
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    cull_step::Summary s;
    int rc;
    try { rc = cull_step::run(frames, ba, dump, s); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    auto list = [](const std::vector<int>& v) {
        std::string o = "[";
        for (size_t k = 0; k < v.size(); ++k) o += (k ? ", " : "") + std::to_string(v[k]);
        return o + "]";
    };
    std::string ids = "[";
    for (size_t k = 0; k < s.keptIds.size(); ++k) {
        ids += k ? ", [" : "[";
        for (size_t i = 0; i < s.keptIds[k].size(); ++i) ids += (i ? ", " : "") + std::to_string(s.keptIds[k][i]);
        ids += "]";
    }
    std::printf("{\"frames\": %d, \"tracked\": %s, \"kept\": %s, \"mistracks_in\": %s, \"mistracks_kept\": %s, \"kept_ids\": %s], \"cull_ms\": %.3f}\n",
                s.frames, list(s.tracked).c_str(), list(s.kept).c_str(), list(s.mistracksIn).c_str(), list(s.mistracksKept).c_str(), ids.c_str(), s.ms);
    return 0;
}
