// clahe_step.cpp — a frame of the shipped configuration (System/CLAHE = true) on the C ABIs of this repository: two stereo pairs
// of a low-contrast scene go through VISFS::FlowTracker::pushFrameCLAHE (cv::createCLAHE(3.0, cv::Size(8, 8))->apply on both images,
// System.cpp:107-111, then the pyramids), the tracker takes its corners on the first equalised left image and tracks them into the
// second.  The same two pairs then go through plain pushFrame, to show what the equalisation buys on such a scene.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/clahe_step.cpp -Lvisfs_amd/lib -lvisfs_window -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o clahe_step && ./clahe_step [prefix]
//
// The scene is tracker_step's wall with its contrast cut to an eighth around grey level 112.  With a prefix, the four images are
// also written as <prefix>_<frame>_<left|right>.pgm.  Prints one JSON line; "digest" is FNV-1a over the bytes of the corners, the
// tracked positions and the status of the equalised run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define TRACKER_STEP_NO_MAIN
#include "tracker_step.cpp"

namespace clahe_step {

using P2 = VISFS::FlowTracker::Point2f;

struct Run {
    int corners = 0, tracked = 0;
    double max_flow_err = 0.0;
    uint64_t digest = 1469598103934665603ull;
};

inline void fnv(uint64_t& h, const void* data, size_t bytes) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 1099511628211ull; }
}

inline bool writePgm(const std::string& path, const std::vector<uint8_t>& img, int w, int h) {
    std::FILE* fp = std::fopen(path.c_str(), "wb");
    if (!fp) return false;
    std::fprintf(fp, "P5\n%d %d\n255\n", w, h);
    const bool ok = std::fwrite(img.data(), 1, img.size(), fp) == img.size();
    return std::fclose(fp) == 0 && ok;
}

inline int run(visfs_ba_handle* ba, const std::vector<uint8_t> (&img)[2][2], int W, int H, double flow, bool equalise, Run& out) {
    VISFS::FlowTracker tracker(ba, W, H);
    std::vector<P2> corners, to;
    std::vector<unsigned char> status;
    for (int f = 0; f < 2; ++f) {
        const int rc = equalise ? tracker.pushFrameCLAHE(img[f][0].data(), img[f][1].data(), W)
                                : tracker.pushFrame(img[f][0].data(), img[f][1].data(), W);
        if (rc != VISFS_BA_OK) { std::fprintf(stderr, "push failed: %s\n", tracker.lastError()); return 1; }
        if (f == 0 && tracker.corners(corners, 300, 0.01, 20.0) != VISFS_BA_OK) { std::fprintf(stderr, "corners failed: %s\n", tracker.lastError()); return 1; }
    }
    if (tracker.track(corners, to, status) != VISFS_BA_OK) { std::fprintf(stderr, "track failed: %s\n", tracker.lastError()); return 1; }
    out.corners = (int)corners.size();
    for (size_t i = 0; i < to.size(); ++i) {
        if (!status[i]) continue;
        ++out.tracked;
        out.max_flow_err = std::fmax(out.max_flow_err, std::hypot(to[i].x - (corners[i].x + flow), to[i].y - corners[i].y));
    }
    if (!corners.empty()) {
        fnv(out.digest, &corners[0].x, corners.size() * sizeof(P2));
        fnv(out.digest, &to[0].x, to.size() * sizeof(P2));
        fnv(out.digest, status.data(), status.size());
    }
    return 0;
}

}  // namespace clahe_step

int main(int argc, char** argv) {
    const std::string dump = argc > 1 ? argv[1] : "";
    const int W = 640, H = 400;
    const double flow = -435.2 * 0.06 / 5.0, disparity = 435.2 * 0.11 / 5.0;
    const tracker_step::Texture wall(2024);
    std::vector<uint8_t> img[2][2];
    for (int f = 0; f < 2; ++f)
        for (int i = 0; i < 2; ++i) {
            img[f][i] = wall.image(W, H, -flow * f + (i ? disparity : 0.0));
            for (uint8_t& v : img[f][i]) v = (uint8_t)(112 + v / 8);                       // an eighth of the contrast
            if (!dump.empty() && !clahe_step::writePgm(dump + "_" + std::to_string(f + 1) + (i ? "_right.pgm" : "_left.pgm"), img[f][i], W, H)) {
                std::fprintf(stderr, "cannot write the images\n");
                return 5;
            }
        }
    visfs_ba_params prm;
    visfs_ba_default_params(&prm);
    visfs_ba_handle* ba = nullptr;
    if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    clahe_step::Run eq, plain;
    int rc;
    try {
        rc = clahe_step::run(ba, img, W, H, flow, true, eq);
        if (rc == 0) rc = clahe_step::run(ba, img, W, H, flow, false, plain);
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::printf("{\"corners\": %d, \"tracked\": %d, \"max_flow_err_px\": %.4g, \"digest\": \"%016llx\", \"plain_corners\": %d, "
                "\"plain_tracked\": %d, \"plain_max_flow_err_px\": %.4g}\n",
                eq.corners, eq.tracked, eq.max_flow_err, (unsigned long long)eq.digest, plain.corners, plain.tracked, plain.max_flow_err);
    return 0;
}
