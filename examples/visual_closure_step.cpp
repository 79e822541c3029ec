// visual_closure_step.cpp — a visual loop closure on the C ABIs of this repository: a tracker (include/visfs_flow.h, visfs_corners.h)
// walks through a few rooms, VISFS::PlaceRecognizer (visfs_amd/host/PlaceRecognizer.h) keeps one key-frame per room, and every
// key-frame is a vertex of an odometry chain whose edges carry drift.  Then one room is seen again from a pose shifted sideways:
// queryVerify (include/visfs_place_verify.h) names the key-frame and verifies it by PnP and the guided stage in one call,
// closureEdge turns the verified pose into a pose-graph edge between the key-frame's vertex and the revisit's, and
// visfs_pose_graph_optimize (include/visfs_pose_graph.h) pulls the drifted chain back.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/visual_closure_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o visual_closure_step && ./visual_closure_step [rooms] [revisited room] [host]
//
// Every room is a textured wall 5 m in front of a stereo camera (the rooms of place_step.cpp).  The true poses of the vertices lie on
// an arc; every odometry edge is the true step plus 0.08 m of drift along x, so the revisit's vertex starts rooms x 0.08 m off.  The
// revisit shifts the camera by 14 px sideways, 0.161 m to the robot's right, so the true closure is (0, -0.161, 0).  With "host"
// everything runs on the one-core twins and no device is needed.  Prints one JSON line with the revisit vertex's error before and after.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "PlaceRecognizer.h"
#include "visfs_ba.h"
#include "visfs_corners.h"
#include "visfs_flow.h"
#include "visfs_place_verify.h"
#include "visfs_pose_graph.h"

namespace visual_closure_step {

struct Rng {                      // SplitMix64 -> uniform
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
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
    uint8_t at(double X, double Y) const {
        double v = 128.0;
        for (size_t k = 0; k < kx.size(); ++k) v += amp[k] * std::cos(kx[k] * X + ky[k] * Y + ph[k]);
        return (uint8_t)std::lround(std::fmin(std::fmax(v, 0.0), 255.0));
    }
};

// pixel q shows the wall at zoom * R(rot) (q - c) + c + t
struct View {
    double rot = 0.0, tx = 0.0, ty = 0.0, cx = 0.0, cy = 0.0;
    std::vector<uint8_t> image(const Texture& wall, int w, int h, double shift) const {
        std::vector<uint8_t> img((size_t)w * h);
        const double c = std::cos(rot), s = std::sin(rot);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const double qx = x + shift - cx, qy = y - cy;
                img[(size_t)y * w + x] = wall.at(c * qx - s * qy + cx + tx, s * qx + c * qy + cy + ty);
            }
        return img;
    }
};

struct Guard {                    // what the run creates, released in the order the library asks for
    visfs_flow* walk = nullptr;
    visfs_flow* fresh = nullptr;
    visfs_pose_graph* graph = nullptr;
    VISFS::PlaceRecognizer* rec = nullptr;
    ~Guard() {
        delete rec;               // detaches its set first
        if (graph) visfs_pose_graph_destroy(graph);
        if (fresh) visfs_flow_destroy(fresh);
        if (walk) visfs_flow_destroy(walk);
    }
};

struct Summary {
    int rooms = 0, keyframes = 0, query_points = 0, best = -1, slot = -1, rows = 0, inliers = 0, guided = 0, vertices = 0, edges = 0, graph_iterations = 0;
    long long key = 0;
    std::vector<int> words;
    double z[3] = { 0 }, z_true[3] = { 0 }, information[9] = { 0 }, out_of_plane[3] = { 0 };
    double odometry_information = 0.0, err_before = 0.0, err_after = 0.0, yaw_err_after = 0.0;
};

// planar poses (x, y, yaw): a (+) b, and the pose of b in the frame of a
struct Pose { double x, y, yaw; };
inline Pose compose(const Pose& a, const Pose& b) {
    const double c = std::cos(a.yaw), s = std::sin(a.yaw);
    return Pose{ a.x + c * b.x - s * b.y, a.y + s * b.x + c * b.y, a.yaw + b.yaw };
}
inline Pose between(const Pose& a, const Pose& b) {
    const double c = std::cos(a.yaw), s = std::sin(a.yaw), dx = b.x - a.x, dy = b.y - a.y;
    return Pose{ c * dx + s * dy, -s * dx + c * dy, b.yaw - a.yaw };
}

using P2 = VISFS::PlaceRecognizer::Point2f;
using P3 = VISFS::PlaceRecognizer::Point3f;

inline int run(int rooms, int revisit, visfs_ba_handle* ba, Summary& out) {
    const int W = 480, H = 320, framesPerRoom = 2, maxFeatures = 300, minDistance = 20;
    const float fx = 435.2f, baseline = 0.11f;
    const double depth = 5.0, slide = 6.0, disparity = (double)fx * baseline / depth;
    const double tx = 14.0;                                                      // the revisit: shifted by 14 px sideways
    const double drift = 0.08, sigma_xy = 0.2, sigma_yaw = 0.05;                 // of an odometry edge
    visfs_flow_camera cam{};
    cam.fx = cam.fy = fx; cam.cx = cam.cx_right = 0.5f * W; cam.cy = 0.5f * H; cam.baseline = baseline;
    const double Tir[12] = { 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0 };            // image -> robot
    for (int i = 0; i < 12; ++i) cam.Tir[i] = Tir[i];
    visfs_flow_params fp;
    visfs_flow_default_params(&fp);
    visfs_corners_params cp;
    visfs_corners_default_params(&cp);
    cp.quality_level = 0.01; cp.min_distance = minDistance;
    Guard g;
    const auto make_flow = [&](visfs_flow** f) { return ba ? visfs_flow_create(ba, &fp, W, H, f) : visfs_flow_create_host(&fp, W, H, f); };
    if (make_flow(&g.walk) != VISFS_BA_OK || make_flow(&g.fresh) != VISFS_BA_OK) return 2;
    if (visfs_pose_graph_create(ba, rooms + 1, rooms + 1, &g.graph) != VISFS_BA_OK) return 2;
    g.rec = new VISFS::PlaceRecognizer(ba, 30, 500);                             // Mem/STMSize, Kp/MaxFeatures
    VISFS::PlaceRecognizer& rec = *g.rec;
    if (rec.attach(g.walk) != VISFS_BA_OK) return 2;

    // corners of the newest left image of f behind the discs of the points it has already
    const auto top_up = [&](visfs_flow* f, std::vector<P2>& pts, std::vector<int32_t>& ids, int32_t& next_id) -> int {
        const int want = maxFeatures - (int)pts.size();
        if (want <= 0) return VISFS_BA_OK;
        std::vector<visfs_corners_disc> discs;
        for (const P2& p : pts) discs.push_back(visfs_corners_disc{ p.x, p.y, minDistance });
        std::vector<float> xy((size_t)want * 2);
        int32_t n = 0;
        cp.max_corners = want;
        const int rc = visfs_flow_corners(f, VISFS_FLOW_SLOT_CURRENT, VISFS_FLOW_IMAGE_LEFT, &cp, (int32_t)discs.size(), discs.empty() ? nullptr : discs.data(),
                                          want, xy.data(), &n);
        if (rc != VISFS_BA_OK) return rc;
        for (int i = 0; i < n; ++i) { pts.push_back(P2{ xy[2 * (size_t)i], xy[2 * (size_t)i + 1] }); ids.push_back(next_id++); }
        return VISFS_BA_OK;
    };

    int32_t next_id = 1;
    for (int r = 0; r < rooms; ++r) {
        const Texture wall(100 + (uint64_t)r);
        std::vector<P2> pts;
        std::vector<int32_t> ids;
        for (int j = 0; j < framesPerRoom; ++j) {
            View v;                                                              // the wall slides by `slide` px a frame; the right camera sees it `disparity` px on
            v.tx = slide * j;
            const std::vector<uint8_t> left = v.image(wall, W, H, 0.0), right = v.image(wall, W, H, disparity);
            if (visfs_flow_push_frame(g.walk, left.data(), right.data(), W) != VISFS_BA_OK) { std::fprintf(stderr, "push failed: %s\n", visfs_flow_last_error(g.walk)); return 1; }
            if (j > 0 && !pts.empty()) {                                         // Tracker.cpp:257-301
                std::vector<P2> to(pts.size());
                std::vector<uint8_t> status(pts.size());
                if (visfs_flow_track(g.walk, (int32_t)pts.size(), &pts[0].x, nullptr, &to[0].x, status.data(), nullptr) != VISFS_BA_OK) return 1;
                std::vector<P2> kept;
                std::vector<int32_t> keptIds;
                for (size_t i = 0; i < to.size(); ++i)
                    if (status[i] && to[i].x >= 0.f && to[i].x < (float)W && to[i].y >= 0.f && to[i].y < (float)H) { kept.push_back(to[i]); keptIds.push_back(ids[i]); }
                pts.swap(kept); ids.swap(keptIds);
            }
            if (top_up(g.walk, pts, ids, next_id) != VISFS_BA_OK) { std::fprintf(stderr, "corners failed: %s\n", visfs_flow_last_error(g.walk)); return 1; }
        }
        // the room's key-frame: the words of its last frame that have a finite 3-D point
        std::vector<P2> rightPts(pts.size());
        std::vector<uint8_t> status(pts.size());
        std::vector<P3> xyz(pts.size());
        if (pts.empty() || visfs_flow_stereo(g.walk, (int32_t)pts.size(), &pts[0].x, &cam, &rightPts[0].x, status.data(), &xyz[0].x) != VISFS_BA_OK) return 1;
        std::vector<P2> kp;
        std::vector<int32_t> kid;
        std::vector<P3> k3;
        for (size_t i = 0; i < pts.size(); ++i)
            if (status[i] && std::isfinite(xyz[i].x) && std::isfinite(xyz[i].y) && std::isfinite(xyz[i].z)) { kp.push_back(pts[i]); kid.push_back(ids[i]); k3.push_back(xyz[i]); }
        int slot = -1;
        if (rec.describe(kp) != VISFS_BA_OK) { std::fprintf(stderr, "describe failed: %s\n", rec.lastDescribeError()); return 1; }
        if (rec.addKeyFrame(kid, k3, 1000 * (int64_t)r + framesPerRoom - 1, &slot) != VISFS_BA_OK || slot != r) { std::fprintf(stderr, "add failed: %s\n", rec.lastError()); return 1; }
        out.words.push_back((int)kp.size());
    }
    out.rooms = rooms; out.keyframes = rec.keyFrames();

    // the revisit, on a tracker that has seen nothing
    {
        const Texture wall(100 + (uint64_t)revisit);
        View v;
        v.cx = cam.cx; v.cy = cam.cy;
        v.tx = tx + slide * (framesPerRoom - 1);                                 // against the key-frame, which had slid already
        const std::vector<uint8_t> left = v.image(wall, W, H, 0.0), right = v.image(wall, W, H, disparity);
        if (visfs_flow_push_frame(g.fresh, left.data(), right.data(), W) != VISFS_BA_OK) return 1;
    }
    std::vector<P2> pts;
    std::vector<int32_t> ids;
    if (top_up(g.fresh, pts, ids, next_id) != VISFS_BA_OK || pts.empty()) return 1;
    out.query_points = (int)pts.size();
    std::vector<P2> rightPts(pts.size());
    std::vector<uint8_t> status(pts.size());
    std::vector<P3> queryXyz(pts.size());                                        // where the key-points lie now: for the covariance
    if (visfs_flow_stereo(g.fresh, (int32_t)pts.size(), &pts[0].x, &cam, &rightPts[0].x, status.data(), &queryXyz[0].x) != VISFS_BA_OK) return 1;
    if (rec.attach(g.fresh) != VISFS_BA_OK || rec.describe(pts) != VISFS_BA_OK) { std::fprintf(stderr, "describe failed: %s\n", rec.lastDescribeError()); return 1; }
    visfs_place_verify_params vp;
    visfs_place_verify_default_params(&vp);
    vp.camera.fx = cam.fx; vp.camera.fy = cam.fy; vp.camera.cx = cam.cx; vp.camera.cy = cam.cy;
    for (int i = 0; i < 12; ++i) vp.camera.Tir[i] = Tir[i];
    std::vector<VISFS::PlaceRecognizer::Verified> verified;
    int best = -1;
    if (rec.queryVerify(vp, queryXyz, verified, &best) != VISFS_BA_OK) { std::fprintf(stderr, "queryVerify failed: %s\n", rec.lastVerifyError()); return 1; }
    out.best = best;
    if (best < 0) { std::fprintf(stderr, "no key-frame verified\n"); return 4; }
    const VISFS::PlaceRecognizer::Verified& top = verified[(size_t)best];
    out.slot = top.slot; out.key = (long long)top.key; out.rows = top.rows; out.inliers = top.inliers; out.guided = top.guided ? 1 : 0;
    // The covariance is the reference's: 2.1981 x the median squared distance and the median angle of the inliers, and on a scene
    // this clean the median angle is 0 in float.  A variance of 0 is no information matrix (closureEdge refuses it), so the caller
    // floors the variances at (1 mm)^2 and (1 mrad)^2, the resolution it trusts its stereo points to.
    VISFS::PlaceRecognizer::Verified floored = top;
    for (int k = 0; k < 6; ++k) floored.cov[7 * k] = std::fmax(floored.cov[7 * k], 1e-6);
    if (VISFS::PlaceRecognizer::closureEdge(floored, out.z, out.information, out.out_of_plane) != VISFS_BA_OK) { std::fprintf(stderr, "no closure edge\n"); return 4; }
    // the truth: the new camera stands tx * depth / fx to the right of the key-frame's, which is -y of the robot
    out.z_true[0] = 0.0; out.z_true[1] = -tx * depth / fx; out.z_true[2] = 0.0;

    // the graph: vertex r is the key-frame of room r, vertex `rooms` the revisit; true poses on an arc, odometry with drift
    const int N = rooms + 1;
    std::vector<Pose> truth((size_t)N);
    for (int r = 0; r < rooms; ++r) truth[(size_t)r] = Pose{ 1.5 * r, 0.2 * r * r, 0.25 * r };
    truth[(size_t)rooms] = compose(truth[(size_t)top.slot], Pose{ out.z_true[0], out.z_true[1], out.z_true[2] });
    std::vector<visfs_pose_graph_edge> edges;
    std::vector<Pose> start((size_t)N);
    start[0] = truth[0];
    out.odometry_information = 1.0 / (sigma_xy * sigma_xy);
    for (int r = 0; r + 1 < N; ++r) {
        Pose step = between(truth[(size_t)r], truth[(size_t)r + 1]);
        step.x += drift;
        start[(size_t)r + 1] = compose(start[(size_t)r], step);
        visfs_pose_graph_edge e{};
        e.i = r; e.j = r + 1; e.z[0] = step.x; e.z[1] = step.y; e.z[2] = step.yaw;
        e.information[0] = e.information[4] = out.odometry_information; e.information[8] = 1.0 / (sigma_yaw * sigma_yaw);
        edges.push_back(e);
    }
    visfs_pose_graph_edge closure{};
    closure.i = top.slot; closure.j = rooms;
    for (int i = 0; i < 3; ++i) closure.z[i] = out.z[i];
    for (int i = 0; i < 9; ++i) closure.information[i] = out.information[i];
    edges.push_back(closure);
    std::vector<double> in((size_t)3 * N), res((size_t)3 * N);
    std::vector<uint8_t> fixed((size_t)N, 0);
    fixed[0] = 1;
    for (int r = 0; r < N; ++r) { in[3 * (size_t)r] = start[(size_t)r].x; in[3 * (size_t)r + 1] = start[(size_t)r].y; in[3 * (size_t)r + 2] = start[(size_t)r].yaw; }
    visfs_pose_graph_params gp;
    visfs_pose_graph_default_params(&gp);
    visfs_pose_graph_result gr{};
    if (visfs_pose_graph_optimize(g.graph, &gp, N, in.data(), fixed.data(), (int32_t)edges.size(), edges.data(), res.data(), nullptr, &gr) != VISFS_BA_OK) {
        std::fprintf(stderr, "optimize failed: %s\n", visfs_pose_graph_last_error(g.graph));
        return 1;
    }
    out.vertices = N; out.edges = (int)edges.size(); out.graph_iterations = gr.iterations;
    const Pose& t = truth[(size_t)rooms];
    out.err_before = std::hypot(start[(size_t)rooms].x - t.x, start[(size_t)rooms].y - t.y);
    out.err_after = std::hypot(res[3 * (size_t)rooms] - t.x, res[3 * (size_t)rooms + 1] - t.y);
    out.yaw_err_after = std::fabs(res[3 * (size_t)rooms + 2] - t.yaw);
    return 0;
}

}  // namespace visual_closure_step

int main(int argc, char** argv) {
    const int rooms = argc > 1 ? std::atoi(argv[1]) : 4;
    const int revisit = argc > 2 ? std::atoi(argv[2]) : 0;
    const bool host = argc > 3 && std::strcmp(argv[3], "host") == 0;
    if (rooms < 1 || rooms > 30 || revisit < 0 || revisit >= rooms) { std::fprintf(stderr, "usage: visual_closure_step [rooms 1..30] [revisited room] [host]\n"); return 2; }
    visfs_ba_handle* ba = nullptr;
    if (!host) {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    }
    visual_closure_step::Summary s;
    int rc;
    try { rc = visual_closure_step::run(rooms, revisit, ba, s); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    if (ba) visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::string words = "[";
    for (size_t k = 0; k < s.words.size(); ++k) words += (k ? ", " : "") + std::to_string(s.words[k]);
    const auto list = [](const double* v, int n) {
        std::string t = "[";
        for (int i = 0; i < n; ++i) { char buf[40]; std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", v[i]); t += buf; }
        return t + "]";
    };
    std::printf("{\"mode\": \"%s\", \"rooms\": %d, \"keyframes\": %d, \"words\": %s], \"query_points\": %d, \"best\": %d, \"recognised_slot\": %d, "
                "\"key\": %lld, \"guided\": %d, \"rows\": %d, \"inliers\": %d, \"z\": %s, \"z_true\": %s, \"information\": %s, \"out_of_plane\": %s, "
                "\"odometry_information\": %.17g, \"vertices\": %d, \"edges\": %d, \"graph_iterations\": %d, \"err_before_m\": %.17g, \"err_after_m\": %.17g, "
                "\"yaw_err_after_rad\": %.17g}\n",
                host ? "host" : "device", s.rooms, s.keyframes, words.c_str(), s.query_points, s.best, s.slot, s.key, s.guided, s.rows, s.inliers,
                list(s.z, 3).c_str(), list(s.z_true, 3).c_str(), list(s.information, 9).c_str(), list(s.out_of_plane, 3).c_str(), s.odometry_information,
                s.vertices, s.edges, s.graph_iterations, s.err_before, s.err_after, s.yaw_err_after);
    return 0;
}
