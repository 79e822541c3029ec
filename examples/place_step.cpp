// place_step.cpp — a revisited room on the C ABIs of this repository: a tracker (include/visfs_flow.h, visfs_corners.h) walks through
// a few rooms and VISFS::PlaceRecognizer (visfs_amd/host/PlaceRecognizer.h over include/visfs_place.h) keeps one key-frame per room,
// the words with a finite 3-D point.  Then a fresh tracker, as after VISFS_TRACKER_LOST, is shown one of the rooms again, turned and
// shifted: the recognizer names the key-frame and visfs_pnp_solve (include/visfs_pnp.h) gives the pose against it from the rows of
// the top candidate.
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/place_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o place_step && ./place_step [rooms] [revisited room] [host]
//
// Every room is a textured wall 5 m in front of a stereo camera (a sum of sinusoids, sampled analytically); within a room the camera
// slides sideways, between rooms every track ends.  The revisit rolls the camera about its optical axis and shifts it sideways, so
// the true pose against the key-frame is known.  With "host" everything runs on the one-core twins and no device is needed.
// Prints one JSON line.
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
#include "visfs_pnp.h"

namespace place_step {

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
    visfs_pnp* pnp = nullptr;
    VISFS::PlaceRecognizer* rec = nullptr;
    ~Guard() {
        delete rec;               // detaches its set first
        if (pnp) visfs_pnp_destroy(pnp);
        if (fresh) visfs_flow_destroy(fresh);
        if (walk) visfs_flow_destroy(walk);
    }
};

struct Summary {
    int rooms = 0, keyframes = 0, query_points = 0, slot = -1, matches = 0, inliers = 0;
    long long key = 0;
    std::vector<int> words, counts;
    double rot_err = 0.0, trans_err = 0.0, T[16] = { 0 };
};

using P2 = VISFS::PlaceRecognizer::Point2f;
using P3 = VISFS::PlaceRecognizer::Point3f;

inline int run(int rooms, int revisit, visfs_ba_handle* ba, Summary& out) {
    const int W = 480, H = 320, framesPerRoom = 2, maxFeatures = 300, minDistance = 20;
    const float fx = 435.2f, baseline = 0.11f;
    const double depth = 5.0, slide = 6.0, disparity = (double)fx * baseline / depth;
    const double rot = 0.6, tx = 14.0, ty = -9.0;                                // the revisit: rolled by 0.6 rad, shifted by (14, -9) px
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
    if ((ba ? visfs_pnp_create(ba, VISFS_PLACE_MAX_POINTS, &g.pnp) : visfs_pnp_create_host(VISFS_PLACE_MAX_POINTS, &g.pnp)) != VISFS_BA_OK) return 2;
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
        v.rot = rot; v.cx = cam.cx; v.cy = cam.cy;
        v.tx = tx + slide * (framesPerRoom - 1); v.ty = ty;                      // against the key-frame, which had slid already
        const std::vector<uint8_t> left = v.image(wall, W, H, 0.0), right = v.image(wall, W, H, disparity);
        if (visfs_flow_push_frame(g.fresh, left.data(), right.data(), W) != VISFS_BA_OK) return 1;
    }
    std::vector<P2> pts;
    std::vector<int32_t> ids;
    if (top_up(g.fresh, pts, ids, next_id) != VISFS_BA_OK) return 1;
    out.query_points = (int)pts.size();
    if (rec.attach(g.fresh) != VISFS_BA_OK || rec.describe(pts) != VISFS_BA_OK) { std::fprintf(stderr, "describe failed: %s\n", rec.lastDescribeError()); return 1; }
    std::vector<VISFS::PlaceRecognizer::Candidate> cands;
    std::vector<int32_t> counts;
    if (rec.query(cands, &counts) != VISFS_BA_OK) { std::fprintf(stderr, "query failed: %s\n", rec.lastError()); return 1; }
    out.counts.assign(counts.begin(), counts.end());
    if (cands.empty()) { std::fprintf(stderr, "no key-frame recognised\n"); return 4; }
    const VISFS::PlaceRecognizer::Candidate& top = cands[0];
    out.slot = top.slot; out.key = (long long)top.key; out.matches = (int)top.ids.size();

    visfs_pnp_params pp;
    visfs_pnp_default_params(&pp);
    visfs_pnp_camera pc{};
    pc.fx = cam.fx; pc.fy = cam.fy; pc.cx = cam.cx; pc.cy = cam.cy;
    for (int i = 0; i < 12; ++i) pc.Tir[i] = Tir[i];
    double cov[36];
    std::vector<int32_t> matches(top.ids.size()), inliers(top.ids.size());
    int32_t n_matches = 0, n_inliers = 0;
    if (visfs_pnp_solve(g.pnp, &pp, &pc, (int32_t)top.ids.size(), &top.fromXyz[0].x, &top.toXy[0].x, nullptr, out.T, cov, matches.data(), &n_matches,
                        inliers.data(), &n_inliers) != VISFS_BA_OK) { std::fprintf(stderr, "pnp failed: %s\n", visfs_pnp_last_error(g.pnp)); return 1; }
    out.inliers = n_inliers;
    if (out.T[15] == 0.0) { std::fprintf(stderr, "no pose found\n"); return 4; }

    // the truth: a point of the new camera lies at Rz(rot) p + (tx, ty, 0) depth / fx in the key-frame's camera; both in the robot frame
    const double c = std::cos(rot), s = std::sin(rot);
    const double Ri[9] = { c, -s, 0, s, c, 0, 0, 0, 1 }, ti[3] = { tx * depth / fx, ty * depth / fx, 0.0 };
    double Rr[9], tr[3];
    for (int a = 0; a < 3; ++a) {
        tr[a] = Tir[4 * a] * ti[0] + Tir[4 * a + 1] * ti[1] + Tir[4 * a + 2] * ti[2];
        for (int b = 0; b < 3; ++b) {
            double v = 0.0;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) v += Tir[4 * a + i] * Ri[3 * i + j] * Tir[4 * b + j];
            Rr[3 * a + b] = v;
        }
    }
    double trace = 0.0, dt = 0.0;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) trace += Rr[3 * a + b] * out.T[4 * a + b];
        dt += (tr[a] - out.T[4 * a + 3]) * (tr[a] - out.T[4 * a + 3]);
    }
    out.rot_err = std::acos(std::fmin(1.0, std::fmax(-1.0, 0.5 * (trace - 1.0))));
    out.trans_err = std::sqrt(dt);
    return 0;
}

}  // namespace place_step

int main(int argc, char** argv) {
    const int rooms = argc > 1 ? std::atoi(argv[1]) : 4;
    const int revisit = argc > 2 ? std::atoi(argv[2]) : 1;
    const bool host = argc > 3 && std::strcmp(argv[3], "host") == 0;
    if (rooms < 1 || rooms > 30 || revisit < 0 || revisit >= rooms) { std::fprintf(stderr, "usage: place_step [rooms 1..30] [revisited room] [host]\n"); return 2; }
    visfs_ba_handle* ba = nullptr;
    if (!host) {
        visfs_ba_params prm;
        visfs_ba_default_params(&prm);
        if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
    }
    place_step::Summary s;
    int rc;
    try { rc = place_step::run(rooms, revisit, ba, s); } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); rc = 1; }
    if (ba) visfs_ba_destroy(ba);
    if (rc != 0) return 1;
    std::string words = "[", counts = "[", T = "[";
    for (size_t k = 0; k < s.words.size(); ++k) words += (k ? ", " : "") + std::to_string(s.words[k]);
    for (size_t k = 0; k < s.counts.size(); ++k) counts += (k ? ", " : "") + std::to_string(s.counts[k]);
    for (int i = 0; i < 16; ++i) { char buf[40]; std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", s.T[i]); T += buf; }
    std::printf("{\"mode\": \"%s\", \"rooms\": %d, \"keyframes\": %d, \"words\": %s], \"query_points\": %d, \"counts\": %s], \"recognised_slot\": %d, "
                "\"key\": %lld, \"matches\": %d, \"inliers\": %d, \"rot_err_rad\": %.6g, \"trans_err_m\": %.6g, \"T\": %s]}\n",
                host ? "host" : "device", s.rooms, s.keyframes, words.c_str(), s.query_points, counts.c_str(), s.slot, s.key, s.matches, s.inliers,
                s.rot_err, s.trans_err, T.c_str());
    return 0;
}
