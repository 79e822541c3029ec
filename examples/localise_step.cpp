// localise_step.cpp — the localisation deployment's chain on one map: sub-maps -> global map -> likelihood field -> particle filter
// (VISFS::MonteCarloLocalizer over include/visfs_mcl.h).
//
//   g++ -std=c++17 -O2 -Iinclude -Ivisfs_amd/host examples/localise_step.cpp -Lvisfs_amd/lib -lvisfs_ba_hip
//       -Wl,-rpath,$PWD/visfs_amd/lib -o localise_step && ./localise_step [host] [kld | hyp]
//
// A robot drives 16 poses of a circle in a room and inserts every scan into the sub-maps; each finished front sub-map becomes a
// tile of a global map, which is composed once.  From that map come a likelihood field and a scan stack.  The robot then starts
// again with a pose guess that is off by 15 cm and 0.08 rad: one visfs_scan_stack_match of the first scan corrects it, and its
// result is the mean of the filter's initial belief.  Twenty steps follow, each an update with noisy odometry and a scan of 120
// returns, and the estimate after each.  `host` runs the one-core twins.  Prints one JSON line; the device and the twin print the
// same numbers and the same hash over every estimate's bits and the final particles.  `kld` makes the filter a KLD filter
// (include/visfs_mcl_kld.h: min_particles 100, kld_err 0.01, kld_z 0.99, at most the 2000 it starts with) and adds the particle
// count after every step to the line.  `hyp` is `kld` with AMCL's pose hypotheses (include/visfs_mcl_hyp.h): for every step that
// resampled the line also tells the number of clusters and the best hypothesis, the pose AMCL would publish, beside the mean.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <vector>

#include "ActiveSubmaps2D.h"
#include "GlobalMap2D.h"
#include "MonteCarloLocalizer.h"
#include "visfs_ba.h"

namespace localise_step {

struct Rng {                      // SplitMix64 -> uniform / normal
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
    double normal() { const double u = uni() + 1e-300, v = uni(); return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v); }
};

struct Pose { double x, y, yaw; };

inline Pose compose(const Pose& a, const Pose& z) {
    const double c = std::cos(a.yaw), s = std::sin(a.yaw);
    return { a.x + c * z.x - s * z.y, a.y + s * z.x + c * z.y, a.yaw + z.yaw };
}

inline void planar(const Pose& p, double T[12]) {
    const double c = std::cos(p.yaw), s = std::sin(p.yaw);
    const double v[12] = { c, -s, 0, p.x, s, c, 0, p.y, 0, 0, 1, 0 };
    for (int i = 0; i < 12; ++i) T[i] = v[i];
}

// n returns on the walls of the room [-3, 3] x [-2, 2], in the robot frame of `p`
inline std::vector<double> scan(const Pose& p, int n, Rng& rng) {
    std::vector<double> out;
    for (int i = 0; i < n; ++i) {
        const double a = 6.283185307179586 * (i + 0.5) / n, dx = std::cos(a + p.yaw), dy = std::sin(a + p.yaw);
        const double tx = dx > 0 ? (3.0 - p.x) / dx : (-3.0 - p.x) / dx, ty = dy > 0 ? (2.0 - p.y) / dy : (-2.0 - p.y) / dy;
        const double r = std::min(tx, ty) + 0.005 * rng.normal();
        out.insert(out.end(), { r * std::cos(a), r * std::sin(a), 0.0 });
    }
    return out;
}

constexpr int kLap = 40, kMapFrames = 16, kLimit = 4, kReturns = 360, kSteps = 20, kBeams = 120, kParticles = 2000;

struct Summary {
    int tiles = 0, obstacles = 0, resampled = 0, launches = 0, copies = 0, waits = 0, field_launches = 0;
    double match_error = 0.0, guess_error = 0.0, final_error = 0.0, final_yaw_error = 0.0, first_n_eff = 0.0, first_trace = 0.0, last_trace = 0.0;
    uint64_t hash = 1469598103934665603ull;
    bool kld = false, hyp = false;
    std::vector<int> counts;      // the particle count after every step (kld only)
    struct Hyp { int step, clusters, count; double best[3], mean[3]; };
    std::vector<Hyp> hyps;        // of every step that resampled (hyp only)
    uint64_t hyp_hash = 1469598103934665603ull;
    double hyp_final_error = 0.0;
};

inline void mix(uint64_t& h, const void* p, size_t bytes) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
}

// What the two flavours differ in: inserting a frame, whether the front is finished, and adding the front to the map.
struct Submaps {
    std::function<int(const double T[12], const std::vector<double>& returns)> insert;
    std::function<bool()> front_finished;
    std::function<int(VISFS::GlobalMap2D& map)> add_front;
};

inline int run(visfs_ba_handle* ba, const Submaps& subs, Summary& out) {
    Rng rng{ 2024 };
    const Pose step{ 0.6 * 6.283185307179586 / kLap, 0.0, 6.283185307179586 / kLap };    // a circle of 0.6 m radius
    VISFS::GlobalMap2D map(ba);
    Pose p{ 0.6, -0.3, 1.5707963267948966 };
    const Pose start = p;
    for (int f = 0; f < kMapFrames; ++f) {
        if (f > 0) p = compose(p, step);
        double T[12];
        planar(p, T);
        if (subs.insert(T, scan(p, kReturns, rng)) != VISFS_BA_OK) return 1;
        if (subs.front_finished()) {
            if (subs.add_front(map) != VISFS_BA_OK) { std::fprintf(stderr, "add failed: %s\n", map.lastError()); return 1; }
            ++out.tiles;
        }
    }
    if (out.tiles == 0 || map.compose(VISFS::GlobalMap2D::Odds) != VISFS_BA_OK) { std::fprintf(stderr, "compose failed: %s\n", map.lastError()); return 1; }

    VISFS::LikelihoodField field(map);
    VISFS::ScanStack stack = map.freeze(5);
    {
        const visfs_mcl_field_info info = field.describe();
        std::vector<uint16_t> t((size_t)info.limits.num_x_cells * (size_t)info.limits.num_y_cells);
        if (visfs_mcl_field_download(field.get(), t.data(), nullptr, nullptr, nullptr) != VISFS_BA_OK) return 1;
        for (uint16_t v : t) out.obstacles += v == 0;
        mix(out.hash, t.data(), t.size() * 2);
        int32_t k = 0;
        visfs_mcl_field_last_counts(field.get(), &k, nullptr, nullptr);
        out.field_launches = k;
    }

    // a cold start near the truth: the stack match corrects the guess, its result is where the belief begins
    Pose truth = start;
    const double guess[3] = { truth.x + 0.15, truth.y - 0.10, truth.yaw + 0.08 };
    visfs_scan_stack_params sp;
    visfs_scan_stack_default_params(&sp);
    sp.linear_search_window = 0.3; sp.angular_search_window = 0.2;
    VISFS::ScanStack::Match m;
    if (stack.match(guess, scan(truth, kReturns, rng), &m, &sp) != VISFS_BA_OK || !m.matched) { std::fprintf(stderr, "match failed: %s\n", stack.lastError()); return 1; }
    out.guess_error = std::hypot(guess[0] - truth.x, guess[1] - truth.y);
    out.match_error = std::hypot(m.x - truth.x, m.y - truth.y);

    VISFS::MonteCarloLocalizer mcl(field, kParticles, 7);
    const double mean[3] = { m.x, m.y, m.yaw }, sigma[3] = { 0.3, 0.3, 0.15 };
    if (out.kld && mcl.enableKld(100, 0.01, 0.99) != VISFS_BA_OK) { std::fprintf(stderr, "enableKld failed: %s\n", mcl.lastError()); return 1; }
    if (out.hyp && mcl.enableHypotheses() != VISFS_BA_OK) { std::fprintf(stderr, "enableHypotheses failed: %s\n", mcl.lastError()); return 1; }
    if (mcl.init(mean, sigma) != VISFS_BA_OK) { std::fprintf(stderr, "init failed: %s\n", mcl.lastError()); return 1; }
    for (int k = 0; k < kSteps; ++k) {
        truth = compose(truth, step);
        const double odo[3] = { step.x + 0.004 * rng.normal(), step.y + 0.004 * rng.normal(), step.yaw + 0.003 * rng.normal() };
        visfs_mcl_result r;
        if (mcl.update(odo, scan(truth, kBeams, rng), &r) != VISFS_BA_OK) { std::fprintf(stderr, "update failed: %s\n", mcl.lastError()); return 1; }
        const visfs_mcl_result e = mcl.estimate();
        if (std::memcmp(&e, &r, sizeof r) != 0) return 1;
        mix(out.hash, r.mean, sizeof r.mean); mix(out.hash, r.covariance, sizeof r.covariance); mix(out.hash, &r.n_eff, sizeof r.n_eff);
        mix(out.hash, &r.W, sizeof r.W); mix(out.hash, &r.best, sizeof r.best); mix(out.hash, r.best_pose, sizeof r.best_pose);
        out.resampled += r.resampled;
        if (out.kld) out.counts.push_back(mcl.particleCount());
        if (out.hyp && r.resampled) {
            const visfs_mcl_hyp_result h = mcl.hypotheses();
            visfs_mcl_hypothesis best;
            if (!h.fresh || h.update != r.update || !mcl.bestHypothesis(&best) || std::memcmp(&best, &h.hyp[0], sizeof best) != 0) {
                std::fprintf(stderr, "step %d resampled, but its hypotheses are not the fresh ones of update %lld\n", k, (long long)r.update);
                return 1;
            }
            mix(out.hyp_hash, &h, sizeof h);
            out.hyps.push_back({ k, h.n_clusters, best.count, { best.mean[0], best.mean[1], best.mean[2] }, { r.mean[0], r.mean[1], r.mean[2] } });
            out.hyp_final_error = std::hypot(best.mean[0] - truth.x, best.mean[1] - truth.y);
        }
        const double trace = r.covariance[0] + r.covariance[4] + r.covariance[8];
        if (k == 0) { out.first_n_eff = r.n_eff; out.first_trace = trace; }
        out.last_trace = trace;
        out.final_error = std::hypot(r.mean[0] - truth.x, r.mean[1] - truth.y);
        out.final_yaw_error = std::fabs(std::remainder(r.mean[2] - truth.yaw, 6.283185307179586));
    }
    std::vector<double> x, y, yaw, w;
    if (mcl.download(&x, &y, &yaw, &w) != VISFS_BA_OK) return 1;
    for (const std::vector<double>* v : { &x, &y, &yaw, &w }) mix(out.hash, v->data(), v->size() * sizeof(double));
    mcl.lastCounts(&out.launches, &out.copies, &out.waits);
    return 0;
}

inline bool finished(const visfs_submaps* s) {
    int32_t n = 0;
    visfs_submap_info info[2];
    return visfs_submaps_describe(s, &n, info) == VISFS_BA_OK && n > 0 && info[0].finished != 0;
}

// the one-core twins: host sub-maps over the C ABI
inline int run_host(Summary& out) {
    visfs_submap_params sp;
    visfs_submap_default_params(&sp);
    sp.num_range_data_limit = kLimit;
    visfs_submaps* s = nullptr;
    if (visfs_submaps_create_host(&sp, &s) != VISFS_BA_OK) return 1;
    Submaps subs;
    subs.insert = [&](const double T[12], const std::vector<double>& ret) {
        visfs_range_data rd{};
        rd.n_returns = (int32_t)(ret.size() / 3); rd.returns = ret.data();
        return visfs_submaps_insert(s, T, 1, &rd);
    };
    subs.front_finished = [&]() { return finished(s); };
    subs.add_front = [&](VISFS::GlobalMap2D& map) { return map.addSubmap(s, 0); };
    const int rc = run(nullptr, subs, out);
    visfs_submaps_destroy(s);
    return rc;
}

// the device: VISFS::Map::ActiveSubmaps2D, the tiles, the map, the field and the filter on the handle's stream
inline int run_device(visfs_ba_handle* ba, Summary& out) {
    VISFS::Map::ActiveSubmaps2D submaps(ba, kLimit);
    Submaps subs;
    subs.insert = [&](const double T[12], const std::vector<double>& ret) {
        std::vector<VISFS::Map::ActiveSubmaps2D::RangeData> rds(1);
        rds[0].returns = ret;
        return submaps.insertRangeData(rds, T);
    };
    subs.front_finished = [&]() { const auto v = submaps.submaps(); return !v.empty() && v[0].finished != 0; };
    subs.add_front = [&](VISFS::GlobalMap2D& map) { return submaps.addToMap(map, 0); };
    return run(ba, subs, out);
}

}  // namespace localise_step

int main(int argc, char** argv) {
    bool host = false;
    localise_step::Summary s;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "host") == 0) host = true;
        if (std::strcmp(argv[i], "kld") == 0) s.kld = true;
        if (std::strcmp(argv[i], "hyp") == 0) s.kld = s.hyp = true;
    }
    int rc;
    try {
        if (host) {
            rc = localise_step::run_host(s);
        } else {
            visfs_ba_params prm;
            visfs_ba_default_params(&prm);
            visfs_ba_handle* ba = nullptr;
            if (visfs_ba_create(&prm, 0, &ba) != VISFS_BA_OK) { std::fprintf(stderr, "no MI355X / gfx950 device\n"); return 3; }
            rc = localise_step::run_device(ba, s);                               // everything made on the handle goes before it
            visfs_ba_destroy(ba);
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
    if (rc != 0) return 1;
    std::printf("{\"mode\": \"%s\", \"tiles\": %d, \"obstacle_cells\": %d, \"steps\": %d, \"particles\": %d, \"guess_error_m\": %.17g, "
                "\"match_error_m\": %.17g, \"final_error_m\": %.17g, \"final_yaw_error_rad\": %.17g, \"first_n_eff\": %.17g, \"first_trace\": %.17g, "
                "\"last_trace\": %.17g, \"resampled\": %d, \"hash\": \"%016llx\", \"field_launches\": %d, \"launches\": %d, \"copies\": %d, \"waits\": %d",
                host ? "host" : "device", s.tiles, s.obstacles, localise_step::kSteps, localise_step::kParticles, s.guess_error, s.match_error,
                s.final_error, s.final_yaw_error, s.first_n_eff, s.first_trace, s.last_trace, s.resampled, (unsigned long long)s.hash, s.field_launches,
                s.launches, s.copies, s.waits);
    if (s.kld) {
        std::printf(", \"kld\": 1, \"counts\": [");
        for (size_t i = 0; i < s.counts.size(); ++i) std::printf("%s%d", i ? ", " : "", s.counts[i]);
        std::printf("]");
    }
    if (s.hyp) {
        std::printf(", \"hyp\": 1, \"hyp_hash\": \"%016llx\", \"hyp_final_error_m\": %.17g, \"hypotheses\": [", (unsigned long long)s.hyp_hash, s.hyp_final_error);
        for (size_t i = 0; i < s.hyps.size(); ++i) {
            const auto& h = s.hyps[i];
            std::printf("%s{\"step\": %d, \"clusters\": %d, \"count\": %d, \"best\": [%.17g, %.17g, %.17g], \"mean\": [%.17g, %.17g, %.17g]}", i ? ", " : "",
                        h.step, h.clusters, h.count, h.best[0], h.best[1], h.best[2], h.mean[0], h.mean[1], h.mean[2]);
        }
        std::printf("]");
    }
    std::printf("}\n");
    return 0;
}
