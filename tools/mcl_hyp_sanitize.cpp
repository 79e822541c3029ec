// mcl_hyp_sanitize.cpp — the one-core host twin of the pose hypotheses (include/visfs_mcl_hyp.h) under the address and
// undefined-behaviour sanitizers: a stand-alone program that drives it through two modes and through a snake of 512 bins.
// It needs no GPU and is no part of the library; build it from the repository root with the library's sources, host code
// instrumented:
//
//   S=visfs_amd/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude tools/mcl_hyp_sanitize.cpp $S/ba_api.cpp $S/ba_*.hip -lpthread
//       -o mcl_hyp_sanitize && ./mcl_hyp_sanitize
//
// Prints one line per case and "ok"; any finding of a sanitizer ends it with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "visfs_ba.h"
#include "visfs_mcl.h"
#include "visfs_mcl_hyp.h"
#include "visfs_mcl_kld.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

// One pure resampling of the particles on a KLD filter with hypotheses: no motion, no points, the gate open.
int resample(visfs_mcl_field* field, const std::vector<double>& x, const std::vector<double>& y, const std::vector<double>& yaw,
             const std::vector<double>& w, int32_t min_particles, visfs_mcl_hyp_result& h, std::vector<int32_t>& label) {
    const int32_t N = (int32_t)x.size();
    visfs_mcl* f = nullptr;
    CHECK(visfs_mcl_create(field, N, 66, &f) == VISFS_BA_OK);
    CHECK(visfs_mcl_hyp_enable(f) == VISFS_BA_ERR_BAD_ARGUMENT);
    visfs_mcl_kld_params kp;
    visfs_mcl_kld_default_params(&kp);
    kp.min_particles = min_particles;
    CHECK(visfs_mcl_kld_enable(f, &kp) == VISFS_BA_OK && visfs_mcl_hyp_enable(f) == VISFS_BA_OK && visfs_mcl_hyp_enable(f) == VISFS_BA_OK);
    CHECK(visfs_mcl_kld_upload(f, N, x.data(), y.data(), yaw.data(), w.data()) == VISFS_BA_OK);
    visfs_mcl_params p;
    visfs_mcl_default_params(&p);
    p.alpha1 = p.alpha2 = p.alpha3 = p.alpha4 = 0.0; p.resample_interval = 1; p.n_eff_ratio = 2.0;
    const double still[3] = { 0.0, 0.0, 0.0 };
    visfs_mcl_result r;
    CHECK(visfs_mcl_update(f, &p, still, 0, nullptr, &r) == VISFS_BA_OK && r.resampled == 1);
    CHECK(visfs_mcl_hyp_last(f, &h) == VISFS_BA_OK && h.fresh == 1 && h.n == visfs_mcl_kld_count(f));
    label.assign((size_t)h.n, -1);
    CHECK(visfs_mcl_hyp_download_labels(f, label.data()) == VISFS_BA_OK);
    p.n_eff_ratio = 0.0;                                                   // the gate closed: kept, no longer fresh
    visfs_mcl_hyp_result h2;
    CHECK(visfs_mcl_update(f, &p, still, 0, nullptr, &r) == VISFS_BA_OK && r.resampled == 0);
    CHECK(visfs_mcl_hyp_last(f, &h2) == VISFS_BA_OK && h2.fresh == 0 && h2.n_clusters == h.n_clusters && h2.hyp[0].count == h.hyp[0].count);
    const double mean[3] = { 1.0, 1.0, 0.0 }, sigma[3] = { 0.1, 0.1, 0.1 };
    CHECK(visfs_mcl_init(f, mean, sigma) == VISFS_BA_OK && visfs_mcl_hyp_last(f, &h2) == VISFS_BA_OK && h2.n_hypotheses == 0);
    visfs_mcl_destroy(f);
    return 0;
}

}  // namespace

int main() {
    const int32_t nx = 60, ny = 50;
    std::vector<uint16_t> cells((size_t)nx * ny, 30000);
    for (int32_t i = 0; i < nx; ++i) cells[(size_t)i] = cells[(size_t)(ny - 1) * nx + i] = 2000;
    visfs_submap_info lim{};
    lim.resolution = 0.05; lim.max_x = ny * 0.05; lim.max_y = nx * 0.05; lim.num_x_cells = nx; lim.num_y_cells = ny;
    visfs_mcl_field_params fp;
    visfs_mcl_field_default_params(&fp);
    visfs_mcl_field* field = nullptr;
    CHECK(visfs_mcl_field_create_from_grid(nullptr, &lim, cells.data(), &fp, &field) == VISFS_BA_OK);
    Rng rng{ 7 };
    const double bin_xy = 0.5, bin_yaw = 3.14159265358979323846 / 18.0;

    {   // two modes: 60 % of the weight about A, 40 % about B
        const int32_t N = 3000;
        std::vector<double> x(N), y(N), yaw(N), w(N);
        for (int32_t i = 0; i < N; ++i) {
            const bool a = i % 2 == 0;
            x[i] = (a ? 2.2 : 4.6) + 0.1 * (rng.uni() - 0.5); y[i] = (a ? 2.3 : 4.2) + 0.1 * (rng.uni() - 0.5);
            yaw[i] = (a ? 0.3 : -1.0) + 0.05 * (rng.uni() - 0.5);
            w[i] = (a ? 0.6 : 0.4) * (1.0 + 0.2 * rng.uni());
        }
        visfs_mcl_hyp_result h;
        std::vector<int32_t> label;
        if (resample(field, x, y, yaw, w, 100, h, label)) return 1;
        CHECK(h.n_clusters == 2 && h.n_hypotheses == 2 && h.hyp[0].count + h.hyp[1].count == h.n && h.hyp[0].count > h.hyp[1].count);
        CHECK(std::fabs(h.hyp[0].mean[0] - 2.2) < 0.1 && std::fabs(h.hyp[1].mean[0] - 4.6) < 0.1 && std::fabs(h.hyp[0].weight + h.hyp[1].weight - 1.0) < 1e-12);
        for (int32_t l : label) CHECK(l == h.hyp[0].label || l == h.hyp[1].label);
        std::printf("two_modes: n %d, clusters %d, counts %d %d\n", h.n, h.n_clusters, h.hyp[0].count, h.hyp[1].count);
    }
    {   // a snake of 512 bins, one wide, bent into a U; 32 particles in each, all 16384 drawn
        std::vector<double> x, y, yaw, w;
        auto bin = [&](int bx, int by) {
            for (int k = 0; k < 32; ++k) {
                x.push_back((bx + 0.05 + 0.9 * rng.uni()) * bin_xy); y.push_back((by + 0.05 + 0.9 * rng.uni()) * bin_xy);
                yaw.push_back((2 + 0.05 + 0.9 * rng.uni()) * bin_yaw); w.push_back(1.0 + 0.25 * rng.uni());
            }
        };
        for (int bx = 0; bx < 254; ++bx) bin(bx, 0);
        bin(253, 1); bin(253, 2);
        for (int bx = 253; bx > -3; --bx) bin(bx, 3);
        CHECK(x.size() == 16384);
        visfs_mcl_hyp_result h;
        std::vector<int32_t> label;
        if (resample(field, x, y, yaw, w, 16384, h, label)) return 1;
        CHECK(h.n == 16384 && h.n_clusters == 1 && h.hyp[0].count == 16384 && h.hyp[0].bins == 512 && h.hyp[0].label == 0);
        for (int32_t l : label) CHECK(l == 0);
        std::printf("snake: n %d, clusters %d, bins %d\n", h.n, h.n_clusters, h.hyp[0].bins);
    }
    visfs_mcl_field_destroy(field);
    std::printf("ok\n");
    return 0;
}
