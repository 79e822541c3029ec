// MonteCarloLocalizer.h — the particle filter the localisation deployment runs beside VISFS (include/visfs_mcl.h).  Header only,
// over the C ABI.
//
// A LikelihoodField is made from a GlobalMap2D's last composed grid (on the device the cells never cross to the host) or from a
// saved grid; a MonteCarloLocalizer on it carries the belief from scan to scan: init() from a pose and its deviations (the result
// of a scan-stack match after a cold start), update() with the odometry step and the match cloud of a ScanFilter, estimate() for the
// mean pose and its covariance.  Objects follow their field's flavour: a field of a device map runs HIP kernels on the map's
// stream, a field made with ba == nullptr is the one-core host twin, and both give the same bytes.  The field must outlive the
// localizer, and a device field the handle it was made on.
#ifndef VISFS_AMD_MONTE_CARLO_LOCALIZER_H
#define VISFS_AMD_MONTE_CARLO_LOCALIZER_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "GlobalMap2D.h"
#include "visfs_mcl.h"
#include "visfs_mcl_kld.h"
#include "visfs_mcl_hyp.h"

namespace VISFS {

class LikelihoodField {
public:
    static visfs_mcl_field_params defaults() {
        visfs_mcl_field_params p;
        visfs_mcl_field_default_params(&p);
        return p;
    }
    // From the map's last composed grid.  Throws std::runtime_error when it is refused (no composed grid, a bad parameter).
    explicit LikelihoodField(const GlobalMap2D& map, const visfs_mcl_field_params& p = defaults()) {
        const int rc = visfs_mcl_field_create_from_map(map.get(), &p, &f_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_mcl_field_create_from_map failed with status " + std::to_string(rc));
    }
    // From a saved grid: cells [num_y_cells][num_x_cells]; ba == nullptr gives the host twin.
    LikelihoodField(visfs_ba_handle* ba, const visfs_submap_info& limits, const std::vector<uint16_t>& cells, const visfs_mcl_field_params& p = defaults()) {
        if (limits.num_x_cells < 1 || limits.num_y_cells < 1 || cells.size() != (size_t)limits.num_x_cells * (size_t)limits.num_y_cells)
            throw std::runtime_error("LikelihoodField: the cells do not fit the limits");
        const int rc = visfs_mcl_field_create_from_grid(ba, &limits, cells.data(), &p, &f_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_mcl_field_create_from_grid failed with status " + std::to_string(rc));
    }
    LikelihoodField(const LikelihoodField&) = delete;
    LikelihoodField& operator=(const LikelihoodField&) = delete;
    ~LikelihoodField() { visfs_mcl_field_destroy(f_); }

    visfs_mcl_field* get() const { return f_; }
    visfs_mcl_field_info describe() const {
        visfs_mcl_field_info i{};
        visfs_mcl_field_describe(f_, &i);
        return i;
    }

private:
    visfs_mcl_field* f_ = nullptr;
};

class MonteCarloLocalizer {
public:
    static visfs_mcl_params defaults() {
        visfs_mcl_params p;
        visfs_mcl_default_params(&p);
        return p;
    }
    // Throws std::runtime_error when creation fails (particles outside 1 .. 65536, no memory).
    MonteCarloLocalizer(const LikelihoodField& field, int particles, uint64_t seed = 0) : n_(particles) {
        const int rc = visfs_mcl_create(field.get(), particles, seed, &f_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_mcl_create failed with status " + std::to_string(rc));
    }
    MonteCarloLocalizer(const MonteCarloLocalizer&) = delete;
    MonteCarloLocalizer& operator=(const MonteCarloLocalizer&) = delete;
    ~MonteCarloLocalizer() { visfs_mcl_destroy(f_); }

    visfs_mcl* get() const { return f_; }
    int particles() const { return n_; }
    visfs_mcl_params params = defaults();

    // The belief about `mean` (x, y, yaw) with the deviations `sigma`; the update counter returns to 0.
    int init(const double mean[3], const double sigma[3]) { return visfs_mcl_init(f_, mean, sigma); }
    // One step: the odometry delta (dx, dy, dyaw) in the previous robot frame and the scan's points [n][3] in the robot frame.
    int update(const double odomDelta[3], const std::vector<double>& pointsXyz, visfs_mcl_result* result = nullptr) {
        return visfs_mcl_update(f_, &params, odomDelta, (int32_t)(pointsXyz.size() / 3), pointsXyz.data(), result);
    }
    // The last update's mean pose, covariance and n_eff; status is VISFS_BA_ERR_BAD_ARGUMENT before any update.
    visfs_mcl_result estimate() const {
        visfs_mcl_result r{};
        visfs_mcl_last_result(f_, &r);
        return r;
    }
    // KLD-adaptive particle counts (include/visfs_mcl_kld.h): from now on a resampling draws only as many particles as the spread
    // of the belief asks for, between minParticles and the particles of the constructor (at most 16384).  The other settings keep
    // the header's defaults; there is no way back.
    int enableKld(int minParticles, double kldErr, double kldZ) {
        visfs_mcl_kld_params p;
        visfs_mcl_kld_default_params(&p);
        p.min_particles = minParticles; p.kld_err = kldErr; p.kld_z = kldZ;
        return visfs_mcl_kld_enable(f_, &p);
    }
    // AMCL's pose hypotheses (include/visfs_mcl_hyp.h), after enableKld(): from now on every resampling also clusters the new
    // particles and keeps the mean and covariance of the at most VISFS_MCL_HYP_MAX largest clusters.  There is no way back.
    int enableHypotheses() { return visfs_mcl_hyp_enable(f_); }
    // the hypotheses of the last resampling, the largest first; n_hypotheses is 0 before the first one and when they are not enabled
    visfs_mcl_hyp_result hypotheses() const {
        visfs_mcl_hyp_result r{};
        visfs_mcl_hyp_last(f_, &r);
        return r;
    }
    // The pose AMCL would publish: the mean of the cluster that holds the most particles.  False while there is no hypothesis.
    bool bestHypothesis(visfs_mcl_hypothesis* out) const {
        const visfs_mcl_hyp_result r = hypotheses();
        if (r.n_hypotheses < 1) return false;
        if (out) *out = r.hyp[0];
        return true;
    }
    // the active count: particles() unless enableKld() has let it fall
    int particleCount() const { return visfs_mcl_kld_count(f_); }
    // the particles on the host (particleCount() of them); any pointer may be null
    int download(std::vector<double>* x, std::vector<double>* y, std::vector<double>* yaw, std::vector<double>* w) const {
        for (std::vector<double>* v : { x, y, yaw, w }) if (v) v->resize((size_t)particleCount());
        return visfs_mcl_download(f_, x ? x->data() : nullptr, y ? y->data() : nullptr, yaw ? yaw->data() : nullptr, w ? w->data() : nullptr,
                                  nullptr, nullptr);
    }
    // what the last init or update issued on the device (all zero on the twin)
    void lastCounts(int* launches, int* copies, int* waits) const {
        int32_t k = 0, c = 0, w = 0;
        visfs_mcl_last_counts(f_, &k, &c, &w);
        if (launches) *launches = k;
        if (copies) *copies = c;
        if (waits) *waits = w;
    }
    const char* lastError() const { return visfs_mcl_last_error(f_); }

private:
    visfs_mcl* f_ = nullptr;
    int n_ = 0;
};

}  // namespace VISFS

#endif
