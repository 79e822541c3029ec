/*
 * visfs_mcl.h — Monte-Carlo localisation on the likelihood field of a global map (implemented in libvisfs_ba_hip.so).
 *
 * A visfs_mcl_field is the exact squared Euclidean distance, in cells and clamped, from every cell of an occupancy grid to its
 * nearest occupied cell, with a fixed-point table of the likelihood-field laser model over it.  A visfs_mcl is a particle filter
 * on such a field: odometry motion model (Probabilistic Robotics' sample_motion_model_odometry), likelihood-field weights,
 * weighted mean and covariance, systematic resampling.  Objects made on a visfs_ba handle live in device memory and run HIP
 * kernels on the handle's device and stream; objects made with h == NULL are the one-core host twin; both give the same bytes.
 * DESIGN.md section 9t states every step.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.  Every refusal is decided on the host before anything is pushed, and leaves the
 * particles, the last result and the last counts in place.
 */
#ifndef VISFS_MCL_H
#define VISFS_MCL_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_submap.h"
#include "visfs_map.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_MCL_ABI_VERSION 1

#define VISFS_MCL_MAX_RADIUS 255          /* cells: floor(max_dist / resolution) */
#define VISFS_MCL_MAX_PARTICLES 65536
#define VISFS_MCL_MAX_BEAMS 16384
/* What the device issues per call (the twin issues nothing): the same for every N, n and grid size. */
#define VISFS_MCL_FIELD_LAUNCHES 2
#define VISFS_MCL_INIT_LAUNCHES 1
#define VISFS_MCL_UPDATE_LAUNCHES 4

typedef struct visfs_mcl_field_params {
    double occupied_probability;  /* a cell is an obstacle when its probability is at least this; default 0.65 */
    double max_dist;              /* laser_likelihood_max_dist, metres; default 2.0 */
    double z_hit, z_rand;         /* defaults 0.5, 0.5 */
    double sigma_hit;             /* default 0.2 */
    double range_max;             /* default 12.0 */
} visfs_mcl_field_params;

typedef struct visfs_mcl_field_info {
    visfs_submap_info limits;     /* resolution, max_x, max_y, num_x_cells, num_y_cells; the known box is empty (min > max) */
    int32_t R, T;                 /* floor(max_dist / res), ceil((max_dist / res)^2): the field's largest value */
    int32_t v_occ;                /* values 1 .. v_occ are obstacles */
    int32_t device;
} visfs_mcl_field_info;

typedef struct visfs_mcl_params {
    double  alpha1, alpha2, alpha3, alpha4;   /* odom_alpha1..4; defaults 0.2 */
    double  n_eff_ratio;                      /* resample when n_eff < n_eff_ratio * N; default 1.0 */
    int32_t resample_interval;                /* ... and the update counter is a multiple of this; >= 1, default 2 */
    int32_t max_beams;                        /* every ceil(n / max_beams)-th point is used; 0 (default): all */
} visfs_mcl_params;

typedef struct visfs_mcl_result {
    int32_t status;
    int32_t resampled;            /* 1: this update resampled */
    int32_t best;                 /* the particle of the largest weight before resampling (the lowest index among equals) */
    int32_t n_beams;              /* the points used */
    int64_t update;               /* the update counter: 1 after the first update since visfs_mcl_init */
    double  mean[3];              /* x, y, yaw (atan2 of the weighted circular sums) */
    double  covariance[9];        /* row-major; [8] is the circular variance -2 ln |mean resultant|; yaw is uncorrelated as in AMCL */
    double  n_eff;                /* W^2 / sum w^2 */
    double  W;                    /* the sum of the weights before they were normalised */
    double  best_pose[3];
    double  best_weight;          /* normalised */
} visfs_mcl_result;

typedef struct visfs_mcl_field visfs_mcl_field;
typedef struct visfs_mcl visfs_mcl;

int  visfs_mcl_abi_version(void);
void visfs_mcl_field_default_params(visfs_mcl_field_params* p);
void visfs_mcl_default_params(visfs_mcl_params* p);

/* ---- the likelihood field ------------------------------------------------------------------------------------------------------ */
/* A cell of value v (v & 32767) is an obstacle iff 1 <= v <= v_occ, v_occ the largest value whose probability 1 - cost(v)
 * (visfs_submap_hook_value_tables) is at least occupied_probability.  Value 0 and everything outside the grid is no obstacle.
 * t[iy][ix] = min(T, min over obstacles of dx^2 + dy^2), uint16.  q[t] = llround(pz^3 2^40), pz = z_hit exp(-z^2 / (2 sigma_hit^2))
 * + z_rand / range_max, z = res sqrt(t) for t < T and max_dist at t = T.
 * BAD_ARGUMENT: a parameter that is not finite and positive, occupied_probability above 1, q[0] above 2^48 (a sum over 16384
 * beams must stay below 2^62).  UNSUPPORTED: R > 255 or T > 65535.
 * From the last composed grid of `m`, read where it lives; the field is of the map's flavour, device and stream and outlives it.
 * On the device: one upload (the parameters and the table), VISFS_MCL_FIELD_LAUNCHES launches, one wait. */
int  visfs_mcl_field_create_from_map(visfs_map* m, const visfs_mcl_field_params* p, visfs_mcl_field** out);
/* The same from host cells [num_y_cells][num_x_cells] and limits as visfs_map_download and visfs_submaps_download hand them out. */
int  visfs_mcl_field_create_from_grid(visfs_ba_handle* h, const visfs_submap_info* limits, const uint16_t* cells,
                                      const visfs_mcl_field_params* p, visfs_mcl_field** out);
void visfs_mcl_field_destroy(visfs_mcl_field* f);
int  visfs_mcl_field_describe(const visfs_mcl_field* f, visfs_mcl_field_info* info);
/* t [num_y_cells][num_x_cells], q [T + 1]; every pointer may be NULL. */
int  visfs_mcl_field_download(visfs_mcl_field* f, uint16_t* t, int64_t* q, int32_t* v_occ, int32_t* T);
/* What creating the field issued on the device (all zero on the twin; `copies` leaves out the cells of create_from_grid). */
int  visfs_mcl_field_last_counts(const visfs_mcl_field* f, int32_t* launches, int32_t* copies, int32_t* waits);

/* ---- the filter ---------------------------------------------------------------------------------------------------------------- */
/* 1 <= n_particles <= 65536.  The filter is of the field's flavour, device and stream; the field must outlive it. */
int  visfs_mcl_create(visfs_mcl_field* field, int32_t n_particles, uint64_t seed, visfs_mcl** out);
void visfs_mcl_destroy(visfs_mcl* f);
const char* visfs_mcl_last_error(const visfs_mcl* f);
/* Particle j = mean + sigma o (g0, g1, g2) (yaw wrapped), w = 1 / N; the update counter returns to 0.  sigma >= 0.
 * On the device: one upload, VISFS_MCL_INIT_LAUNCHES launch, one wait. */
int  visfs_mcl_init(visfs_mcl* f, const double mean[3], const double sigma[3]);
/* One filter step: motion by odom_delta = (dx, dy, dyaw) in the previous robot frame, weights from points_xyz[n][3] (robot frame,
 * z ignored; 0 <= n <= 16384), sums, resampling.  BAD_ARGUMENT: a value that is not finite, a negative alpha, or
 * |rot1 + rot2| + 6 (sigma_rot1 + sigma_rot2) above 2 pi: the noise is bounded by 6 sigma, so below that a yaw needs one wrap.
 *  `result` may be NULL.
 * On the device: one upload, VISFS_MCL_UPDATE_LAUNCHES launches, one download, one wait, whatever N and n are. */
int  visfs_mcl_update(visfs_mcl* f, const visfs_mcl_params* p, const double odom_delta[3], int32_t n, const double* points_xyz,
                      visfs_mcl_result* result);
/* The last update's result (status BAD_ARGUMENT before any). */
int  visfs_mcl_last_result(const visfs_mcl* f, visfs_mcl_result* result);

/* ---- hooks --------------------------------------------------------------------------------------------------------------------- */
/* The particles [N], the last update's integer sums Q [N] and ancestors [N] (the index itself when it did not resample; both zero
 * / the index before any update); every pointer may be NULL. */
int  visfs_mcl_download(visfs_mcl* f, double* x, double* y, double* yaw, double* w, int64_t* Q, int32_t* ancestors);
/* Replaces the particles: finite poses, yaw in (-pi, pi], finite weights >= 0 with a positive sum.  The counter is kept. */
int  visfs_mcl_upload(visfs_mcl* f, const double* x, const double* y, const double* yaw, const double* w);
/* The lanes that share one particle's beams in the weight kernel: 1, 2, 4, .. 64, or 0 for the library's choice (the default).
 * The results do not depend on it. */
int  visfs_mcl_hook_set_lanes(visfs_mcl* f, int32_t lanes);
/* What the last init or update issued on the device (all zero on the twin). */
int  visfs_mcl_last_counts(const visfs_mcl* f, int32_t* launches, int32_t* copies, int32_t* waits);
/* sincos_any of section 9t: sin and cos of `a`, |a| <= 16, as the filter forms them. */
int  visfs_mcl_hook_sincos(int32_t n, const double* a, double* s, double* c);

#ifdef __cplusplus
}
#endif
#endif
