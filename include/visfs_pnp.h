/*
 * visfs_pnp.h — the PnP-RANSAC pose guess of a frame on the GPU (implemented in libvisfs_ba_hip.so).
 *
 * The reference's estimateMotion3DTo2D (corelib/src/MultiviewGeometry.cpp:94-216) and the solvePnPRansac wrapper it calls
 * (:219-315): from the 3-D words of the frame before and their pixels in this frame, the pose that LocalMap::insertSignature and
 * localOptimize start from, its inliers and its covariance.  On an object of visfs_pnp_create a call is two HIP kernels on the stream
 * of the owning handle (every hypothesis of the RANSAC search in one launch, the refit and the whole refinement loop in one
 * workgroup); on an object of visfs_pnp_create_host the same arithmetic runs on one core and gives the same bytes.  The id matching
 * of :113-129 is done by the caller (visfs_amd/host/MotionEstimator.h does it over std::map); this interface takes rows.
 *
 * DESIGN.md section 9e states every step.  cv::solvePnPRansac is restated from OpenCV's published algorithm; parity with OpenCV
 * itself is not pinned, and its random stream and its early exit at confidence 0.99 are replaced: the samples come from a counter
 * hash of (seed, hypothesis), and every hypothesis is evaluated.  Lens distortion and Estimator/PnPFlags are not carried: the camera
 * is the rectified one visfs_flow_camera assumes, the minimal solver is P3P and the refit is iterative.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_PNP_H
#define VISFS_PNP_H

#include <stdint.h>
#include "visfs_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_PNP_ABI_VERSION 1
#define VISFS_PNP_MAX_POINTS      4096
#define VISFS_PNP_MAX_ITERATIONS  4096
#define VISFS_PNP_MAX_REFINE      32

typedef struct visfs_pnp_params {
    int32_t  min_inliers;       /* Estimator/MinInliers       (default 12); below 4 is raised to 4 (:234), in every test of a call */
    int32_t  iterations;        /* Estimator/PnPIterations    (default 50): hypotheses, 1 .. 4096 */
    float    reproj_error;      /* Estimator/PnPReprojError   (default 2.0), px */
    int32_t  refine_iterations; /* Estimator/RefineIterations (default 5; 0 .. 32) */
    float    refine_sigma;      /* 3.0 (MultiviewGeometry.h:130) */
    uint64_t seed;              /* sampling seed (default 0): a call is a pure function of its arguments */
} visfs_pnp_params;

/* cvKdouble() and getTansformImageToRobot() (3x4 row-major) of the GeometricCamera. */
typedef struct visfs_pnp_camera {
    double fx, fy, cx, cy;
    double Tir[12];
} visfs_pnp_camera;

typedef struct visfs_pnp visfs_pnp;

int  visfs_pnp_abi_version(void);
void visfs_pnp_default_params(visfs_pnp_params* p);

/* A solver for up to capacity_points rows (1 .. 4096, beyond: VISFS_BA_ERR_UNSUPPORTED) on the device and stream of handle `h`;
 * every buffer of a call is allocated here. */
int  visfs_pnp_create(visfs_ba_handle* h, int32_t capacity_points, visfs_pnp** out);
/* The host restatement (one core, no device): the same arithmetic in sequence, for parity tests. */
int  visfs_pnp_create_host(int32_t capacity_points, visfs_pnp** out);
void visfs_pnp_destroy(visfs_pnp* p);
const char* visfs_pnp_last_error(const visfs_pnp* p);

/* n rows: from_xyz[n][3] (the word in the robot frame of the frame before), to_xy[n][2] (its pixel now), to_xyz[n][3] or NULL (its
 * 3-D position now, for the covariance only).
 *  - A row is kept when its from_xyz is finite; matches_out[*n_matches] holds the kept row numbers in input order.
 *  - T_out[16] (4x4 row-major) is the reference's `transform`, (Tir * pnp)^-1, or the all-zero matrix (the sentinel Estimator.cpp:209
 *    tests) when fewer than min_inliers rows are kept or fewer than min_inliers inliers remain.  As the reference is written
 *    (:241-245), that is also the result when the RANSAC winner has fewer than min_inliers inliers and when refine_iterations == 0:
 *    `_inliers` is never assigned then, so there are no inliers.
 *  - inliers_out[*n_inliers]: row numbers of the inliers (the list of the refinement pass before the last selection, :278, :310).
 *  - cov_out[36] (6x6 row-major): :159-205, with to_xyz the two medians x 2.1981, without it the rms reprojection form; identity
 *    with the zero transform.
 * matches_out and inliers_out have room for n entries.  The status is VISFS_BA_OK in all these cases.
 * VISFS_BA_ERR_BAD_ARGUMENT: n < 0 or above the capacity, iterations < 1, refine_iterations < 0, a threshold that is not finite or
 * is negative, a camera value that is not finite or a zero focal length.  VISFS_BA_ERR_UNSUPPORTED: iterations > 4096,
 * refine_iterations > 32. */
int  visfs_pnp_solve(visfs_pnp* p, const visfs_pnp_params* params, const visfs_pnp_camera* camera, int32_t n, const float* from_xyz,
                     const float* to_xy, const float* to_xyz, double* T_out, double* cov_out, int32_t* matches_out, int32_t* n_matches,
                     int32_t* inliers_out, int32_t* n_inliers);

/* ---- test hooks -------------------------------------------------------------------------------------------------------------- */
/* Sizes of the last visfs_pnp_solve call of p: kept rows, hypotheses evaluated (0 when too few rows were kept) and refinement
 * passes.  VISFS_BA_ERR_NOT_LOADED before the first call. */
int  visfs_pnp_last_sizes(const visfs_pnp* p, int32_t* m, int32_t* n_hypotheses, int32_t* n_passes);
/* State of the last call; any pointer may be NULL.  Per hypothesis: samples[h][4] (kept-row numbers), valid[h], models[h][12]
 * (R|t of the camera-frame pose, 3x4 row-major; zero when not valid), counts[h].  *winner: the winning hypothesis or -1;
 * refit_tq[7]: the refit on the winner's inliers (t, then q as x y z w).  Per refinement pass: pass_tq[k][7] after its refit,
 * pass_threshold[k] that selected with it, pass_count[k] and pass_inliers[k][m] (kept-row numbers, the first pass_count[k] valid). */
int  visfs_pnp_download(visfs_pnp* p, int32_t* samples, int32_t* valid, double* models, int32_t* counts, int32_t* winner,
                        double* refit_tq, double* pass_tq, float* pass_threshold, int32_t* pass_count, int32_t* pass_inliers);

#ifdef __cplusplus
}
#endif
#endif
