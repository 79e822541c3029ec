/*
 * visfs_fund.h — the fundamental-matrix cull of a tracked frame on the GPU (implemented in libvisfs_ba_hip.so).
 *
 * The reference's Tracker::rejectOutlierWithFundationMatrix (corelib/src/Tracker.cpp:83-96), which imageProcess runs when
 * Tracker/FlowBack is off (:275-277): cv::findFundamentalMat(cornersFrom, cornersTo, FM_RANSAC, Tracker/FundationPixelError, 0.99,
 * mask), the mask ANDed into the Lucas-Kanade status.  It sits between visfs_flow_track and visfs_pnp_solve.  On an object of
 * visfs_fund_create a call is one copy in, two HIP kernels (every hypothesis of the RANSAC search in one launch, then the mask of the
 * winner) and one copy out on the stream of the owning handle; on an object of visfs_fund_create_host the same arithmetic runs on
 * one core and gives the same bytes.
 *
 * DESIGN.md section 9f states every step.  cv::findFundamentalMat is restated from OpenCV's published algorithm; parity with OpenCV
 * itself is not pinned, and its random stream and its early exit at confidence 0.99 are replaced: the samples come from a counter
 * hash of (seed, hypothesis), and every hypothesis is evaluated.  There is no refit: as in OpenCV's RANSAC the result is the best
 * seven-point model and its mask.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_FUND_H
#define VISFS_FUND_H

#include <stdint.h>
#include "visfs_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_FUND_ABI_VERSION 1
#define VISFS_FUND_MAX_POINTS     4096
#define VISFS_FUND_MAX_ITERATIONS 4096

typedef struct visfs_fund_params {
    float    pixel_error;  /* Tracker/FundationPixelError (default 1.0); <= 0 means 3.0, as findFundamentalMat does */
    int32_t  iterations;   /* hypotheses, 1 .. 4096 (default 1000 = OpenCV's maxIters) */
    uint64_t seed;         /* sampling seed (default 0): a call is a pure function of its arguments */
} visfs_fund_params;

typedef struct visfs_fund visfs_fund;

int  visfs_fund_abi_version(void);
void visfs_fund_default_params(visfs_fund_params* p);

/* A cull for up to capacity_points rows (1 .. 4096, beyond: VISFS_BA_ERR_UNSUPPORTED) on the device and stream of handle `h`; every
 * buffer of a call is allocated here. */
int  visfs_fund_create(visfs_ba_handle* h, int32_t capacity_points, visfs_fund** out);
/* The host restatement (one core, no device): the same arithmetic in sequence, for parity tests. */
int  visfs_fund_create_host(int32_t capacity_points, visfs_fund** out);
void visfs_fund_destroy(visfs_fund* p);
const char* visfs_fund_last_error(const visfs_fund* p);

/* n rows: from_xy[n][2] (cornersFrom), to_xy[n][2] (cornersTo), status_in[n] (the Lucas-Kanade status; nonzero is set).
 *  - Every row whose four coordinates are finite enters the search, whatever its status (findFundamentalMat is given all corners);
 *    a row with a coordinate that is not finite is never sampled and its mask is 0.  m is the number of rows that enter.
 *  - mask_out[n]: 1 on the inliers of the winning model.  status_out[i] = status_in[i] && mask_out[i] (Tracker.cpp:89-95);
 *    status_out may be status_in.  *n_inliers: the number of ones in mask_out.  F_out[9] (row-major, may be NULL): the winning model
 *    on the raw pixels, x_to^T F x_from = 0, of unit Frobenius norm before the conditioning is taken off.
 *  - m < 7 (OpenCV returns an empty matrix and leaves the mask untouched): *applied = 0, status_out = (status_in != 0), mask_out and
 *    F_out all zero.  Otherwise *applied = 1.
 *  - m == 7: no search; mask_out is 1 on every row that entered, F_out the first model of those seven rows or zero without one.
 *  - m >= 8: the search.  A winner needs 7 inliers; without one mask_out, status_out and F_out are all zero.
 * The status is VISFS_BA_OK in all these cases.  VISFS_BA_ERR_BAD_ARGUMENT: a required pointer is null, n < 0 or above the capacity,
 * iterations < 1, a pixel_error that is not finite.  VISFS_BA_ERR_UNSUPPORTED: iterations > 4096. */
int  visfs_fund_cull(visfs_fund* p, const visfs_fund_params* params, int32_t n, const float* from_xy, const float* to_xy,
                     const uint8_t* status_in, uint8_t* status_out, uint8_t* mask_out, double* F_out, int32_t* n_inliers,
                     int32_t* applied);

/* ---- test hooks -------------------------------------------------------------------------------------------------------------- */
/* Sizes of the last visfs_fund_cull call of p: rows that entered and hypotheses evaluated (0 when m < 7; 1 when
 * m == 7: the seven rows themselves, reported as hypothesis 0 with counts of zero).
 * VISFS_BA_ERR_NOT_LOADED before the first call. */
int  visfs_fund_last_sizes(const visfs_fund* p, int32_t* m, int32_t* n_hypotheses);
/* State of the last call; any pointer may be NULL.  Per hypothesis: samples[h][7] (numbers among the rows that entered), n_models[h]
 * (0 .. 3; 0: the sample is invalid), models[h][3][9] (the conditioned models F^ in their order, zero behind n_models[h]),
 * counts[h][3].  *winner_h, *winner_k: the winning hypothesis and model, or -1.  T1[9], T2[9]: the two Hartley transforms (row-major;
 * zero when m < 7). */
int  visfs_fund_download(visfs_fund* p, int32_t* samples, int32_t* n_models, double* models, int32_t* counts, int32_t* winner_h,
                         int32_t* winner_k, double* T1, double* T2);

#ifdef __cplusplus
}
#endif
#endif
