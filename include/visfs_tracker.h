/*
 * visfs_tracker.h — the resident front end: Tracker::pretreatment + Tracker::imageProcess in one call (in libvisfs_ba_hip.so).
 *
 * The reference's Tracker (corelib/src/Tracker.cpp:98-419) keeps its state in std::maps between frames: the words of lastSignature_
 * with their 3-D points, trackCnt_, globalFeatureId_ and the blocked words of pretreatment.  Here that state is one table in the
 * memory of the visfs_flow object the tracker was made on (id, left pixel, 3-D point, track count, in ascending id order).
 * visfs_tracker_process takes a stereo pair in and hands the Signature's contents out: one upload, one sequence of launches, one
 * download and one synchronisation on an object of visfs_flow_create; the same steps on one core on an object of
 * visfs_flow_create_host.  DESIGN.md section 9h lists the steps, the quirks of the reference that are kept and the two things dropped.
 *
 * The flow keys (window, levels, gates, flow_back, depth gates) are those of the visfs_flow object.  Tracker/CullByFundationMatrix
 * (Tracker.cpp:275-277, :83-96) is part of this call since ABI 2: with `cull` set and the flow object's flow_back off, the mask of the
 * fundamental-matrix search of visfs_fund.h is ANDed into the Lucas-Kanade status between the temporal track and the reduce, on rows
 * that never leave the device.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_TRACKER_H
#define VISFS_TRACKER_H

#include <stdint.h>
#include "visfs_clahe.h"
#include "visfs_corners.h"
#include "visfs_flow.h"
#include "visfs_fund.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_TRACKER_ABI_VERSION  2
#define VISFS_TRACKER_MAX_FEATURES 4096
#define VISFS_TRACKER_MAX_OUTLIERS 4096

/* result flags */
#define VISFS_TRACKER_NO_PREVIOUS  1   /* nothing to track against: the pair was pushed, nothing else ran (Tracker.cpp:168) */
#define VISFS_TRACKER_BOOTSTRAPPED 2   /* the from-table was empty: its words were extracted from the previous pair (:179-230) */
#define VISFS_TRACKER_LOST         4   /* fewer than min_inliers words survived the reduce (:303): the table is empty now */

typedef struct visfs_tracker visfs_tracker;

typedef struct visfs_tracker_params {
    int32_t max_features;       /* Tracker/MaxFeatures   (default 300; 1 .. 4096) */
    double  quality_level;      /* Tracker/QualityLevel  (default 0.01; > 0) */
    int32_t min_distance;       /* Tracker/MinDistance   (default 40; 0 .. 32768); blocked words mask min_distance / 2 */
    int32_t min_inliers;        /* Estimator/MinInliers  (default 10; >= 0) */
    int32_t clahe;              /* System/CLAHE: 0 pushes the raw pair, else the pair equalised with clahe_params */
    visfs_clahe_params clahe_params;
    int32_t cull;               /* Tracker/CullByFundationMatrix (default 0).  As in the reference it runs only when the flow object's
                                 * flow_back is 0; with flow_back set the field is ignored */
    visfs_fund_params cull_params;  /* pixel_error: Tracker/FundationPixelError (default 1.0; <= 0 means 3.0), iterations (default
                                 * 1000; 1 .. 4096), seed (default 0; used as given in every call, as OpenCV's RANSAC restarts its
                                 * generator per call) */
} visfs_tracker_params;

/* The arrays belong to the tracker and stay valid until its next call.  Every list is in ascending id order, the order uKeys and
 * uValues give the reference's maps in. */
typedef struct visfs_tracker_result {
    int32_t  flags;
    int32_t  n_covisible, n_new, n_words, n_blocked;
    uint64_t next_id;                       /* globalFeatureId_ after the call */
    /* setCovisibleWords / setCovisibleWords3d / setkeyPointsMatchesFormer: the from_xyz and to_xy rows visfs_pnp_solve takes */
    const uint64_t* covisible_id;           /* [n_covisible] */
    const float*    covisible_from_xy;      /* [n_covisible][2] */
    const float*    covisible_from_xyz;     /* [n_covisible][3], NaN where a bootstrapped word was not triangulated */
    const float*    covisible_to_xy;        /* [n_covisible][2] */
    /* setKeyPointsNewExtract */
    const uint64_t* new_id;                 /* [n_new] */
    const float*    new_xy;                 /* [n_new][2] */
    /* setWords / setKeyPointMatchesImageRight / setWords3d, and the word_uv / word_xyz of visfs_window_insert */
    const uint64_t* word_id;                /* [n_words] */
    const float*    word_left_xy;           /* [n_words][2] */
    const float*    word_right_xy;          /* [n_words][2] */
    const float*    word_xyz;               /* [n_words][3], robot frame */
    const int32_t*  word_count;             /* [n_words], trackCnt_ after updateTrackCounter */
    /* setBlockedWords of the from-signature */
    const uint64_t* blocked_id;             /* [n_blocked] */
} visfs_tracker_result;

int  visfs_tracker_abi_version(void);
void visfs_tracker_default_params(visfs_tracker_params* p);      /* 300, 0.01, 40, 10, CLAHE off (3.0, 8, 8), cull off (1.0, 1000, 0) */

/* A tracker on the pyramids, device and stream of f (a visfs_flow_create or a visfs_flow_create_host object), which must outlive it.
 * cam: the stereo camera of visfs_flow_stereo.  The half-width tables of the two mask radii are made here.
 * VISFS_BA_ERR_UNSUPPORTED: max_features > 4096, min_distance > 32768.  VISFS_BA_ERR_BAD_ARGUMENT: max_features < 1, quality_level
 * not finite or <= 0, min_distance or min_inliers negative, a non-finite Tir, a CLAHE setting visfs_flow_push_frame_clahe refuses.
 * The cull fields are looked at only when cull != 0: VISFS_BA_ERR_BAD_ARGUMENT for iterations < 1 or a pixel_error that is not
 * finite, VISFS_BA_ERR_UNSUPPORTED for iterations > 4096.  Every buffer of the cull is allocated here.
 * (visfs_tracker_group_create is stricter: the members of a group must agree in cull and in every field of cull_params, as in every
 * other field of this struct, also where cull is 0 or flow_back makes it inert.) */
int  visfs_tracker_create(visfs_flow* f, const visfs_tracker_params* p, const visfs_flow_camera* cam, visfs_tracker** out);
void visfs_tracker_destroy(visfs_tracker* t);
const char* visfs_tracker_last_error(const visfs_tracker* t);
/* Empties the table; the id counter keeps counting.  The next call extracts its words afresh. */
int  visfs_tracker_reset(visfs_tracker* t);

/* One frame.  left, right: 8-bit grey, `stride` bytes per row.  delta_guess: getDeltaPoseGuess() as 3x4 row-major doubles, or NULL for
 * "not set".  outlier_ids[n_outliers]: Estimator::getOutliers() of the frame before (at most 4096; ids not in the table are ignored).
 * VISFS_BA_ERR_BAD_ARGUMENT: a NULL image or result, a stride below the width, n_outliers negative or above the cap, a non-finite
 * delta_guess.  VISFS_BA_ERR_NOT_LOADED: the images of f were pushed by somebody else since this tracker's last call; it does not
 * track against a "previous" it has no words for. */
int  visfs_tracker_process(visfs_tracker* t, const uint8_t* left, const uint8_t* right, int32_t stride, const double* delta_guess,
                           int32_t n_outliers, const uint64_t* outlier_ids, visfs_tracker_result* result);

/* ---- test hook --------------------------------------------------------------------------------------------------------------- */
/* Intermediate state of the last visfs_tracker_process call; any pointer may be NULL.
 * Per from-row (after pretreatment or the bootstrap; at most max_features): the initial flow handed to LK (the from-pixel itself
 * without a guess), cornersTo, the status after the gate, the bounds test of :286.
 * The disc list of getMask in draw order (at most 2 * max_features) with its drawn flags.
 * The stereo status per row of kept + new (at most max_features).
 * VISFS_BA_ERR_NOT_LOADED before the first call that got past NO_PREVIOUS. */
int  visfs_tracker_download(const visfs_tracker* t, int32_t* n_from, float* guess_xy, float* to_xy, uint8_t* lk_status,
                            uint8_t* in_bounds, int32_t* n_discs, visfs_corners_disc* discs, uint8_t* disc_drawn, int32_t* n_rows,
                            uint8_t* stereo_status);

/* The fundamental-matrix cull of the last visfs_tracker_process call that got past NO_PREVIOUS; any pointer may be NULL.  The values
 * mean what visfs_fund_cull, visfs_fund_last_sizes and visfs_fund_download report for the same from-rows: *applied (0: fewer than seven
 * rows entered and the status passed through), *m (rows with four finite coordinates), *n_hypotheses (0, 1 for seven rows, else
 * iterations), *n_inliers, mask[n_from], status[n_from] (the Lucas-Kanade status after the AND, which the reduce kept its rows on;
 * lk_status of visfs_tracker_download stays the status before it), F[9], T1[9], T2[9], the winner (h, k) or (-1, -1).
 * A tracker whose cull is inactive (cull == 0, or flow_back set) reports *applied = 0 and *m = 0, zeros elsewhere, writes neither mask
 * nor status and returns VISFS_BA_OK.  VISFS_BA_ERR_NOT_LOADED before the first call that got past NO_PREVIOUS. */
int  visfs_tracker_download_cull(const visfs_tracker* t, int32_t* applied, int32_t* m, int32_t* n_hypotheses, int32_t* n_inliers,
                                 uint8_t* mask, uint8_t* status, double* F, double* T1, double* T2, int32_t* winner_h,
                                 int32_t* winner_k);

#ifdef __cplusplus
}
#endif
#endif
