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
 * (flowBack off, Tracker.cpp:275) is not part of this call: a caller that needs it runs the staged chain (visfs_flow_track ->
 * visfs_fund_cull of visfs_fund.h -> its own reduce) instead.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_TRACKER_H
#define VISFS_TRACKER_H

#include <stdint.h>
#include "visfs_clahe.h"
#include "visfs_corners.h"
#include "visfs_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_TRACKER_ABI_VERSION  1
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
void visfs_tracker_default_params(visfs_tracker_params* p);      /* 300, 0.01, 40, 10, CLAHE off (3.0, 8, 8) */

/* A tracker on the pyramids, device and stream of f (a visfs_flow_create or a visfs_flow_create_host object), which must outlive it.
 * cam: the stereo camera of visfs_flow_stereo.  The half-width tables of the two mask radii are made here.
 * VISFS_BA_ERR_UNSUPPORTED: max_features > 4096, min_distance > 32768.  VISFS_BA_ERR_BAD_ARGUMENT: max_features < 1, quality_level
 * not finite or <= 0, min_distance or min_inliers negative, a non-finite Tir, a CLAHE setting visfs_flow_push_frame_clahe refuses. */
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

#ifdef __cplusplus
}
#endif
#endif
