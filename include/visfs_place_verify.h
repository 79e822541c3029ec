/*
 * visfs_place_verify.h — a place query whose candidates are verified by PnP in the same call, and the loop-closure edge of a
 * verified candidate (implemented in libvisfs_ba_hip.so).  DESIGN.md section 9x is the definition.
 *
 * visfs_place_query (visfs_place.h) returns up to eight candidate key-frames with the rows visfs_pnp_solve takes.  Whether a
 * candidate is the same place is decided by a PnP-RANSAC pose with enough inliers.  visfs_place_query_verify runs the query, then
 *   stage 1: per candidate, what visfs_pnp_solve gives on the candidate's rows (byte for byte, one seed for all candidates);
 *   stage 2: per candidate with a stage-1 pose, a guided search: the key-frame's 3-D points are projected with that pose, every entry
 *            looks for the nearest descriptor among the query's key-points inside a small window, the pairs are made one to one, and
 *            the pose is refined on them from the stage-1 model (no new RANSAC search);
 * on rows that never leave the device: one upload, seven launches, one download and one wait for zero to eight candidates.
 *
 * A verifier made on a device store runs HIP kernels on the stream of the store's handle; one made on a store of
 * visfs_place_db_create(NULL, ...) runs the same arithmetic on one core and gives the same bytes.  A verifier must be destroyed
 * before its store.  Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_PLACE_VERIFY_H
#define VISFS_PLACE_VERIFY_H

#include <stdint.h>
#include "visfs_place.h"
#include "visfs_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_PLACE_VERIFY_ABI_VERSION 1
#define VISFS_PLACE_VERIFY_LAUNCHES    7

typedef struct visfs_place_verifier visfs_place_verifier;

typedef struct visfs_place_verify_params {
    visfs_pnp_params pnp;               /* visfs_pnp_default_params */
    visfs_pnp_camera camera;            /* no default: the caller's */
    int32_t guided;                     /* default 1; 0: stage 2 does not run */
    float   guided_radius;              /* default 6.0 px = 3 x reproj_error; finite and >= 0 */
    int32_t guided_max_distance;        /* default 64 (the default max_distance of visfs_place_params); 0 .. 256 */
    int32_t pad;
} visfs_place_verify_params;

typedef struct visfs_place_verify_stage1 {      /* what visfs_pnp_solve returns on row[c][0 .. count) */
    int32_t n_matches, n_inliers;
    int32_t matches[VISFS_PLACE_MAX_POINTS];    /* row numbers of row[c]; unused: zero */
    int32_t inliers[VISFS_PLACE_MAX_POINTS];    /* row numbers of row[c]; unused: zero */
    double  T[16];                              /* all zero: no pose */
    double  cov[36];
} visfs_place_verify_stage1;

typedef struct visfs_place_verify_stage2 {
    int32_t ran, n_rows;                        /* ran: guided was set and stage 1 left a pose */
    visfs_place_row row[VISFS_PLACE_MAX_POINTS];    /* the guided rows, ascending query_index; unused: zero */
    int32_t n_inliers, pad;
    int32_t inliers[VISFS_PLACE_MAX_POINTS];    /* numbers of the guided rows; unused: zero */
    double  T[16];                              /* all zero: no pose (fewer than min_inliers guided rows or inliers) */
    double  cov[36];                            /* the identity with the zero transform when ran, all zero when not */
} visfs_place_verify_stage2;

typedef struct visfs_place_verify_candidate {
    visfs_place_verify_stage1 stage1;
    visfs_place_verify_stage2 stage2;
} visfs_place_verify_candidate;

typedef struct visfs_place_verify_result {
    int32_t status;                     /* VISFS_BA_OK */
    int32_t best;                       /* the candidate with the most final inliers (stage 2's where it ran, else stage 1's), at least
                                           min_inliers of them (raised to 4 as visfs_pnp_solve does); the lowest c among equals; -1: none */
    visfs_place_verify_candidate candidate[VISFS_PLACE_MAX_CANDIDATES];     /* candidates from n_candidates on: zero */
} visfs_place_verify_result;

int  visfs_place_verify_abi_version(void);
/* PnP defaults, guided 1, guided_radius 6.0, guided_max_distance 64; the camera is zeroed (a zero focal length is refused). */
void visfs_place_verify_default_params(visfs_place_verify_params* p);

/* A verifier of the flavour of db; every buffer of a call is allocated here. */
int  visfs_place_verifier_create(visfs_place_db* db, visfs_place_verifier** out);
void visfs_place_verifier_destroy(visfs_place_verifier* v);
const char* visfs_place_verifier_last_error(const visfs_place_verifier* v);

/* visfs_place_query(db, set, place_params, place_result) followed by the two stages on every candidate.  place_result is byte for
 * byte what visfs_place_query gives.  query_xyz [n of the set][3] or NULL: the 3-D positions of the query's key-points now, for the
 * covariance only (the to_xyz of visfs_pnp_solve, taken at row.query_index).
 * Refused on the host before anything is pushed, with the codes of visfs_place_query and visfs_pnp_solve:
 * VISFS_BA_ERR_BAD_ARGUMENT: a place parameter out of range, different flavours, iterations < 1, refine_iterations < 0, a threshold or
 * the radius not finite or negative, guided_max_distance outside 0 .. 256, a camera value not finite or a zero focal length;
 * VISFS_BA_ERR_UNSUPPORTED: iterations > 4096, refine_iterations > 32; VISFS_BA_ERR_NOT_LOADED: the set was never described. */
int  visfs_place_query_verify(visfs_place_verifier* v, const visfs_place_set* set, const visfs_place_params* place_params,
                              const visfs_place_verify_params* verify_params, const float* query_xyz, visfs_place_result* place_result,
                              visfs_place_verify_result* verify_result);
/* uploads, launches, downloads and stream waits of the last visfs_place_query_verify of v (all 0 on the twin) */
int  visfs_place_verify_last_counts(const visfs_place_verifier* v, int32_t* uploads, int32_t* launches, int32_t* downloads, int32_t* waits);

/* ---- test hooks --------------------------------------------------------------------------------------------------------------- */
/* What visfs_pnp_last_sizes and visfs_pnp_download report for candidate c's stage (1 or 2) of the last call; any pointer may be
 * NULL.  Stage 2 has no hypotheses: *n_hypotheses is 0 and *winner -1.  A stage that did not run: all sizes 0, winner -1.
 * VISFS_BA_ERR_NOT_LOADED before the first call, VISFS_BA_ERR_BAD_ARGUMENT for c outside 0 .. 7 or a stage other than 1 and 2. */
int  visfs_place_verify_download_pnp(visfs_place_verifier* v, int32_t c, int32_t stage, int32_t* m, int32_t* n_hypotheses, int32_t* n_passes,
                                     int32_t* samples, int32_t* valid, double* models, int32_t* counts, int32_t* winner, double* refit_tq,
                                     double* pass_tq, float* pass_threshold, int32_t* pass_count, int32_t* pass_inliers);
/* The guided stage of candidate c: pick[512] per entry of the slot (D * 1024 + i of the query it picked, -1: none) and keep[512]
 * per query (D * 1024 + j of the entry it keeps, -1: none); all -1 when stage 2 did not run for c. */
int  visfs_place_verify_download_guided(visfs_place_verifier* v, int32_t c, int32_t* pick, int32_t* keep);

/* The window test of the guided stage on one pair: 1 iff the query at (qx, qy) lies within `radius` of the projection (pu, pv). */
int  visfs_place_verify_hook_window(double pu, double pv, float qx, float qy, float radius);

/* ---- host-only helper --------------------------------------------------------------------------------------------------------- */
/* The loop-closure edge of a verified candidate.  T[16] and cov[36] are a stage's: T is the reference's `transform`,
 * (Tir * pnp)^-1, which takes a point in the robot frame of the query to the robot frame of the key-frame, that is the pose of
 * the query (vertex j) in the frame of the key-frame (vertex i); tests/test_place_verify_host.py holds this to a scene's true pose.
 * z_out = (T[3], T[7], atan2(T[4], T[0])): what visfs_pose_graph_edge takes between i and j.  information_out: the inverse of the
 * 3 x 3 block of cov over (x, y, yaw) (cov is ordered x y z roll pitch yaw), symmetrised.  out_of_plane = (z, roll, pitch) of T
 * (yaw-pitch-roll angles), so the caller can gate a pose that leaves the plane.
 * VISFS_BA_ERR_BAD_ARGUMENT: a NULL or non-finite input, the all-zero transform, a block that is not positive definite. */
int  visfs_place_closure_edge(const double T[16], const double cov[36], double z_out[3], double information_out[9], double out_of_plane[3]);

#ifdef __cplusplus
}
#endif
#endif
