/*
 * visfs_tracker_pnp.h — the PnP-RANSAC pose guess inside the resident front end (implemented in libvisfs_ba_hip.so).
 *
 * visfs_tracker_process and visfs_tracker_group_process (visfs_tracker.h, visfs_tracker_group.h) hand out the covisible rows that
 * visfs_pnp_solve (visfs_pnp.h) takes.  With the pose guess enabled on a tracker, estimateMotion3DTo2D
 * (corelib/src/MultiviewGeometry.cpp:94-216) runs inside those calls on the rows where they are: on a device tracker three more
 * launches of the call's one launch sequence, whatever the number of members, and the result in the call's one download; on a
 * host-twin tracker the same steps in sequence.  DESIGN.md section 9k.
 *
 * The result is byte for byte what visfs_pnp_solve returns for n = n_covisible, from_xyz = covisible_from_xyz,
 * to_xy = covisible_to_xy of the same call and the tracker's own camera (fx, fy, cx, cy and Tir of its visfs_flow_camera), with
 * to_xyz = NULL when the call's n_words is 0 (the reference tests _words3dTo.size(), MultiviewGeometry.cpp:160) and otherwise, per
 * covisible row, the word_xyz of the word with the same id in this call's word list, or a NaN triple when the id is not among the
 * words.  visfs_tracker.h stays at its ABI; this interface has its own.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_TRACKER_PNP_H
#define VISFS_TRACKER_PNP_H

#include <stdint.h>
#include "visfs_pnp.h"
#include "visfs_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_TRACKER_PNP_ABI_VERSION 1

/* What visfs_pnp_solve hands back through its output arguments.  The arrays belong to the tracker and stay valid until its next
 * process call (or its next visfs_tracker_enable_pnp). */
typedef struct visfs_tracker_pnp_result {
    int32_t ran;                /* 0: the pose guess is off, or the call was VISFS_TRACKER_NO_PREVIOUS: counts 0, T zero, cov identity */
    int32_t n_matches;          /* covisible rows with a finite from_xyz */
    int32_t n_inliers;
    int32_t pad;
    const int32_t* matches;     /* [n_matches] covisible row numbers, ascending */
    const int32_t* inliers;     /* [n_inliers] covisible row numbers */
    double T[16];               /* (Tir * pnp)^-1, 4x4 row-major, or all zero (the sentinel) */
    double cov[36];             /* 6x6 row-major; the identity with the sentinel */
} visfs_tracker_pnp_result;

int visfs_tracker_pnp_abi_version(void);

/* From the tracker's next process call on (single or grouped) the pose guess runs inside it with parameters *p, the seed as given
 * in every call; p == NULL switches it off again, after which every call is what it was before.  Every buffer is allocated here,
 * sized by the tracker's max_features and p->iterations; a call allocates nothing.  The arrays of a visfs_tracker_result handed
 * out before are no longer valid afterwards.
 * Refusals are those of visfs_pnp_solve's parameter check, with its codes.  VISFS_BA_ERR_BAD_ARGUMENT for a tracker that is in a
 * group: enable first, then create the group.  visfs_tracker_group_create requires its members to agree on whether the pose guess
 * is on and on every field of its parameters. */
int visfs_tracker_enable_pnp(visfs_tracker* t, const visfs_pnp_params* p);

/* The pose guess of the tracker's last process call.  It came down with that call's one download: nothing is issued to the
 * device and nothing is waited for.  VISFS_BA_ERR_NOT_LOADED before the tracker's first process call. */
int visfs_tracker_pnp_last(const visfs_tracker* t, visfs_tracker_pnp_result* out);

/* ---- test hook ----------------------------------------------------------------------------------------------------------------- */
/* What visfs_pnp_last_sizes and visfs_pnp_download report for the same rows; any pointer may be NULL, so a first call can ask
 * for the sizes alone.  samples[h][4], valid[h], models[h][12], counts[h] per hypothesis; pass_tq[k][7], pass_threshold[k],
 * pass_count[k], pass_inliers[k][m] per refinement pass.  When the pose guess did not run in the last call the sizes are 0, the
 * winner is -1 and the status is VISFS_BA_OK.  VISFS_BA_ERR_NOT_LOADED when there is no call to report on. */
int visfs_tracker_download_pnp(const visfs_tracker* t, int32_t* m, int32_t* n_hypotheses, int32_t* n_passes, int32_t* samples,
                               int32_t* valid, double* models, int32_t* counts, int32_t* winner, double* refit_tq, double* pass_tq,
                               float* pass_threshold, int32_t* pass_count, int32_t* pass_inliers);

#ifdef __cplusplus
}
#endif
#endif
