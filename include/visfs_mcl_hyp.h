/*
 * visfs_mcl_hyp.h — AMCL's pose hypotheses for the KLD filter of visfs_mcl_kld.h (implemented in libvisfs_ba_hip.so).
 *
 * After visfs_mcl_hyp_enable every update that resamples also clusters the new particle set as AMCL's pf_cluster_stats does: the
 * occupied histogram bins (the bins of visfs_mcl_kld.h) are grouped into connected clusters (two bins are adjacent when each of
 * their three indices differs by at most 1; the yaw index does not wrap), every cluster gets its particle count, and the at most
 * VISFS_MCL_HYP_MAX clusters with the most particles get their mean pose and covariance.  hyp[0] is the pose AMCL would publish.
 * On the device this runs inside the resampling launch: an update stays one upload, VISFS_MCL_UPDATE_LAUNCHES launches, one
 * download and one wait.  The device and the one-core host twin give the same bytes.  DESIGN.md section 9v states every step.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.  Every refusal is decided on the host before anything is pushed, and leaves the
 * filter as it was.
 */
#ifndef VISFS_MCL_HYP_H
#define VISFS_MCL_HYP_H

#include <stdint.h>
#include "visfs_mcl.h"
#include "visfs_mcl_kld.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_MCL_HYP_ABI_VERSION 1

#define VISFS_MCL_HYP_MAX 8                 /* the hypotheses kept: the clusters with the most particles */

typedef struct visfs_mcl_hypothesis {
    int32_t label;                /* the lowest draw index of the cluster's bins: its name, whatever the schedule */
    int32_t count;                /* its particles */
    int32_t bins;                 /* its histogram bins */
    int32_t pad;
    double  weight;               /* count / n */
    double  mean[3];              /* x, y and the circular mean of the yaw */
    double  covariance[9];        /* row-major; x, y from the moments, [8] = -2 ln of the mean resultant length, yaw uncorrelated */
} visfs_mcl_hypothesis;

typedef struct visfs_mcl_hyp_result {
    int32_t fresh;                /* 1: the last update resampled and computed these */
    int32_t n_clusters;           /* every cluster of the new set, also those beyond VISFS_MCL_HYP_MAX */
    int32_t n_hypotheses;         /* min(n_clusters, VISFS_MCL_HYP_MAX); 0: none since the particles were last replaced */
    int32_t n;                    /* the n_after they describe */
    int64_t update;               /* the update that computed them */
    visfs_mcl_hypothesis hyp[VISFS_MCL_HYP_MAX];   /* by count descending, then label ascending; unused entries zero */
} visfs_mcl_hyp_result;

int visfs_mcl_hyp_abi_version(void);

/* From now on every resampling of the KLD filter `f` computes the hypotheses of its new set.  Idempotent; there is no way back.
 * BAD_ARGUMENT on a filter that is no KLD filter (visfs_mcl_kld_enable first). */
int visfs_mcl_hyp_enable(visfs_mcl* f);
/* The hypotheses of the last resampling.  An update that does not resample keeps them and clears `fresh`; visfs_mcl_init,
 * visfs_mcl_upload and visfs_mcl_kld_upload remove them (all zero) until the next resampling.  BAD_ARGUMENT, and zeros, when
 * hypotheses are not enabled. */
int visfs_mcl_hyp_last(const visfs_mcl* f, visfs_mcl_hyp_result* r);

/* ---- hooks --------------------------------------------------------------------------------------------------------------------- */
/* label [n] of the last resampling: the cluster label of every particle of its new set.  BAD_ARGUMENT when there are no
 * hypotheses. */
int visfs_mcl_hyp_download_labels(visfs_mcl* f, int32_t* label);
/* The propagation rounds the last device resampling ran (0 on the twin).  Informational: it depends on the schedule. */
int visfs_mcl_hyp_hook_rounds(const visfs_mcl* f, int32_t* rounds);

#ifdef __cplusplus
}
#endif
#endif
