/*
 * visfs_mcl_kld.h — KLD-adaptive particle counts for the Monte-Carlo localiser of visfs_mcl.h (implemented in libvisfs_ba_hip.so).
 *
 * A KLD filter has the capacity N it was created with and an active count n, 1 <= n <= N.  An update runs the plain filter's
 * steps on the n active particles; when it resamples, it draws up to N new particles one after the other, counts the histogram
 * bins (bin_xy x bin_xy x bin_yaw) that hold a drawn particle, and stops at the first draw count that exceeds the KLD limit of
 * that bin count (AMCL's pf_update_resample with pf_resample_limit).  The draw count at the stop is the next n.  The device and
 * the one-core host twin give the same bytes.  DESIGN.md section 9u states every step.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.  Every refusal is decided on the host before anything is pushed, and leaves the
 * particles, the count, the parameters, the last results and the last counts in place.
 */
#ifndef VISFS_MCL_KLD_H
#define VISFS_MCL_KLD_H

#include <stdint.h>
#include "visfs_mcl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_MCL_KLD_ABI_VERSION 1

#define VISFS_MCL_KLD_MAX_PARTICLES 16384   /* the capacity: two table slots per draw fill the 128 KiB of LDS */
#define VISFS_MCL_KLD_BIN_CLAMP 16777216    /* every bin index is clamped to [-2^24, 2^24] */

typedef struct visfs_mcl_kld_params {
    int32_t min_particles;        /* the limit is never below this; 1 .. N, default 100 */
    double  kld_err, kld_z;       /* defaults 0.01, 0.99; kld_z enters as z itself */
    double  bin_xy, bin_yaw;      /* the histogram's bin sizes, metres and radians; defaults 0.5, pi / 18 */
} visfs_mcl_kld_params;

typedef struct visfs_mcl_kld_result {
    int32_t n_before;             /* the count the last update ran with */
    int32_t n_after;              /* the count from the next update on; n_before when the update did not resample */
    int32_t bins;                 /* k at the stop; 0 when the update did not resample */
    int32_t limit;                /* limit[bins]; 0 when the update did not resample */
} visfs_mcl_kld_result;

int  visfs_mcl_kld_abi_version(void);
void visfs_mcl_kld_default_params(visfs_mcl_kld_params* p);

/* Makes `f` a KLD filter, or replaces the parameters of one; there is no way back.  The particles, the update counter and the
 * active count are kept.  The table limit[0 .. N] is made here and, on the device, uploaded here: limit[k] = N for k <= 1, else
 * b = 2 / (9 (k - 1)), x = 1 - b + sqrt(b) kld_z, limit = ceil((k - 1) / (2 kld_err) x^3) clamped to [min_particles, N].
 * BAD_ARGUMENT: min_particles outside 1 .. N, a value that is not finite and positive, kld_err >= 1.  UNSUPPORTED: N > 16384.
 * From then on visfs_mcl_update resamples as the head of this file says (on the device: still one upload,
 * VISFS_MCL_UPDATE_LAUNCHES launches, one download, one wait), visfs_mcl_init and visfs_mcl_upload set the count to N, and
 * visfs_mcl_download writes only the first n entries of every array (an entry of Q or of the ancestors that the last update did
 * not write, beyond its n_before or after visfs_mcl_kld_upload, is that of the last update or init that wrote it).
 * visfs_mcl_result's n_eff, mean and covariance are those of the n_before particles. */
int  visfs_mcl_kld_enable(visfs_mcl* f, const visfs_mcl_kld_params* p);
/* The last update's counts (BAD_ARGUMENT, and zeros, before any update of the KLD filter, or when `f` is no KLD filter). */
int  visfs_mcl_kld_last(const visfs_mcl* f, visfs_mcl_kld_result* r);
/* The active count n (N on a filter that is no KLD filter; 0 for a null filter). */
int32_t visfs_mcl_kld_count(const visfs_mcl* f);
/* visfs_mcl_upload with a count: replaces the particles by x, y, yaw, w [n], 1 <= n <= N, and sets the active count to n.
 * BAD_ARGUMENT as visfs_mcl_upload, for n outside 1 .. N and on a filter that is no KLD filter. */
int  visfs_mcl_kld_upload(visfs_mcl* f, int32_t n, const double* x, const double* y, const double* yaw, const double* w);

/* ---- hooks --------------------------------------------------------------------------------------------------------------------- */
/* The table as the filter holds it (on the device: what the device holds), limit [N + 1]. */
int  visfs_mcl_kld_limits(visfs_mcl* f, int32_t* limit);
/* How many bits of a bin's hash choose the home slot of a draw in the device's table: 0 sends every draw to slot 0 (the longest
 * probe chains), -1 (the default) and everything above the table's width mean the full width.  The results do not depend on it. */
int  visfs_mcl_kld_hook_set_hash_bits(visfs_mcl* f, int32_t bits);
/* The bin index of section 9u as the filter forms it: bins[i] = floor(v[i] / size) clamped to [-2^24, 2^24]; finite v, size
 * finite and positive. */
int  visfs_mcl_kld_hook_bins(int32_t n, const double* v, double size, int32_t* bins);

#ifdef __cplusplus
}
#endif
#endif
