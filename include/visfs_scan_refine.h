/*
 * visfs_scan_refine.h — sub-cell refinement of a scan's pose on a probability grid (implemented in libvisfs_ba_hip.so).
 *
 * The matchers (visfs_scan_match.h, visfs_scan_fast.h, visfs_scan_group.h) return a pose on their search lattice: whole cells and
 * whole angular steps from the guess.  The refinement here is the continuous step that follows a correlative match in the pipeline
 * they restate (Cartographer's Ceres scan matcher): the occupied-space cost of the returns, interpolated bicubically on the same
 * grid, plus a pull towards a target translation and the initial yaw, minimised over (x, y, yaw) by Levenberg-Marquardt.  One
 * workgroup of VISFS_SCAN_REFINE_LANES work items refines one pose inside one launch; a one-core host twin serves host sub-maps
 * and host stacks; both give the same bytes.  DESIGN.md section 9o states the cost, the control and the reduction order.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_SCAN_REFINE_H
#define VISFS_SCAN_REFINE_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_submap.h"
#include "visfs_scan_fast.h"
#include "visfs_scan_group.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_SCAN_REFINE_ABI_VERSION 1

#define VISFS_SCAN_REFINE_LANES 256                 /* the workgroup size; part of the definition: the sums are formed per lane */
#define VISFS_SCAN_REFINE_MAX_POINTS 16384          /* n (beyond: VISFS_BA_ERR_UNSUPPORTED) */
#define VISFS_SCAN_REFINE_MAX_ITERATIONS 50         /* max_iterations outside [1, 50]: VISFS_BA_ERR_BAD_ARGUMENT */
#define VISFS_SCAN_REFINE_MAX_TRIALS 500            /* 10 trials per iteration at most */
#define VISFS_SCAN_REFINE_MAX_ROTATION 1.0          /* |yaw - initial yaw| a trial may reach, radians */

/* termination */
#define VISFS_SCAN_REFINE_ITERATIONS 0              /* max_iterations outer iterations ran */
#define VISFS_SCAN_REFINE_NO_PROGRESS 1             /* ten trials rejected in a row, or a trial that changed nothing (rho == 0) */
#define VISFS_SCAN_REFINE_TOLERANCE 2               /* an accepted step lowered the cost by function_tolerance of it or less */

typedef struct visfs_scan_refine_params {
    double  occupied_space_weight;         /* default 1   (Cartographer's ceres_scan_matcher defaults) */
    double  translation_weight;            /* default 10  */
    double  rotation_weight;               /* default 40  */
    double  function_tolerance;            /* default 1e-6; 0: no such test */
    int32_t max_iterations;                /* default 20, 1 .. 50 */
} visfs_scan_refine_params;

typedef struct visfs_scan_refine_result {
    int32_t status;                        /* VISFS_BA_OK; in a group, VISFS_BA_ERR_UNSUPPORTED for a member whose match overflowed */
    int32_t refined;                       /* 0: nothing was refined (n == 0, no sub-map yet, a skipped member): the start back */
    int32_t iterations, trials;            /* outer iterations run, trials evaluated (accepted and rejected) */
    int32_t termination;                   /* VISFS_SCAN_REFINE_ITERATIONS / _NO_PROGRESS / _TOLERANCE */
    int32_t reserved;                      /* 0 */
    double  x, y, yaw;                     /* the refined pose */
    double  initial_cost, final_cost;      /* the sum of squared residuals at the start and at the returned pose */
    double  information[9];                /* J^T J over all residuals at the returned pose (no damping), row-major, (x, y, yaw) */
} visfs_scan_refine_result;

int  visfs_scan_refine_abi_version(void);
void visfs_scan_refine_default_params(visfs_scan_refine_params* p);

/* The returns (robot frame, [n][3], z ignored) refined against sub-map `index` of `s` (device or host flavour) from the pose
 * initial_xy_yaw towards the translation target_xy.  The grid is read on the sub-maps' stream as it is after every insertion made
 * so far; nothing in `s` changes.  n == 0, or no sub-map yet: refined = 0 and the start back.  n > 16384:
 * VISFS_BA_ERR_UNSUPPORTED.  A non-finite pose, target, point or parameter, a negative weight or tolerance, max_iterations outside
 * 1 .. 50, or an index that names no active sub-map while there is one: VISFS_BA_ERR_BAD_ARGUMENT.  An error launches nothing and
 * leaves the hook data of the last call.  The reason is in visfs_submaps_last_error(s). */
int  visfs_scan_refine(visfs_submaps* s, int32_t index, const visfs_scan_refine_params* p, const double initial_xy_yaw[3],
                       const double target_xy[2], int32_t n, const double* points_xyz, visfs_scan_refine_result* out);

/* The same against level 0 of a frozen stack (the reason of an error in visfs_scan_stack_last_error(st)). */
int  visfs_scan_stack_refine(visfs_scan_stack* st, const visfs_scan_refine_params* p, const double initial_xy_yaw[3],
                             const double target_xy[2], int32_t n, const double* points_xyz, visfs_scan_refine_result* out);

/* visfs_scan_group_match, then in the same call the refinement of every member with status OK and matched = 1, from its winner
 * towards its guess's translation: results, status and best_member are byte for byte visfs_scan_group_match's, and refined[i] is
 * byte for byte what visfs_scan_stack_refine(members[i], rp, winner of i, guess of i, ...) returns.  An unmatched member gets
 * refined = 0 with its winner as the pose; an overflowed member gets status VISFS_BA_ERR_UNSUPPORTED and refined = 0.  On the
 * device the call is the match's sequence plus one launch (the member as blockIdx.x); the winner is read where the match left
 * it, the records come with the match's one download.  The argument checks of both calls run before anything is pushed. */
int  visfs_scan_group_match_refine(visfs_scan_group* g, const visfs_scan_stack_params* mp, const visfs_scan_refine_params* rp,
                                   const double* guesses /*[m][3]*/, int32_t n, const double* points_xyz,
                                   visfs_scan_stack_result* results /*[m]*/, int32_t* status /*[m]*/, int32_t* best_member,
                                   visfs_scan_refine_result* refined /*[m]*/);

/* ---- hooks (tests) ----------------------------------------------------------------------------------------------------------- */
/* The trace of the last successful refinement on `s` / `st` / member `member` of the last visfs_scan_group_match_refine that ran to
 * its end: *trials, and per trial (cost of the trial pose, lambda of the trial, 1 if accepted else 0, x, y, yaw - initial yaw), in
 * order; `cap` is the capacity of `trace` in trials.  A trial whose step could not be formed or left the rotation bound has the
 * cost DBL_MAX.  *trials = 0 after a call that refined nothing, and before any call.  `trace` may be NULL. */
int  visfs_scan_refine_download(visfs_submaps* s, int32_t cap, double* trace /*[cap][6]*/, int32_t* trials);
int  visfs_scan_stack_refine_download(visfs_scan_stack* st, int32_t cap, double* trace, int32_t* trials);
int  visfs_scan_group_refine_download(visfs_scan_group* g, int32_t member, int32_t cap, double* trace, int32_t* trials);

#ifdef __cplusplus
}
#endif
#endif
