/*
 * visfs_tracker_group.h — a rig of resident trackers processed by one call (in libvisfs_ba_hip.so).
 *
 * visfs_tracker_process (visfs_tracker.h) runs one stereo pair per call; its launches are far too small for the device, and the
 * trackers of one handle share that handle's stream, so n cameras cost n calls one behind the other.  A tracker group takes the
 * frames of n trackers in one call: every kernel of the frame sequence runs once with a member dimension, one upload carries the
 * per-call table, the outlier ids and the guesses of all members, one synchronisation ends the call.  The number of kernel launches
 * does not depend on n.  Each member's result is byte for byte what visfs_tracker_process gives for it alone, and single calls on a
 * member between group calls are allowed.  DESIGN.md section 9i has the table layout, the launch list and the measurement.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_TRACKER_GROUP_H
#define VISFS_TRACKER_GROUP_H

#include <stdint.h>
#include "visfs_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_TRACKER_GROUP_ABI_VERSION 1
#define VISFS_TRACKER_GROUP_MAX 64

typedef struct visfs_tracker_group visfs_tracker_group;

typedef struct visfs_tracker_frame {          /* the arguments of visfs_tracker_process for one member */
    const uint8_t*  left;
    const uint8_t*  right;
    int32_t         stride;
    const double*   delta_guess;              /* 3x4 or NULL */
    int32_t         n_outliers;
    const uint64_t* outlier_ids;
} visfs_tracker_frame;

int  visfs_tracker_group_abi_version(void);

/* members[n]: all device trackers of one handle, or all trackers of host-twin flow objects; each on a flow object of its own; all with
 * the same image size, field-wise equal visfs_flow_params and field-wise equal visfs_tracker_params.  Cameras may differ.  A tracker
 * is in at most one group.  The members must outlive the group or be destroyed before its next call, which then fails.
 * VISFS_BA_ERR_UNSUPPORTED: n outside 1 .. 64.  VISFS_BA_ERR_BAD_ARGUMENT: everything else; visfs_tracker_last_error of the
 * offending member names its index. */
int  visfs_tracker_group_create(int32_t n, visfs_tracker* const* members, visfs_tracker_group** out);
void visfs_tracker_group_destroy(visfs_tracker_group* g);                 /* the members live on */
const char* visfs_tracker_group_last_error(const visfs_tracker_group* g);

/* Equals visfs_tracker_process(members[i], frames[i]..., &results[i]) for i = 0 .. n - 1.  Every argument check of that call runs for
 * every member before anything is pushed: a failure changes no member and names the member in the error string.  The result arrays
 * belong to the member and stay valid until that member's next call, single or grouped.
 * VISFS_BA_ERR_NOT_LOADED: a member or its flow object has been destroyed, or a member's images were pushed by somebody else. */
int  visfs_tracker_group_process(visfs_tracker_group* g, const visfs_tracker_frame* frames /*[n]*/,
                                 visfs_tracker_result* results /*[n]*/);

/* What the last process call issued, counted by the library where it issues them; all zero for a host group.  Any pointer may be
 * NULL. */
int  visfs_tracker_group_last_counts(const visfs_tracker_group* g, int32_t* kernel_launches, int32_t* copies_and_memsets,
                                     int32_t* synchronisations);

#ifdef __cplusplus
}
#endif
#endif
