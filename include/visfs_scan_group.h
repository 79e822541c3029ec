/*
 * visfs_scan_group.h — one scan matched against many frozen sub-map grid stacks in one call (implemented in libvisfs_ba_hip.so).
 *
 * visfs_scan_stack_match (visfs_scan_fast.h) searches one frozen sub-map.  A robot that comes back to a place does not know which
 * sub-map it is in: its scan has to be matched against every finished sub-map near the guess.  A visfs_scan_group holds a set of
 * visfs_scan_stacks and matches one scan against all of them in one call: on the device every kernel of the single call's sequence
 * runs once with the member as a grid dimension, so the launches (H + 5), the upload, the download and the stream wait do not grow
 * with the number of members.  Each member's record is byte for byte what visfs_scan_stack_match gives on that member: the members
 * share nothing but the scan (no common incumbent).  A group of host-twin stacks runs the one-core twin per member.  DESIGN.md
 * section 9n states the semantics.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_SCAN_GROUP_H
#define VISFS_SCAN_GROUP_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_scan_fast.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_SCAN_GROUP_ABI_VERSION 1

#define VISFS_SCAN_GROUP_MAX 64                     /* members of a group (m outside [1, 64]: VISFS_BA_ERR_UNSUPPORTED) */
#define VISFS_SCAN_GROUP_MAX_FRONTIER 67108864      /* m * frontier_capacity of one call (beyond: VISFS_BA_ERR_UNSUPPORTED) */

typedef struct visfs_scan_group visfs_scan_group;

int  visfs_scan_group_abi_version(void);

/* members[m]: all device stacks of one handle, or all host-twin stacks; all with bitwise equal resolution and equal depth (a scan
 * then has the same angular step, S, nl, L, H and top nodes per scan on every member).  Grid sizes and limits may differ.  The same
 * stack may appear more than once, and a stack may be in several groups: the group only reads its levels.  The members must outlive
 * the group.  VISFS_BA_ERR_UNSUPPORTED: m outside 1 .. 64.  VISFS_BA_ERR_BAD_ARGUMENT: a NULL member, device and host members
 * mixed, members of different handles, unequal resolution or depth.  visfs_scan_group_last_error(NULL) gives the reason of the
 * calling thread's last failed create; it names the member index. */
int  visfs_scan_group_create(int32_t m, visfs_scan_stack* const* members, visfs_scan_group** out);
void visfs_scan_group_destroy(visfs_scan_group* g);                       /* the members live on */
const char* visfs_scan_group_last_error(const visfs_scan_group* g);

/* The returns (robot frame, [n][3], z ignored) against every member: results[i] is byte for byte what
 * visfs_scan_stack_match(members[i], p, guesses + 3 i, n, points_xyz, &results[i]) returns.  One scan and one set of params; every
 * member has its own guess (x, y, yaw).  Every argument and limit check of the single call runs for every member before anything is
 * pushed; a failed check returns the single call's code, names the member and changes nothing.  frontier_capacity applies per
 * member; m * frontier_capacity > 2^26: VISFS_BA_ERR_UNSUPPORTED.
 * status[i] is VISFS_BA_OK, or VISFS_BA_ERR_UNSUPPORTED when member i's frontier overflowed: the call still returns VISFS_BA_OK,
 * results[i] is left untouched and last_error says "member i: frontier overflow at level h: ..." (the lowest such member).
 * best_member: the member with status OK and matched = 1 of the largest integer sum (n is common, so the score is monotone in the
 * sum), among equal sums the lowest index; -1 when there is none.  n == 0: every guess back with matched = 0, best_member = -1.
 * A device error returns VISFS_BA_ERR_DEVICE and leaves the hook data of the previous call.  The members' own hook data
 * (visfs_scan_stack_match_download) are not touched; single calls on a member between group calls are allowed. */
int  visfs_scan_group_match(visfs_scan_group* g, const visfs_scan_stack_params* p, const double* guesses /*[m][3]*/, int32_t n,
                            const double* points_xyz, visfs_scan_stack_result* results /*[m]*/, int32_t* status /*[m]*/,
                            int32_t* best_member);

/* ---- hooks (tests) ----------------------------------------------------------------------------------------------------------- */
/* Member `member` of the last group call that ran to its end (n > 0), in the layout and sort order of
 * visfs_scan_stack_match_download.  A member whose status was not OK, and every member before any such call, gets an all-zero
 * header. */
int  visfs_scan_group_match_download(visfs_scan_group* g, int32_t member, int32_t header[8], int32_t scored[16], int32_t kept[16],
                                     int64_t bounds_cap, int32_t* bounds, int64_t survivors_cap, int32_t* survivors);
/* What the last match call issued, counted by the library where it issues them; all zero for a host group.  Any pointer may be
 * NULL. */
int  visfs_scan_group_last_counts(const visfs_scan_group* g, int32_t* kernel_launches, int32_t* copies_and_memsets,
                                  int32_t* synchronisations);

#ifdef __cplusplus
}
#endif
#endif
