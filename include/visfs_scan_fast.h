/*
 * visfs_scan_fast.h — branch-and-bound scan matching over frozen sub-map grid stacks (implemented in libvisfs_ba_hip.so).
 *
 * visfs_scan_match (visfs_scan_match.h) scores every candidate about a good guess and reads a sub-map that keeps changing.  A
 * visfs_scan_stack is an immutable snapshot of one probability grid with its precomputed window-maximum levels (Cartographer's
 * fast correlative scan matcher), and visfs_scan_stack_match searches it by branch and bound: relocalisation from a guess that is
 * metres and tens of degrees off, and loop closure against a finished sub-map that must not move under the search.  The score is
 * the exact integer sum of visfs_scan_match without delta-cost weights, so the result is defined without reference to the
 * pruning: the leaf of maximal sum, earliest in generation order.  A stack made on a device handle or on device sub-maps lives in
 * device memory and is searched by HIP kernels; a stack made on host sub-maps (or with h == NULL) is searched by the one-core
 * twin; both give the same bits.  DESIGN.md section 9m states the semantics.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_SCAN_FAST_H
#define VISFS_SCAN_FAST_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_submap.h"
#include "visfs_scan_match.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_SCAN_FAST_ABI_VERSION 1

/* limits of a stack and of one call (beyond them: VISFS_BA_ERR_UNSUPPORTED) */
#define VISFS_SCAN_FAST_MAX_DEPTH 16                /* levels of a stack (depth outside [1, 16]: VISFS_BA_ERR_BAD_ARGUMENT) */
#define VISFS_SCAN_FAST_MAX_BYTES 1073741824        /* all levels of a stack together: 1 GiB */
#define VISFS_SCAN_FAST_MAX_POINTS 16384            /* n */
#define VISFS_SCAN_FAST_MAX_LINEAR 512              /* nl */
#define VISFS_SCAN_FAST_MAX_SCANS 1025              /* S */
#define VISFS_SCAN_FAST_MAX_CELLS 4194304           /* S * n */
#define VISFS_SCAN_FAST_MAX_TOP_NODES 4194304       /* S * ceil(L / 2^H)^2: the nodes of the top level, all of which are scored */
#define VISFS_SCAN_FAST_MAX_FRONTIER 67108864       /* frontier_capacity (outside [4, 2^26]: VISFS_BA_ERR_BAD_ARGUMENT) */

typedef struct visfs_scan_stack visfs_scan_stack;

typedef struct visfs_scan_stack_info {
    double  resolution, max_x, max_y;      /* the limits frozen with the grid */
    int32_t num_x_cells, num_y_cells;
    int32_t depth;                         /* levels 0 .. depth - 1 */
    int32_t device;                        /* 1: device memory and kernels; 0: the host twin */
    int64_t bytes;                         /* all levels together */
} visfs_scan_stack_info;

typedef struct visfs_scan_stack_params {
    double  linear_search_window;          /* metres,  default 7    (Cartographer's constraint-builder defaults) */
    double  angular_search_window;         /* radians, default 30 degrees                                       */
    double  min_score;                     /* default 0: a winner below it gives matched = 0 */
    int32_t frontier_capacity;             /* default 2^20: the nodes kept at one level, at most */
} visfs_scan_stack_params;

typedef struct visfs_scan_stack_result {
    visfs_scan_match_result match;         /* as visfs_scan_match fills it; score = candidate score with weight 1 */
    int32_t depth_used;                    /* H + 1: the levels the search descended through */
} visfs_scan_stack_result;

int  visfs_scan_fast_abi_version(void);
void visfs_scan_stack_default_params(visfs_scan_stack_params* p);

/* Sub-map `index` of `s` as it is after every insertion made so far, frozen with `depth` levels.  Device sub-maps give a device
 * stack, built on the sub-maps' stream from the grid where it lives; host sub-maps give the host twin.  Later insertions,
 * finishing and cropping, or destroying `s` do not change the stack (a device stack needs the handle `s` was created on to outlive
 * it).  An error is reported through visfs_submaps_last_error(s). */
int  visfs_scan_stack_create(visfs_submaps* s, int32_t index, int32_t depth, visfs_scan_stack** out);
/* The same from cells [num_y_cells][num_x_cells] and limits as visfs_submaps_download and visfs_submaps_describe hand them out
 * (resolution, max_x, max_y, num_x_cells, num_y_cells are read).  h == NULL: the host twin. */
int  visfs_scan_stack_create_from_grid(visfs_ba_handle* h, const visfs_submap_info* limits, const uint16_t* cells, int32_t depth,
                                       visfs_scan_stack** out);
void visfs_scan_stack_destroy(visfs_scan_stack* st);
const char* visfs_scan_stack_last_error(const visfs_scan_stack* st);
int  visfs_scan_stack_describe(const visfs_scan_stack* st, visfs_scan_stack_info* info);

/* The returns (robot frame, [n][3], z ignored) against the stack about the guess (x, y, yaw): rotations and cells as
 * visfs_scan_match forms them, every offset xo, yo in [-nl, nl], no delta-cost weights.  The winner is the leaf of maximal integer
 * sum and, among equal sums, of the smallest generation-order index (k * L + xo + nl) * L + yo + nl.  matched = 0 when the winner's
 * score is below min_score (fields still filled) and for n == 0 (the guess back).  nl <= 512, S <= 1025, n <= 16384,
 * S * n <= 2^22, S * ceil(L / 2^H)^2 <= 2^22 with H = min(depth - 1, smallest h with 2^h >= L): beyond them, and when the nodes
 * kept at one level exceed frontier_capacity ("frontier overflow", with the level, in last_error), VISFS_BA_ERR_UNSUPPORTED.  An
 * error leaves the hook data of the last successful call. */
int  visfs_scan_stack_match(visfs_scan_stack* st, const visfs_scan_stack_params* p, const double guess_xy_yaw[3], int32_t n,
                            const double* points_xyz, visfs_scan_stack_result* out);

/* ---- hooks (tests) ----------------------------------------------------------------------------------------------------------- */
/* Level h as stored: dims = (width, height, low-side extension e = 2^h - 1, 0); the array [height][width] holds x in [-e, nx) and
 * y in [-e, ny).  `out` may be NULL (dims only); otherwise `cap` >= width * height items. */
int  visfs_scan_stack_download_level(visfs_scan_stack* st, int32_t h, int64_t cap, uint16_t* out, int32_t dims[4]);
/* The last successful match: header = (S, L, n, H, top nodes per scan, survivors, B, 0); per level h in [0, 16) the nodes scored
 * by the sweep and the nodes kept (U >= B); the top level's bounds [S][ceil(L / 2^H)^2]; the level-0 survivors (index, Q) sorted
 * by index.  Any pointer but `header` may be NULL; bounds_cap and survivors_cap are the capacities of those arrays in items
 * (survivors: pairs).  After no successful match the header is all zero. */
int  visfs_scan_stack_match_download(visfs_scan_stack* st, int32_t header[8], int32_t scored[16], int32_t kept[16],
                                     int64_t bounds_cap, int32_t* bounds, int64_t survivors_cap, int32_t* survivors);

#ifdef __cplusplus
}
#endif
#endif
