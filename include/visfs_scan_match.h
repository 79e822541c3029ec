/*
 * visfs_scan_match.h — correlative scan matching on the laser sub-maps (implemented in libvisfs_ba_hip.so).
 *
 * The step Estimator::laserPretreatment names and leaves empty ("Correlative scan match."): an exhaustive search over (x, y, yaw)
 * about a pose guess for the pose at which a scan's returns fall on the most probable cells of a sub-map's probability grid
 * (Cartographer's real-time correlative scan matcher), in front of the occupied-space refinement the sliding-window BA already runs.
 * On device sub-maps the search runs as HIP kernels on the sub-maps' stream and reads the grid where it lives; on host sub-maps
 * (visfs_submaps_create_host) the same search runs on one core, and both give the same bits.  DESIGN.md section 9l states the
 * semantics.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_SCAN_MATCH_H
#define VISFS_SCAN_MATCH_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_SCAN_MATCH_ABI_VERSION 1

/* limits of one call (beyond them: VISFS_BA_ERR_UNSUPPORTED) */
#define VISFS_SCAN_MATCH_MAX_POINTS 16384       /* n */
#define VISFS_SCAN_MATCH_MAX_LINEAR 32          /* nl */
#define VISFS_SCAN_MATCH_MAX_SCANS 1025         /* S */
#define VISFS_SCAN_MATCH_MAX_CANDIDATES 2097152 /* S * L * L, L = 2 nl + 1 */

typedef struct visfs_scan_match_params {
    double linear_search_window;           /* metres,  default 0.1            (Cartographer's defaults) */
    double angular_search_window;          /* radians, default 20 degrees                                 */
    double translation_delta_cost_weight;  /* default 0.1 */
    double rotation_delta_cost_weight;     /* default 0.1 */
} visfs_scan_match_params;

typedef struct visfs_scan_match_result {
    int32_t matched;             /* 0: no sub-map yet, or n == 0: pose = the guess, score = 0, everything else 0 */
    double  x, y, yaw;           /* the corrected pose: guess + winner */
    double  score;               /* the winner's weighted score */
    int64_t sum;                 /* the winner's integer sum Q */
    int32_t scan_index, x_offset, y_offset;    /* the winner, in cell-index space: k in [0, S), xo and yo in [-nl, nl] */
    int32_t num_scans, num_linear;             /* S = 2 na + 1, nl */
    double  angular_step;
} visfs_scan_match_result;

int  visfs_scan_match_abi_version(void);
void visfs_scan_match_default_params(visfs_scan_match_params* p);

/* The returns (robot frame, [n][3], z ignored) against sub-map `index` (0 = front = the matching sub-map) of `s`, device or host
 * flavour alike, about the guess (x, y, yaw) in the map frame.  The sub-maps are read as they are after every insertion made so
 * far and are not changed.  1 <= n <= 16384 (n == 0, or no sub-map yet: matched = 0); nl <= 32, S <= 1025, S * L * L <= 2^21:
 * beyond them VISFS_BA_ERR_UNSUPPORTED.  A non-finite guess, point, window or weight, a negative window, or an index that names no
 * active sub-map while there is one: VISFS_BA_ERR_BAD_ARGUMENT.  An error launches nothing and leaves the last call's candidates. */
int  visfs_scan_match(visfs_submaps* s, int32_t index, const visfs_scan_match_params* p, const double guess_xy_yaw[3],
                      int32_t n, const double* points_xyz, visfs_scan_match_result* out);

/* Hook (tests): every candidate of the last successful call on `s`: the integer sums and the scores, [S][L][L] in generation order
 * (scan k outermost, then xo, then yo), and the discretised cells [S][n][2] (x index, y index) before any offset.  Any pointer may be
 * NULL.  `cap` is the capacity of each array given, in its own items (candidates; cells): S * L * L for sums and scores, S * n for
 * cells_xy.  After a call that ended with matched = 0 there is nothing to write. */
int  visfs_scan_match_download(visfs_submaps* s, int64_t cap, int32_t* sums, double* scores, int32_t* cells_xy);

/* Estimator::laserPretreatment (Estimator.cpp:116-157), host only: the scan split into Estimator/NumSubdivisionsPerScan parts
 * (empty parts skipped), origin and points taken from the laser to the camera (robot) frame, returns below min_range dropped,
 * returns beyond max_range turned into misses at missing_ray_length along their ray.  The per-point times the reference re-bases
 * are read by nothing downstream and are not carried. */
typedef struct visfs_scan_pretreat_params {
    int32_t num_subdivisions;    /* numSubdivisionsPerScan_ (>= 1) */
    double  min_range;           /* Estimator/MinLaserRange         (default 0.1)  */
    double  max_range;           /* Estimator/MaxLaserRange         (default 30)   */
    double  missing_ray_length;  /* Estimator/MissingDataRayLength  (default 5)    */
} visfs_scan_pretreat_params;

void visfs_scan_pretreat_default_params(visfs_scan_pretreat_params* p);
/* points_xyz [n][3] and origin in the laser frame, T_laser_to_camera 3x4 row-major.  rd_out has room for p->num_subdivisions
 * entries; *n_out of them are filled, in order, their `returns` / `misses` pointing into returns_out / misses_out (room for
 * [n][3] each), which must outlive them.  n == 0: *n_out = 0. */
int  visfs_scan_pretreat(const visfs_scan_pretreat_params* p, const double T_laser_to_camera[12], const double origin[3],
                         int32_t n, const double* points_xyz, double* returns_out, double* misses_out,
                         visfs_range_data* rd_out, int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif
