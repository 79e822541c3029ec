/*
 * visfs_scan_filter.h — the laser pretreatment with its voxel filters, for batches of scans (implemented in libvisfs_ba_hip.so).
 *
 * Estimator::laserPretreatment names three steps: "Transform to gravity aligned.", "Filter.", "Correlative scan match.".  This is
 * the second one, together with the split and the range classification that visfs_scan_pretreat (visfs_scan_match.h) does on the
 * host: one call takes up to 64 raw scans in the laser frame and gives, per scan, the visfs_range_data that visfs_submaps_insert
 * takes (returns and misses of every subdivision, each thinned by a fixed voxel filter) and the match cloud that visfs_scan_match,
 * visfs_scan_stack_match, visfs_scan_group_match and their refine forms take (the filtered returns within a range, thinned by the
 * adaptive voxel filter of Cartographer 1.0).  An object made on a handle runs one HIP kernel per call on that handle's device and
 * stream, one workgroup per scan; an object made with h == NULL is the one-core host twin; both give the same bytes.  DESIGN.md
 * section 9s states the semantics.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.  Every refusal is decided on the host before anything is pushed, and leaves the
 * last call's results and counts in place.
 */
#ifndef VISFS_SCAN_FILTER_H
#define VISFS_SCAN_FILTER_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_submap.h"
#include "visfs_scan_match.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_SCAN_FILTER_ABI_VERSION 1

#define VISFS_SCAN_FILTER_MAX_SCANS 64
#define VISFS_SCAN_FILTER_MAX_POINTS 16384        /* n of one scan (VISFS_SCAN_MATCH_MAX_POINTS) */
#define VISFS_SCAN_FILTER_MAX_SUBDIVISIONS 16
#define VISFS_SCAN_FILTER_MAX_TRACE 16
#define VISFS_SCAN_FILTER_MAX_VOXEL 1048575       /* |round(p / length)| per axis: 2^20 - 1 */

/* hook classes of an input point */
#define VISFS_SCAN_FILTER_DROPPED 0
#define VISFS_SCAN_FILTER_RETURN 1
#define VISFS_SCAN_FILTER_MISS 2

typedef struct visfs_scan_filter_params {
    visfs_scan_pretreat_params pretreat;   /* 1 <= num_subdivisions <= 16 */
    double  voxel_size;                    /* the fixed filter over returns and misses; default 0.025; 0: off */
    double  adaptive_max_length;           /* the adaptive filter over the match cloud; default 0.5; 0: off */
    int32_t adaptive_min_num_points;       /* default 200 */
    double  adaptive_max_range;            /* default 50: filtered returns with |p| (robot frame) beyond it leave the match cloud */
} visfs_scan_filter_params;

/* One raw scan in the laser frame. */
typedef struct visfs_scan_filter_scan {
    double T_laser_to_camera[12];          /* 3x4 row-major */
    double origin[3];
    int32_t n;                             /* 0 .. 16384 */
    const double* points_xyz;              /* [n][3] */
} visfs_scan_filter_scan;

typedef struct visfs_scan_filter_record {
    int32_t status;                        /* VISFS_BA_OK, or VISFS_BA_ERR_UNSUPPORTED: a voxel index beyond +-(2^20 - 1); everything below 0 then */
    int32_t n_range_data;                  /* non-empty subdivisions */
    int32_t n_returns, n_misses;           /* over all subdivisions, after the fixed filter */
    int32_t n_in_range;                    /* filtered returns within adaptive_max_range */
    int32_t n_match;                       /* points of the match cloud */
    int32_t passes;                        /* voxel-filter passes of the adaptive search (0 .. 12) */
    int32_t reserved;
    double  match_length;                  /* the voxel length the match cloud was filtered at; 0: unfiltered */
} visfs_scan_filter_record;

typedef struct visfs_scan_filter visfs_scan_filter;

int  visfs_scan_filter_abi_version(void);
void visfs_scan_filter_default_params(visfs_scan_filter_params* p);

/* A filter on the device and stream of handle `h`; h == NULL: the one-core host twin. */
int  visfs_scan_filter_create(visfs_ba_handle* h, visfs_scan_filter** out);
void visfs_scan_filter_destroy(visfs_scan_filter* f);
const char* visfs_scan_filter_last_error(const visfs_scan_filter* f);

/* Pretreats and filters scans[0 .. m).  records ([m]) may be NULL.  m == 0: VISFS_BA_OK, nothing launched, no results.
 * VISFS_BA_ERR_BAD_ARGUMENT: a non-finite point, transform or origin; a negative or non-finite voxel_size, adaptive_max_length or
 * adaptive_max_range; adaptive_min_num_points < 0; num_subdivisions < 1; n < 0.  VISFS_BA_ERR_UNSUPPORTED: m > 64, n > 16384,
 * num_subdivisions > 16.  On the device: one upload, one launch, one download, one wait, whatever m and the sizes are. */
int  visfs_scan_filter_process(visfs_scan_filter* f, const visfs_scan_filter_params* p, int32_t m, const visfs_scan_filter_scan* scans,
                               visfs_scan_filter_record* records);

/* Scans of the last successful call. */
int  visfs_scan_filter_num_scans(const visfs_scan_filter* f, int32_t* m);
int  visfs_scan_filter_record_of(const visfs_scan_filter* f, int32_t scan, visfs_scan_filter_record* record);
/* The range data of scan `scan` of the last successful call, in order of the subdivisions: *n_out entries, written up to `cap` of
 * them (rd_out may be NULL when cap == 0).  Their pointers lie in the object's download block: valid until the next successful
 * visfs_scan_filter_process or the object's destruction. */
int  visfs_scan_filter_range_data(const visfs_scan_filter* f, int32_t scan, int32_t cap, visfs_range_data* rd_out, int32_t* n_out);
/* The match cloud [n][3] of scan `scan`, valid as long as the range data (*xyz is NULL when *n is 0). */
int  visfs_scan_filter_match_cloud(const visfs_scan_filter* f, int32_t scan, const double** xyz, int32_t* n);

/* ---- hooks (tests) ------------------------------------------------------------------------------------------------------------- */
/* Per input point of scan `scan` ([n] each, any may be NULL): its class (VISFS_SCAN_FILTER_DROPPED / RETURN / MISS), the
 * subdivision it fell into (0 .. num_subdivisions - 1) and whether the fixed filter kept it (a dropped point: 0); and the adaptive
 * search's trace: *n_trace = passes pairs (length, count) in the order they were tried (room for 16 each).  A scan whose status is
 * not VISFS_BA_OK gives zeros. */
int  visfs_scan_filter_download(const visfs_scan_filter* f, int32_t scan, uint8_t* point_class, uint8_t* subdivision, uint8_t* kept,
                                double* trace_length, int32_t* trace_count, int32_t* n_trace);
/* The slots of the open-addressed table one voxel-filter pass over `count` points uses, and the slot a voxel of list `list`
 * (fixed filter: 2 * subdivision + (class == MISS); adaptive passes: 0) hashes to before probing.  Host only. */
int  visfs_scan_filter_hook_slot(const int32_t voxel[3], int32_t list, int32_t count, int32_t* slots, int32_t* slot);
/* What the last successful call issued on the device (all zero on the twin and before any call). */
int  visfs_scan_filter_last_counts(const visfs_scan_filter* f, int32_t* launches, int32_t* copies, int32_t* waits);

#ifdef __cplusplus
}
#endif
#endif
