/*
 * visfs_submap.h — laser sub-maps resident on the GPU (implemented in libvisfs_ba_hip.so).
 *
 * The reference's ActiveSubmaps2D of probability grids (Map/2d/Submap2D.cpp, ProbabilityGridRangeDataInserter2D.cpp,
 * RayToPixelMask.cpp): at most two sub-maps, both receiving every range data; the front one is the "matching" sub-map the laser
 * occupied-space factor of the sliding-window BA reads.  The grids live in device memory; insertions run as HIP kernels on the stream
 * of the handle the sub-maps were created on; visfs_submaps_solve_window hands the matching grid to the BA without it crossing to the
 * host.  DESIGN.md section 9b states the semantics (and the two quirks of the reference that are reproduced).
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_SUBMAP_H
#define VISFS_SUBMAP_H

#include <stdint.h>
#include "visfs_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_SUBMAP_ABI_VERSION 1

/* The LocalMap keys (Parameters.h:164-169). */
typedef struct visfs_submap_params {
    int32_t num_range_data_limit;  /* LocalMap/NumRangeDataLimit  (default 50) */
    int32_t grid_map_type;         /* LocalMap/GridMapType        (default 0 = probability grid; 1 = TSDF: VISFS_BA_ERR_UNSUPPORTED) */
    double  map_resolution;        /* LocalMap/MapResolution      (default 0.05) */
    int32_t insert_free_space;     /* LocalMap/InsertFreeSpace    (default 1; read but without effect, as in the reference) */
    double  hit_probability;       /* LocalMap/HitProbability     (default 0.55) */
    double  miss_probability;      /* LocalMap/MissProbability    (default 0.49) */
} visfs_submap_params;

/* One Sensor::RangeData in the robot frame (as Estimator::laserPretreatment leaves it). */
typedef struct visfs_range_data {
    double origin[3];
    int32_t n_returns;
    const double* returns;         /* [n_returns][3] */
    int32_t n_misses;
    const double* misses;          /* [n_misses][3] */
} visfs_range_data;

/* What visfs_submaps_describe reports of one sub-map (index 0 = front = the matching sub-map). */
typedef struct visfs_submap_info {
    int32_t num_range_data;        /* Submap::getNumRangeData() */
    int32_t finished;              /* Submap::getInsertionStatus(): finished (cropped) */
    double  resolution;            /* limits() */
    double  max_x, max_y;
    int32_t num_x_cells, num_y_cells;
    int32_t known_min_x, known_min_y, known_max_x, known_max_y;   /* knownCellsBox_ (empty: min > max) */
} visfs_submap_info;

typedef struct visfs_submaps visfs_submaps;

int  visfs_submap_abi_version(void);
void visfs_submap_default_params(visfs_submap_params* p);

/* Sub-maps on the device and stream of handle `h`.  VISFS_BA_ERR_UNSUPPORTED for grid_map_type 1 (TSDF). */
int  visfs_submaps_create(visfs_ba_handle* h, const visfs_submap_params* p, visfs_submaps** out);
/* The host restatement of the same sub-maps (one core, no device): the reference's sequential insertion, for parity tests. */
int  visfs_submaps_create_host(const visfs_submap_params* p, visfs_submaps** out);
void visfs_submaps_destroy(visfs_submaps* s);
const char* visfs_submaps_last_error(const visfs_submaps* s);

/* LocalMap::insertMatchingSubMap2d: every range data (robot frame) inserted in order, each one insertion, at pose Twr (3x4 row-major). */
int  visfs_submaps_insert(visfs_submaps* s, const double Twr[12], int32_t n, const visfs_range_data* rd);

/* Number of active sub-maps (0, 1 or 2) in *n; info[0 .. *n) filled when info != NULL (capacity 2). */
int  visfs_submaps_describe(const visfs_submaps* s, int32_t* n, visfs_submap_info* info);
/* Sub-map `index`'s uint16 cells and float correspondence costs, [num_y_cells][num_x_cells]; either pointer may be NULL. */
int  visfs_submaps_download(const visfs_submaps* s, int32_t index, uint16_t* cells, float* cost);

/* visfs_ba_solve_window with w->grid replaced by the matching sub-map's device grid (no sub-map yet: no laser edges).  `s` must live
 * on the device of `h`. */
int  visfs_submaps_solve_window(visfs_ba_handle* h, const visfs_submaps* s, const visfs_ba_window* w, visfs_ba_result* r);

/* ---- host-only hooks (parity tests) ---------------------------------------------------------------------------------------- */
/* The cells of rayToPixelMask(begin, end, scale) from the per-column work items the kernels run, in the reference's order.
 * Returns the number of cells (written up to `cap`), or a negative VISFS_BA_* code. */
int  visfs_submap_hook_ray(const int32_t begin[2], const int32_t end[2], int32_t scale, int32_t cap, int32_t* cells_xy);
/* The same cells from the mark kernel's work items of the ray's record, sized as a batch sizes them (columns x chunks of 8 cells)
 * and walked in item order.  *n_items: the number of work items.  Returns the number of cells, or a negative VISFS_BA_* code. */
int  visfs_submap_hook_mark_items(const int32_t begin[2], const int32_t end[2], int32_t scale, int32_t cap, int32_t* cells_xy,
                                  int64_t* n_items);
/* computeLookupTableToApplyCorrespondenceCostOdds(odds) (32768 entries, each with the update marker). */
int  visfs_submap_hook_odds_table(double odds, uint16_t* table);
/* The value tables: correspondence cost of every value (0 = unknown -> max cost; 32768 doubles) and the crop's
 * value -> probability -> value round trip (32768 entries, 0 -> 0). */
int  visfs_submap_hook_value_tables(double* cost, uint16_t* crop);
/* ProbabilityGrid::computeCroppedGrid of a grid [ny][nx] with known box `box` (min_x, min_y, max_x, max_y; empty: min > max).
 * out_dims = (offset_x, offset_y, num_x, num_y); out_cells [num_y][num_x] (capacity `cap` cells); out_box the cropped known box. */
int  visfs_submap_hook_crop(int32_t nx, int32_t ny, const uint16_t* cells, const int32_t box[4], int64_t cap, int32_t out_dims[4],
                            uint16_t* out_cells, int32_t out_box[4]);

#ifdef __cplusplus
}
#endif
#endif
