/*
 * visfs_map.h — a global occupancy map composed from frozen sub-maps (implemented in libvisfs_ba_hip.so).
 *
 * A visfs_map is an ordered set of at most 256 tiles and the grid composed from them.  A tile is the raw uint16 cells of one
 * sub-map, frozen with the limits it had, and a pose (x, y, yaw) that takes its grid frame into the map frame: the identity when
 * the sub-map is added, anchor_now o anchor_when_frozen^-1 after a pose-graph optimisation has moved its anchor
 * (visfs_map_pose_from_anchor).  visfs_map_compose draws every tile at its pose into one grid by nearest-neighbour sampling and
 * combines the values of the tiles that know a cell; the grid can be downloaded or frozen into a visfs_scan_stack
 * (visfs_scan_fast.h) without leaving the device.  A map made on a handle lives in device memory and is composed by a HIP kernel;
 * a map made with h == NULL is the one-core host twin; both give the same bytes.  DESIGN.md section 9r states the semantics.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.  Every refusal is decided on the host before anything is pushed, and leaves the
 * last composed grid and the last counts in place.
 */
#ifndef VISFS_MAP_H
#define VISFS_MAP_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_submap.h"
#include "visfs_scan_fast.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_MAP_ABI_VERSION 1

#define VISFS_MAP_MAX_TILES 256
#define VISFS_MAP_MAX_CELLS 67108864      /* cells of the composed grid (2^26) */
#define VISFS_MAP_MAX_TILE_BYTES 1073741824
#define VISFS_MAP_ODDS 0      /* default */
#define VISFS_MAP_LATEST 1
#define VISFS_MAP_OCCUPIED 2

typedef struct visfs_map_params {
    int32_t combine;
    double  resolution;           /* > 0; default 0.05; read when explicit_limits = 0 */
    int32_t explicit_limits;      /* 0: limits from the tiles' extents; 1: `limits` below */
    visfs_submap_info limits;     /* resolution, max_x, max_y, num_x_cells, num_y_cells are read */
} visfs_map_params;

typedef struct visfs_map_info {
    visfs_submap_info limits;     /* of the composed grid; known_* = the union of the drawn tiles' culling boxes (empty: min > max) */
    int32_t tiles, tiles_drawn;   /* drawn: tiles whose cell box meets the grid */
} visfs_map_info;

typedef struct visfs_map visfs_map;

int  visfs_map_abi_version(void);
void visfs_map_default_params(visfs_map_params* p);

/* A map on the device and stream of handle `h`; h == NULL: the one-core host twin. */
int  visfs_map_create(visfs_ba_handle* h, visfs_map** out);
void visfs_map_destroy(visfs_map* m);
const char* visfs_map_last_error(const visfs_map* m);

/* Sub-map `index` of `s` as it stands after every insertion made so far becomes the next tile, at pose (x, y, yaw); its index in
 * *tile.  The sub-maps must be of the map's flavour, device and stream (VISFS_BA_ERR_BAD_ARGUMENT otherwise).  On the device the cells
 * never cross to the host.  The update marker is stripped (v & 32767).  Later insertions into the sub-map, or its destruction, do
 * not change the tile. */
int  visfs_map_add_submap(visfs_map* m, visfs_submaps* s, int32_t index, const double pose[3], int32_t* tile);
/* The same from cells [num_y_cells][num_x_cells] and limits as visfs_submaps_download and visfs_submaps_describe hand them out
 * (resolution, max_x, max_y, num_x_cells, num_y_cells are read). */
int  visfs_map_add_grid(visfs_map* m, const visfs_submap_info* limits, const uint16_t* cells, const double pose[3], int32_t* tile);
/* The poses of tiles first .. first + count - 1 ([count][3]).  Host only: no launch, no copy. */
int  visfs_map_set_poses(visfs_map* m, int32_t first, int32_t count, const double* poses);
/* Drops every tile.  The last composed grid stays until the next compose. */
int  visfs_map_clear(visfs_map* m);
/* A tile's frozen limits (resolution, max_x, max_y, num_x_cells, num_y_cells; the known box is not kept: empty, min > max) and its
 * pose; either may be NULL. */
int  visfs_map_describe_tile(const visfs_map* m, int32_t tile, visfs_submap_info* limits, double pose[3]);

/* Draws the tiles.  The grid's limits are p->limits, or the tiles' transformed extents rounded outwards to multiples of
 * p->resolution.  Output cell (ix, iy) has its centre at X = max_x - (iy + 0.5) res, Y = max_y - (ix + 0.5) res; every tile in
 * increasing index is sampled at the cell of the centre taken into its frame; a cell outside the tile or of value 0 contributes
 * nothing.  count = the tiles that know the cell, saturating at 255; the value is 0 for count 0, else by p->combine: LATEST the value
 * of the highest tile index, OCCUPIED the smallest value (the largest probability), ODDS the value whose log-odds is nearest to the
 * clamped sum of the tiles' log-odds (visfs_map_hook_odds_table).  On the device: one upload, one launch, one wait. */
int  visfs_map_compose(visfs_map* m, const visfs_map_params* p, visfs_map_info* info);
/* The last composed grid: uint16 cells and uint8 counts, [num_y_cells][num_x_cells]; either pointer may be NULL. */
int  visfs_map_download(visfs_map* m, uint16_t* cells, uint8_t* count);
/* The last composed grid frozen with `depth` levels into a stack of the map's flavour, read where it lives.  The stack outlives the map. */
int  visfs_scan_stack_create_from_map(visfs_map* m, int32_t depth, visfs_scan_stack** out);

/* ---- host only --------------------------------------------------------------------------------------------------------------- */
/* The tile pose after a pose-graph optimisation: anchor_now o anchor_when_frozen^-1 (poses as x, y, yaw). */
int  visfs_map_pose_from_anchor(const double anchor_when_frozen[3], const double anchor_now[3], double pose_out[3]);
/* L[v] = llround(log((1 - c_v) / c_v) * 2^20), c_v the correspondence cost of value v; table[0] = 0. */
int  visfs_map_hook_odds_table(int32_t table[32768]);
/* The host plan of a compose without an object: the composed limits (known_* as visfs_map_info gives them) and per tile its culling
 * box in output cells, boxes[n][4] = (min_x, min_y, max_x, max_y), empty as min > max; *tiles_drawn may be NULL. */
int  visfs_map_plan(int32_t n_tiles, const visfs_submap_info* tile_limits, const double* poses, const visfs_map_params* p,
                    visfs_submap_info* limits, int32_t* boxes, int32_t* tiles_drawn);
/* What the last compose issued on the device (all zero on the twin and before any compose). */
int  visfs_map_last_counts(const visfs_map* m, int32_t* launches, int32_t* copies, int32_t* waits);

#ifdef __cplusplus
}
#endif
#endif
