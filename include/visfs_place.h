/*
 * visfs_place.h — visual place recognition on the resident images of a visfs_flow object (implemented in libvisfs_ba_hip.so).
 *
 * Two parts: a 256-bit steered binary descriptor on key-points of a resident level-0 image, and a matcher of one frame's
 * descriptors against a store of key-frames that returns, per recognised key-frame, the from_xyz / to_xy rows visfs_pnp_solve
 * takes.  The reference's localisation launch files run rtabmap beside VISFS for this (Kp/DetectorStrategy 8: GFTT corners with ORB
 * descriptors, Kp/MaxFeatures 500, Mem/STMSize 30); corners (visfs_corners.h), words with 3-D points and the PnP solve exist here
 * already.  The descriptor is in the manner of the ORB paper (intensity-centroid orientation quantised to 32 bins, one pre-rotated
 * test pattern per bin, 5 x 5 box sums) but it is NOT OpenCV's ORB: OpenCV's table of 256 pairs is not restated here, the pattern
 * is drawn from a counter hash instead, and parity with OpenCV is not pinned.  DESIGN.md section 9w is the definition; all of it is
 * integer arithmetic behind the one lrintf of a key-point's centre, so a device object and a host twin give the same bytes.
 *
 * Objects made on a device flow object / a handle run HIP kernels on the stream of the owning handle; objects made on a host flow
 * object / on NULL run the same arithmetic on one core.  A set must be destroyed before its flow object, a store before its handle.
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_PLACE_H
#define VISFS_PLACE_H

#include <stdint.h>
#include "visfs_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_PLACE_ABI_VERSION     1
#define VISFS_PLACE_MAX_POINTS      512     /* key-points of a set, entries of a key-frame */
#define VISFS_PLACE_MAX_KEYFRAMES   1024
#define VISFS_PLACE_MAX_CANDIDATES  8
#define VISFS_PLACE_DESC_BYTES      32
#define VISFS_PLACE_BINS            32
#define VISFS_PLACE_MARGIN          15      /* a centre is valid from 15 to w - 16 and from 15 to h - 16 */
#define VISFS_PLACE_QUERY_LAUNCHES  2
#define VISFS_PLACE_NO_SECOND       257     /* d2 of a query whose slot holds one valid entry */

typedef struct visfs_place_set visfs_place_set;     /* the descriptors of one frame */
typedef struct visfs_place_db  visfs_place_db;      /* the key-frame store */

typedef struct visfs_place_params {
    int32_t first_slot, last_slot;      /* half open; default 0, 1024 (clipped to the slots in use) */
    int32_t max_distance;               /* default 64; 0 .. 256 */
    int32_t ratio_num, ratio_den;       /* default 4 / 5; accepted iff d1 * ratio_den < d2 * ratio_num; 1 .. 1024 each */
    int32_t min_matches;                /* default 40; 0 .. 512: a slot is a candidate iff count >= min_matches */
    int32_t cross_check;                /* default 1 */
} visfs_place_params;

typedef struct visfs_place_row {        /* one accepted match: what visfs_pnp_solve takes as from_xyz / to_xy, and where it came from */
    int32_t query_index, db_index, distance, id;
    float   from_xyz[3];                /* the entry's 3-D point */
    float   to_xy[2];                   /* the query key-point as given to visfs_place_describe */
} visfs_place_row;

typedef struct visfs_place_candidate {
    int32_t slot, count;
    int64_t key;
} visfs_place_candidate;

typedef struct visfs_place_result {
    int32_t status;                     /* VISFS_BA_OK */
    int32_t n_slots;                    /* slots in the clipped range */
    int32_t n_candidates;
    int32_t first_slot;                 /* count[k] belongs to slot first_slot + k */
    visfs_place_candidate candidate[VISFS_PLACE_MAX_CANDIDATES];    /* by count descending, then slot ascending; unused: zero */
    int32_t count[VISFS_PLACE_MAX_KEYFRAMES];                       /* unused: zero */
    visfs_place_row row[VISFS_PLACE_MAX_CANDIDATES][VISFS_PLACE_MAX_POINTS];    /* candidate c: row[c][0 .. count), ascending query_index; unused: zero */
} visfs_place_result;

int  visfs_place_abi_version(void);
void visfs_place_default_params(visfs_place_params* p);

/* ---- the descriptor set ------------------------------------------------------------------------------------------------------- */
/* A set of the flavour of f.  VISFS_BA_ERR_BAD_ARGUMENT: capacity < 1; VISFS_BA_ERR_UNSUPPORTED: capacity > 512. */
int  visfs_place_set_create(visfs_flow* f, int32_t capacity, visfs_place_set** out);
void visfs_place_set_destroy(visfs_place_set* s);
const char* visfs_place_set_last_error(const visfs_place_set* s);
/* Describes xy[n][2] on level 0 of image `image` of slot `slot` (VISFS_FLOW_SLOT_*, VISFS_FLOW_IMAGE_*); 0 <= n <= capacity.  A
 * key-point whose coordinates are not finite or whose centre lies closer than 15 pixels to an edge gets 32 zero bytes and valid 0
 * (a coordinate outside [-1, w] or [-1, h] is refused before it is rounded; by the same rule it is invalid anyway).
 * On the device: one upload, one launch (k_place_describe), no download, no wait.  VISFS_BA_ERR_BAD_ARGUMENT: slot, image or n out of
 * range, an image smaller than 31 x 31; VISFS_BA_ERR_NOT_LOADED: the slot holds no frame. */
int  visfs_place_describe(visfs_place_set* s, int32_t slot, int32_t image, int32_t n, const float* xy);
/* uploads, launches, downloads and stream waits of the last visfs_place_describe of s */
int  visfs_place_set_last_counts(const visfs_place_set* s, int32_t* uploads, int32_t* launches, int32_t* downloads, int32_t* waits);

/* ---- the key-frame store ------------------------------------------------------------------------------------------------------ */
/* h: a handle (device store) or NULL (host twin).  VISFS_BA_ERR_BAD_ARGUMENT: max_keyframes < 1; VISFS_BA_ERR_UNSUPPORTED: > 1024. */
int  visfs_place_db_create(visfs_ba_handle* h, int32_t max_keyframes, visfs_place_db** out);
void visfs_place_db_destroy(visfs_place_db* db);
const char* visfs_place_db_last_error(const visfs_place_db* db);
/* Appends the set as it stands as the next slot: its descriptors and valid flags (device to device), ids[n] and xyz[n][3] (the
 * words' ids and 3-D points; n is the set's) and key in one upload.  *slot_out: the slot taken.  VISFS_BA_ERR_UNSUPPORTED: the store
 * is full; VISFS_BA_ERR_BAD_ARGUMENT: set and store of different flavours (or of different handles);
 * VISFS_BA_ERR_NOT_LOADED: the set was never described. */
int  visfs_place_db_add(visfs_place_db* db, const visfs_place_set* s, const int32_t* ids, const float* xyz, int64_t key, int32_t* slot_out);
int  visfs_place_db_reset(visfs_place_db* db);
int  visfs_place_db_size(const visfs_place_db* db, int32_t* n_slots);
/* The nearest-neighbour search of the set against the slots [first_slot, min(last_slot, size)): DESIGN.md 9w.  On the device: one
 * upload, two launches (k_place_match, k_place_rank), one download, one wait, for any number of slots.
 * VISFS_BA_ERR_BAD_ARGUMENT: a parameter out of its range, first_slot > last_slot, different flavours;
 * VISFS_BA_ERR_NOT_LOADED: the set was never described. */
int  visfs_place_query(visfs_place_db* db, const visfs_place_set* s, const visfs_place_params* p, visfs_place_result* result);
/* uploads, launches, downloads and stream waits of the last visfs_place_query of db */
int  visfs_place_last_counts(const visfs_place_db* db, int32_t* uploads, int32_t* launches, int32_t* downloads, int32_t* waits);

/* ---- test hooks --------------------------------------------------------------------------------------------------------------- */
/* The last describe of s; any pointer may be NULL.  xy[n][2], desc[n][32], valid[n], bin[n].  VISFS_BA_ERR_NOT_LOADED before the first call. */
int  visfs_place_set_download(visfs_place_set* s, int32_t* n, float* xy, uint8_t* desc, uint8_t* valid, uint8_t* bin);
/* A test hook only: puts n <= capacity key-points with given descriptors into s in place of a describe, so the matcher can be tested
 * on descriptors made to order (ties, duplicates, a lone entry).  xy[n][2], desc[n][32], valid[n]; the bins become 0.  It looks at no
 * image: the frame check of visfs_place_describe is bypassed, and the set counts as described even when its flow object holds no
 * frame.  Waits for the copies. */
int  visfs_place_set_upload(visfs_place_set* s, int32_t n, const float* xy, const uint8_t* desc, const uint8_t* valid);
/* One slot of the store; any pointer may be NULL.  desc[n][32], valid[n], ids[n], xyz[n][3]. */
int  visfs_place_db_download(visfs_place_db* db, int32_t slot, int32_t* n, int64_t* key, uint8_t* desc, uint8_t* valid, int32_t* ids, float* xyz);
/* The rotated test points: pts[bin][point][x, y]; test t of bin k compares point 2t with point 2t + 1. */
int  visfs_place_hook_pattern(int8_t* pts);

#ifdef __cplusplus
}
#endif
#endif
