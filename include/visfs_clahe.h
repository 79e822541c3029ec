/*
 * visfs_clahe.h — contrast-limited adaptive histogram equalisation in front of the resident frame push (implemented in
 * libvisfs_ba_hip.so).
 *
 * The reference equalises both images of every frame before the tracker sees them when System/CLAHE is set
 * (corelib/src/System.cpp:107-111: cv::createCLAHE(3.0, cv::Size(8, 8))->apply on left and right; both shipped launch files set the
 * key).  visfs_flow_push_frame_clahe is visfs_flow_push_frame with that step in front: the raw images go to the device once, two
 * kernels equalise them straight into level 0 of the new "current" slot, and the pyramids and Scharr derivatives are built from the
 * equalised images.  DESIGN.md section 9g states the arithmetic (restated from OpenCV's published 8-bit algorithm; parity with
 * OpenCV itself is not pinned).
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_CLAHE_H
#define VISFS_CLAHE_H

#include <stdint.h>
#include "visfs_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_CLAHE_ABI_VERSION 1
#define VISFS_CLAHE_MAX_TILES 32

typedef struct visfs_clahe_params {
    double  clip_limit;   /* System.cpp:108: 3.0; 0 = no clipping; finite, >= 0 */
    int32_t tiles_x;      /* 8; 1 .. 32 */
    int32_t tiles_y;      /* 8; 1 .. 32 */
} visfs_clahe_params;

int  visfs_clahe_abi_version(void);
void visfs_clahe_default_params(visfs_clahe_params* p);          /* 3.0, 8, 8 */

/* visfs_flow_push_frame with cv::CLAHE::apply on both images first.  The equalised images become level 0 of the new "current" slot;
 * the pyramids and Scharr derivatives are built from them.  The caller's buffers are not written.  Works on objects of
 * visfs_flow_create (HIP kernels on the handle's stream) and of visfs_flow_create_host (one core, the same arithmetic); the buffers of
 * this path are allocated at the first call.  Read the equalised image back with visfs_flow_download_level(f, CURRENT, image, 0, ..).
 * VISFS_BA_ERR_BAD_ARGUMENT: NULL params, clip_limit not finite or negative, a tile count below 1, stride below the width.
 * VISFS_BA_ERR_UNSUPPORTED: a tile count above 32, or width <= tiles_x or height <= tiles_y (the reflected extension of an image
 * that does not divide into the tiles must be a single reflection). */
int  visfs_flow_push_frame_clahe(visfs_flow* f, const visfs_clahe_params* p,
                                 const uint8_t* left, const uint8_t* right, int32_t stride);

/* ---- test hooks -------------------------------------------------------------------------------------------------------------- */
/* Geometry and clip value for a w x h image: extended size, tile size, integer clip limit (0 = none). */
int  visfs_clahe_hook_geometry(const visfs_clahe_params* p, int32_t w, int32_t h,
                               int32_t* ext_w, int32_t* ext_h, int32_t* tile_w, int32_t* tile_h, int32_t* clip);
/* Tile counts of the last push_frame_clahe of f: VISFS_BA_ERR_NOT_LOADED before the first. */
int  visfs_flow_clahe_last_tiles(const visfs_flow* f, int32_t* tiles_x, int32_t* tiles_y);
/* State of the last push_frame_clahe of f, image = VISFS_FLOW_IMAGE_*; any pointer may be NULL.
 * lut[tiles_y][tiles_x][256] uint8; hist[tiles_y][tiles_x][256] int32, the histogram after clipping and redistribution.
 * VISFS_BA_ERR_NOT_LOADED before the first call. */
int  visfs_flow_clahe_download(const visfs_flow* f, int32_t image, uint8_t* lut, int32_t* hist);

#ifdef __cplusplus
}
#endif
#endif
