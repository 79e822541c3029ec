/*
 * visfs_corners.h — corner extraction on the resident images of a visfs_flow object (implemented in libvisfs_ba_hip.so).
 *
 * The two cv::goodFeaturesToTrack calls of the reference's Tracker::imageProcess (corelib/src/Tracker.cpp:181 for a first frame,
 * :327 to top the words up to Tracker/MaxFeatures) with OpenCV's defaults (blockSize 3, gradientSize 3, minimum-eigenvalue response,
 * no Harris), and the mask of Tracker::getMask (:116-141) built from a list of discs.  The image is level 0 of a pyramid that
 * visfs_flow_push_frame already keeps on the device; the mask is rasterised there too, so neither crosses to the host.  On an
 * object of visfs_flow_create the call runs as HIP kernels on the stream of the owning handle; on an object of
 * visfs_flow_create_host the same arithmetic runs on one core.  DESIGN.md section 9d states the arithmetic (restated from OpenCV's
 * published algorithm; parity with OpenCV itself is not pinned) and the one deliberate deviation (exact integer box sums).
 *
 * The buffers of this path are allocated at the first visfs_flow_corners call of an object, not at visfs_flow_create.
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_CORNERS_H
#define VISFS_CORNERS_H

#include <stdint.h>
#include "visfs_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_CORNERS_ABI_VERSION 1
#define VISFS_CORNERS_MAX_CORNERS 4096
#define VISFS_CORNERS_MAX_RADIUS  32768

typedef struct visfs_corners_params {
    int32_t max_corners;        /* Tracker/MaxFeatures      (default 300; 1 .. 4096) */
    double  quality_level;      /* Tracker/QualityLevel     (default 0.01; > 0) */
    double  min_distance;       /* Tracker/MinDistance      (default 40.0; >= 0, below 1: no distance test) */
} visfs_corners_params;

/* One disc of the mask: centre (lrintf(x), lrintf(y)), filled as cv::circle(..., thickness = -1) fills it. */
typedef struct visfs_corners_disc {
    float   x, y;
    int32_t radius;             /* 0 .. 32768 */
} visfs_corners_disc;

int  visfs_corners_abi_version(void);
void visfs_corners_default_params(visfs_corners_params* p);      /* 300, 0.01, 40.0: Parameters.h:148-150 */

/* goodFeaturesToTrack on level 0 of image `image` of slot `slot` (VISFS_FLOW_SLOT_*, VISFS_FLOW_IMAGE_*).
 * discs[n_discs], in the order given: a disc whose centre lies in the image is drawn only if its centre pixel is still free
 * (Tracker.cpp:132, :136); a centre outside the image is drawn without that test, clipped.  n_discs == 0: no mask.
 * Output: xy[n][2] (integer-valued, strongest first, in the order of acceptance) and *n_out = n <= max_corners <= capacity.
 * VISFS_BA_ERR_BAD_ARGUMENT: max_corners < 1 or > capacity, quality_level not finite or <= 0, min_distance not finite or negative, a
 * non-finite disc coordinate, a negative radius.  VISFS_BA_ERR_UNSUPPORTED: max_corners > 4096, a radius > 32768.
 * VISFS_BA_ERR_NOT_LOADED: the slot holds no frame. */
int  visfs_flow_corners(visfs_flow* f, int32_t slot, int32_t image, const visfs_corners_params* p, int32_t n_discs,
                        const visfs_corners_disc* discs, int32_t capacity, float* xy, int32_t* n_out);

/* ---- test hooks -------------------------------------------------------------------------------------------------------------- */
/* State of the last visfs_flow_corners call of f; any pointer may be NULL.  eig[h][w]: the response before thresholding;
 * mask[h][w]: 255 = free; disc_drawn[n_discs of that call, see visfs_flow_corners_last_discs]: 1 where the disc was drawn;
 * *n_candidates: the local maxima that entered the sort; *max_val: the largest response under the mask.  VISFS_BA_ERR_NOT_LOADED before the first call. */
int  visfs_flow_corners_download(const visfs_flow* f, float* eig, uint8_t* mask, uint8_t* disc_drawn, int32_t* n_candidates,
                                 float* max_val);
/* n_discs of the last visfs_flow_corners call of f: the length disc_drawn must have.  VISFS_BA_ERR_NOT_LOADED before the first call. */
int  visfs_flow_corners_last_discs(const visfs_flow* f, int32_t* n_discs);
/* The half-width table of a filled circle of that radius: hw[|dy|] for |dy| = 0 .. radius. */
int  visfs_corners_hook_halfwidth(int32_t radius, int32_t* hw);

#ifdef __cplusplus
}
#endif
#endif
