/*
 * visfs_flow.h — pyramidal Lucas-Kanade tracking with stereo triangulation on the GPU (implemented in libvisfs_ba_hip.so).
 *
 * The pixel half of the reference's Tracker::imageProcess (corelib/src/Tracker.cpp:233-274, :343-388): the four
 * cv::calcOpticalFlowPyrLK passes of a frame (previous-left -> left and back, left -> right and back) with their forward-backward
 * gates, and generateKeyPoints3DStereo (MultiviewGeometry.cpp:57-92) for the stereo survivors.  It produces the `word_uv` /
 * `word_xyz` arguments of visfs_window_insert.  The image pyramids and their Scharr derivatives stay in device memory across frames;
 * the calls run as HIP kernels on the stream of the handle the object was created on.  Corner extraction on the same resident
 * images is include/visfs_corners.h and the PnP guess is include/visfs_pnp.h; the fundamental-matrix cull that replaces the forward-backward gate when flow_back is off is include/visfs_fund.h.  DESIGN.md section 9c states the arithmetic (restated from OpenCV's published
 * algorithm; parity with OpenCV itself is not pinned) and the one deliberate deviation (exact integer window sums).
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_FLOW_H
#define VISFS_FLOW_H

#include <stdint.h>
#include "visfs_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_FLOW_ABI_VERSION 1

/* The Tracker keys (Parameters.h:148-157) and the two gates written into Tracker.cpp. */
typedef struct visfs_flow_params {
    int32_t win_size;           /* Tracker/FlowWinSize      (default 21; 3 .. 21 (even sizes allowed, as in calcOpticalFlowPyrLK)) */
    int32_t max_level;          /* Tracker/FlowMaxLevel     (default 3; 0 .. 7) */
    int32_t iterations;         /* Tracker/FlowIterations   (default 30) */
    float   eps;                /* Tracker/FlowEps          (default 0.01) */
    int32_t flow_back;          /* Tracker/FlowBack         (default 1) */
    float   min_eig_threshold;  /* calcOpticalFlowPyrLK's minEigThreshold (1e-4, Tracker.cpp:259) */
    float   back_gate_track;    /* round-trip gate of the temporal pass, px (1.5, Tracker.cpp:268) */
    float   back_gate_stereo;   /* round-trip gate of the stereo pass, px (0.5, Tracker.cpp:364) */
    float   min_depth;          /* Tracker/MinDepth         (default 0.2; negative: no lower gate) */
    float   max_depth;          /* Tracker/MaxDepth         (default 10.0; <= 0: no upper gate) */
} visfs_flow_params;

/* What generateKeyPoints3DStereo reads of the two GeometricCamera. */
typedef struct visfs_flow_camera {
    float fx, fy, cx, cy;       /* left camera, cvKfloat() */
    float cx_right;             /* right camera's cx */
    float baseline;             /* getBaseLine() */
    double Tir[12];             /* getTansformImageToRobot(), 3x4 row-major */
} visfs_flow_camera;

/* Slots and images of the test hooks. */
#define VISFS_FLOW_SLOT_PREVIOUS 0
#define VISFS_FLOW_SLOT_CURRENT  1
#define VISFS_FLOW_IMAGE_LEFT    0
#define VISFS_FLOW_IMAGE_RIGHT   1

typedef struct visfs_flow visfs_flow;

int  visfs_flow_abi_version(void);
void visfs_flow_default_params(visfs_flow_params* p);

/* A tracker for width x height images on the device and stream of handle `h`; every buffer of a frame is allocated here. */
int  visfs_flow_create(visfs_ba_handle* h, const visfs_flow_params* p, int32_t width, int32_t height, visfs_flow** out);
/* The host restatement (one core, no device): the same work items in sequence, for parity tests. */
int  visfs_flow_create_host(const visfs_flow_params* p, int32_t width, int32_t height, visfs_flow** out);
void visfs_flow_destroy(visfs_flow* f);
const char* visfs_flow_last_error(const visfs_flow* f);

/* A stereo pair of 8-bit grey images, `stride` bytes per row.  Builds both pyramids (levels 0 .. max_level) and the Scharr
 * derivative of every level; the pair pushed before becomes "previous". */
int  visfs_flow_push_frame(visfs_flow* f, const uint8_t* left, const uint8_t* right, int32_t stride);

/* previous-left -> current-left for from_xy[n][2]; guess_xy[n][2] (or NULL) starts the search there (OPTFLOW_USE_INITIAL_FLOW).
 * With flow_back, the reverse pass from to_xy and the gate status && reverse status && |reverse - from| <= back_gate_track.
 * Output in input order: to_xy[n][2], status[n], err[n] (the minimum eigenvalue of the forward pass; may be NULL).  The in-bounds
 * test and the compaction (Tracker.cpp:285-301) stay with the caller.  VISFS_BA_ERR_NOT_LOADED before the second frame. */
int  visfs_flow_track(visfs_flow* f, int32_t n, const float* from_xy, const float* guess_xy, float* to_xy, uint8_t* status, float* err);

/* current-left -> current-right for left_xy[n][2] with the back_gate_stereo round trip, then generateKeyPoints3DStereo: xyz[n][3] in
 * the robot frame for the survivors, a NaN triple where the reference leaves badPoint or status is 0.  The in-bounds test of
 * Tracker.cpp:376 stays with the caller.  VISFS_BA_ERR_NOT_LOADED before the first frame. */
int  visfs_flow_stereo(visfs_flow* f, int32_t n, const float* left_xy, const visfs_flow_camera* cam, float* right_xy, uint8_t* status,
                       float* xyz);

/* ---- test hooks -------------------------------------------------------------------------------------------------------------- */
/* Size of pyramid level `level`. */
int  visfs_flow_level_size(const visfs_flow* f, int32_t level, int32_t* width, int32_t* height);
/* Level `level` of image `image` of slot `slot`: pixels [h][w] uint8 and derivative [h][w][2] int16 (Ix, Iy); either may be NULL. */
int  visfs_flow_download_level(const visfs_flow* f, int32_t slot, int32_t image, int32_t level, uint8_t* pixels, int16_t* derivative);
/* generateKeyPoints3DStereo alone (host arithmetic, the function the kernel runs): n pairs, xyz[n][3]. */
int  visfs_flow_hook_triangulate(const visfs_flow_params* p, const visfs_flow_camera* cam, int32_t n, const float* left_xy,
                                 const float* right_xy, float* xyz);

#ifdef __cplusplus
}
#endif
#endif
