// The tracker object behind include/visfs_flow.h, shared by the translation units that work on it: ba_flow.hip (pyramids, LK passes)
// ba_corners.hip (corner extraction, include/visfs_corners.h) and ba_clahe.hip (the equalised frame push, include/visfs_clahe.h).
#pragma once
#include "ba_flow.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_flow.h"

#include <string>
#include <vector>

namespace flow {
struct CornerState;                       // ba_corners.hip
void corners_release(visfs_flow* f);      // frees what the first visfs_flow_corners call of f allocated (no-op before it)
struct ClaheState;                        // ba_clahe.hip
void clahe_release(visfs_flow* f);        // likewise for the first visfs_flow_push_frame_clahe call
struct TrackerState;                      // ba_tracker.hip
void tracker_release(visfs_flow* f);      // detaches the trackers made on f: their calls fail from then on, their memory is freed

// Corner extraction for the resident front end (ba_corners.hip): the host restatement with the raster's discs given as they are
// (max_corners <= 0: nothing runs and the count is 0).  The device form is group_corners of ba_group.hpp.
struct Disc;
int corners_host(visfs_flow* f, const uint8_t* px, int32_t max_corners, double quality_level, double min_distance, const Disc* discs,
                 int n_discs, const int32_t* hw, float* xy, int32_t* n_out);

// The steps of a frame push (ba_flow.hip), for the pushes that put something else than the caller's bytes into level 0.
// device_stage: waits for the stream, then copies both images through the pinned block to dst[0], dst[1] (w * h bytes each).
int device_stage(visfs_flow* f, uint8_t* const dst[2], const uint8_t* left, const uint8_t* right, int32_t stride);
// device_pyramids / host_pyramids: levels 1 .. max_level and the Scharr derivatives of every level from the level 0 of `slot`.
int device_pyramids(visfs_flow* f, int slot);
void host_pyramids(visfs_flow* f, int slot, int image);
}  // namespace flow

struct visfs_flow {
    visfs_flow_params prm{};
    flow::LkParams lk{};
    int32_t w = 0, h = 0;
    flow::Layout lay{};
    std::string err;
    bool device = false;
    int frames = 0;              // pushed so far
    int cur = 0;                 // slot of the current pair

    // host restatement: [slot][image]
    std::vector<uint8_t> hpx[2][2];
    std::vector<uint32_t> hder[2][2];

    // device
    visfs_ba_handle* ba = nullptr;
    int dev = 0;
    hipStream_t stream = nullptr;
    host::DeviceBuf<char> d_mem; // the four images' pixels and derivatives
    uint8_t* dpx[2][2] = {};
    uint32_t* dder[2][2] = {};
    host::PinnedBuf<uint8_t> h_img;  // both level-0 images of a frame
    host::Staged<char> io;       // a call's points in, results out
    int32_t io_cap = 0;          // points

    // corner extraction (ba_corners.hip): nothing until the first visfs_flow_corners call
    flow::CornerState* corners = nullptr;

    // equalised push (ba_clahe.hip): nothing until the first visfs_flow_push_frame_clahe call
    flow::ClaheState* clahe = nullptr;

    // resident front end (ba_tracker.hip): the trackers made on this object, nothing until the first visfs_tracker_create
    flow::TrackerState* trackers = nullptr;

    ~visfs_flow() {              // before the members free what they own; the three states above went in visfs_flow_destroy
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};
