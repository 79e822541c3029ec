// The tracker object behind include/visfs_flow.h, shared by the translation units that work on it: ba_flow.hip (pyramids, LK passes)
// and ba_corners.hip (corner extraction, include/visfs_corners.h).
#pragma once
#include "ba_flow.hpp"
#include "../../include/visfs_flow.h"

#include <string>
#include <vector>

namespace flow {
struct CornerState;                       // ba_corners.hip
void corners_release(visfs_flow* f);      // frees what the first visfs_flow_corners call of f allocated (no-op before it)
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
    char* d_mem = nullptr;       // the four images' pixels and derivatives
    uint8_t* dpx[2][2] = {};
    uint32_t* dder[2][2] = {};
    uint8_t* h_img = nullptr;    // pinned: both level-0 images of a frame
    char* h_io = nullptr;        // pinned: a call's points in, results out
    char* d_io = nullptr;
    int32_t io_cap = 0;          // points

    // corner extraction (ba_corners.hip): nothing until the first visfs_flow_corners call
    flow::CornerState* corners = nullptr;
};
