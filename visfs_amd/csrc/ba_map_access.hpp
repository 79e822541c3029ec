// What ba_map.hip lends the likelihood field of ba_mcl.hip (struct visfs_map is private to ba_map.hip).
#pragma once
#include "ba_submap_access.hpp"

struct visfs_map;

namespace gmap {

// The last composed grid where it lives: dense cells [ny][nx] of the limits, in the memory `device` says.
struct MapAccess {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    bool have = false;                        // a grid has been composed
    submap::Limits L;
    const uint16_t* cells = nullptr;
};

}  // namespace gmap

int visfs_internal_map_access(visfs_map* m, gmap::MapAccess* a);
