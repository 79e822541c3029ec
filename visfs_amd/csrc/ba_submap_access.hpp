// What ba_submap.hip lends the scan matcher of ba_scan.hip (struct visfs_submaps is private to ba_submap.hip).
#pragma once
#include "ba_submap.hpp"

#include <string>

struct visfs_submaps;

namespace submap {

// The cells of a sub-map as a match reads them: the allocation [ny][nx] and where the limits' cell (0, 0) lies in it (ox, oy)
// (a device allocation may trail its limits by a growth that no batch has realised yet; cells outside it are unknown).
struct GridView {
    const uint16_t* cells = nullptr;
    int32_t nx = 0, ny = 0, ox = 0, oy = 0;
};

struct ScanAccess {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    int32_t count = 0;                        // active sub-maps
    Limits L;                                 // sub-map `index`: the limits in force
    GridView grid;                            // ... and its cells (device or host memory, as `device` says)
};

}  // namespace submap

// Flushes a staged insertion batch (device flavour, as visfs_submaps_download finds it), then describes sub-map `index`; only
// `device`, `dev`, `stream` and `count` are filled when `index` names no active sub-map.
int visfs_internal_scan_access(visfs_submaps* s, int32_t index, submap::ScanAccess* a);
int visfs_internal_scan_fail(visfs_submaps* s, int rc, const char* why);
// the opaque sub-maps as a sink of ba_host.hpp's HIP_TRY and guarded
inline void set_error(visfs_submaps* s, const std::string& text) { if (s) (void)visfs_internal_scan_fail(s, VISFS_BA_ERR_DEVICE, text.c_str()); }
// The matcher's state, kept by the sub-maps object and freed with `destroy` (on the sub-maps' device) when they go.
void** visfs_internal_scan_slot(visfs_submaps* s, void (*destroy)(void*));
// The same for the refinement's state (ba_scan_refine.hip).
void** visfs_internal_refine_slot(visfs_submaps* s, void (*destroy)(void*));
