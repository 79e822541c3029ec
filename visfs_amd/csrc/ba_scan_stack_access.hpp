// What ba_scan_fast.hip lends the global map of ba_map.hip (stack_build is private to ba_scan_fast.hip).
#pragma once
#include <string>

#include "ba_submap_access.hpp"

struct visfs_scan_stack;

// A stack of `depth` levels (already checked to lie in [1, 16]) over limits `L`, built by stack_build from the grid `g` in the memory
// of the given flavour (device: read on `stream`, which is waited for before the call returns).  On failure *out stays null and
// `err` has the text.
int visfs_internal_stack_from_view(bool device, int dev, hipStream_t stream, const submap::Limits& L, const submap::GridView& g, int32_t depth,
                                   visfs_scan_stack** out, std::string* err);
