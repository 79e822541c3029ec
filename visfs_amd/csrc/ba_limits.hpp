// ba_limits.hpp — the size limits that the host plan of an upload (ba_plan.hpp) shares with the kernels.  No HIP here: ba_device.hpp
// includes this file, and so does the CPU-only test driver of the plan.
#pragma once

namespace visfs_ba {

constexpr int LIN_CHUNK = 256;        // observations per pose-major workgroup
constexpr int MAX_PCG_ONE_ROW_POSES = 256; // persistent PCG with one workgroup per block row: all co-resident (256 CUs, >= 1 workgroup each)
constexpr int MAX_PCG_FREE_POSES = 1024;   // beyond 256 free poses a workgroup owns several block rows (<= 256 workgroups) and an owner thread up to 4 blocks
constexpr int RUN_MAX_W = 64;        // k_schur_runs: widest pose span of a run of landmarks (slot table [landmarks][span], 16-bit entries)
constexpr int RUN_MAX_TILES = 416;   // ... observations of one sub-batch (21 doubles of LDS each: two workgroups per CU)
constexpr int RUN_TILE = 21;         // ... doubles per staged tile: Q = N D (9), N (9), Pc (3)
constexpr int SCH_CHUNK = 64;         // co-observation pairs per Schur wavefront and pass (DeviceGraph::sch_chunk = 64 x passes)
constexpr int SM_MAX_N6 = 64;         // <= 10 free poses: the reduced camera system is solved in LDS

}  // namespace visfs_ba
