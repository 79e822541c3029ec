// The member tables of a tracker group (include/visfs_tracker_group.h) and the batched enqueue functions of the
// translation units that own the kernels: ba_flow.hip (pyramids), ba_clahe.hip (equalised level 0), ba_corners.hip (corner
// extraction).  ba_tracker.hip owns the group, fills one pinned block with every table of a call, sends it up in one copy and hands each
// function the device address of its records.  The member index of every batched kernel is blockIdx.z.
#pragma once
#include <vector>

#include "ba_clahe.hpp"
#include "ba_corners.hpp"
#include "ba_flow_object.hpp"
#include "ba_host.hpp"

namespace flow {

struct GroupCounts : host::Counts {};         // what a group call issued

struct PyrRec {                                // the slot a member's frame goes into
    uint8_t* px[2];
    uint32_t* der[2];
};

struct ClaheRec {
    const uint8_t* raw[2];
    uint8_t* lut[2];
    int32_t* hist[2];
    uint8_t* dst[2];                           // level 0 of the slot
};

struct CornerDev;                              // ba_corners.hip
struct CornerRec {                             // one corner extraction of a member: its arguments and its state
    const uint8_t* px;
    const Disc* discs;
    const int32_t* hw;
    const int32_t* args;                       // { number of raster discs, max_corners } in device memory
    float* eig;
    uint8_t* mask;
    uint64_t* keys;
    uint64_t* sorted;
    CornerDev* st;
    float* xy;
    int32_t skip, pad;                         // the member takes no part in this extraction
};

// group_stage: the copies of device_stage without its wait (the caller has waited once for the whole group).
int group_stage(visfs_flow* f, uint8_t* const dst[2], const uint8_t* left, const uint8_t* right, int32_t stride, GroupCounts* cnt);
void group_pyr_fill(const visfs_flow* f, int slot, PyrRec* r);
int group_pyramids(visfs_flow* f, int n, const PyrRec* d_recs, GroupCounts* cnt);          // f: any member (geometry, stream)

// group_clahe_prepare: allocates the member's CLAHE state (at group creation).  group_clahe_fill returns where the raw images go.
int group_clahe_prepare(visfs_flow* f);
void group_clahe_fill(visfs_flow* f, const clahe::Geom& g, int slot, ClaheRec* r, uint8_t* raw[2]);
int group_clahe(visfs_flow* f, const clahe::Geom& g, int n, const ClaheRec* d_recs, GroupCounts* cnt);
void group_clahe_pushed(visfs_flow* f, const clahe::Geom& g);                              // the bookkeeping of a completed push

int group_corners_prepare(visfs_flow* f);
void group_corners_fill(visfs_flow* f, const uint8_t* px, const Disc* d_discs, const int32_t* d_hw, const int32_t* d_args, bool skip,
                        CornerRec* r, const int32_t** d_n_out, const float** d_xy);
int group_corners(visfs_flow* f, double quality_level, double min_distance, int n, const CornerRec* d_recs, GroupCounts* cnt);

}  // namespace flow

namespace fund {

struct CullRec;                                // ba_fund.hpp
struct CullShape;
// The search and the winner's mask of the fundamental-matrix cull for the n members of a tracker call (ba_fund.hip, DESIGN.md section
// 9j): two launches with grid.z = n behind the rows kernel of ba_tracker.hip.  max_rows: the most rows any member can have.
int group_cull(hipStream_t stream, int n, const CullRec* d_recs, int32_t max_rows, const CullShape& S, flow::GroupCounts* cnt);
// The same steps for a host-twin tracker, the rows and the conditioning included.
void cull_host(const CullRec& r, const float* from_xy, const float* to_xy, const uint8_t* lk_st, int32_t n_from, const CullShape& S);

}  // namespace fund

struct visfs_pnp_params;                       // include/visfs_pnp.h
struct visfs_pnp;
struct visfs_pnp_camera;

namespace pnp {

struct PnpRec;                                 // ba_pnp.hpp
struct RefineFromRec;
struct PnpShape;
struct Row;
struct Result;
struct Cam;
// The search and the refinement of the pose guess for the n members of a tracker call (ba_pnp.hip): two
// launches with grid.z = n behind the rows kernel of ba_tracker.hip.
int group_pnp(hipStream_t stream, int n, const PnpRec* d_recs, const PnpShape& S, flow::GroupCounts* cnt);
// The refinement alone for the n members of a call, each from the model its record names (k_pnp_refine_from_g, DESIGN.md section
// 9x): one launch with grid.z = n.  host_refine_from is its twin on a solver of visfs_pnp_create_host, which then reports the passes
// through visfs_pnp_download; S.min_inliers is already raised to 4.
int group_refine_from(hipStream_t stream, int n, const RefineFromRec* d_recs, const PnpShape& S, flow::GroupCounts* cnt);
int host_refine_from(visfs_pnp* p, const Row* rows, int32_t m, const Cam& K, const PnpShape& S, const double start_tq[7], Result* res,
                     std::vector<int32_t>* inliers);
// the model block of the last visfs_pnp_solve or host_refine_from of a solver
const Result& last_result(const visfs_pnp* p);
// The parameter check of visfs_pnp_solve; `why` is a string literal.
int check_params(const visfs_pnp_params& q, const visfs_pnp_camera& c, const char** why);
// MultiviewGeometry.cpp:147-205 from the model and the inliers (numbers of `rows`), on the host in every flavour: the transform
// (Tir * pnp)^-1 into T_out[16] and the scaling of the covariance cov[36], which the caller has set to the identity.  matches[k]:
// the input row of rows[k]; to_xyz: per input row, or NULL.
void finalize(const Result& res, const Row* rows, const double Tir[12], const Cam& K, const int32_t* inliers, size_t n_inliers,
              const int32_t* matches, const float* to_xyz, double* T_out, double* cov);

}  // namespace pnp
