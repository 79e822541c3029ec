// The objects of include/visfs_mcl.h as ba_mcl.hip holds them, and what ba_mcl.hip and ba_mcl_kld.hip ask of each other
// (include/visfs_mcl_kld.h).  Internal: nothing here is exported.
#pragma once

#include "ba_host.hpp"
#include "ba_mcl.hpp"
#include "ba_submap.hpp"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

struct visfs_mcl;
namespace mcl {
struct Kld;
void kld_free(visfs_mcl* f);                 // ba_mcl_kld.hip, called only when f->kld is set
}

struct visfs_mcl_field {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    submap::Limits L;
    int32_t R = 0, T = 0, v_occ = 0;
    std::vector<uint16_t> h_t;
    std::vector<int64_t> h_q;                 // both flavours keep the table
    host::DeviceBuf<uint16_t> d_t;
    host::DeviceBuf<int64_t> d_q;
    host::Counts counts;

    ~visfs_mcl_field() {                      // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

struct visfs_mcl {
    visfs_mcl_field* field = nullptr;
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int32_t N = 0, lanes = 0, cur = 0;
    int32_t n = 0;                            // the active count, which is also the stride of the particle arrays: N unless kld moved it
    uint64_t seed = 0;
    int64_t update = 0;
    // twin: x, y, yaw, w each [n] at stride n, two buffers of 4 N
    std::vector<double> h_st[2];
    std::vector<int64_t> h_Q;
    std::vector<int32_t> h_anc;
    // device
    host::DeviceBuf<double> d_st[2];
    host::DeviceBuf<double> d_cs;
    host::DeviceBuf<int64_t> d_Q;
    host::DeviceBuf<int32_t> d_anc;
    host::DeviceBuf<uint64_t> d_C;
    host::DeviceBuf<uint64_t> d_bsum;
    host::DeviceBuf<double> d_part;
    host::DeviceBuf<double> d_pbw;
    host::DeviceBuf<int32_t> d_pbi;
    host::PinnedBuf<char> h_up;               // pinned: the header and the beams
    host::DeviceBuf<char> d_up;
    host::PinnedBuf<mcl::Rec> h_rec;          // pinned
    host::DeviceBuf<mcl::Rec> d_rec;
    visfs_mcl_result last;
    bool have_last = false;
    host::Counts counts;
    mcl::Kld* kld = nullptr;                  // null: the plain filter

    ~visfs_mcl() {                            // before the members free what they own
        if (kld) mcl::kld_free(this);
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace mcl {

// ---- ba_mcl.hip
// visfs_mcl_upload with a count: the refusals, the copy at stride n, and n becomes the active count.
int upload_n(visfs_mcl* f, int32_t n, const double* x, const double* y, const double* yaw, const double* w);

// Where k_mcl_finish writes the record of a KLD update: the head of the longer record that the update downloads.
Rec* kld_device_rec(visfs_mcl* f);
// The fourth launch of a KLD update, its one download and its one wait; `rec` and the pending counts are filled.
int kld_device_resample(visfs_mcl* f, const Hdr* up, const double* st, double* out, int32_t blocks, Rec& rec);
// The twin's resampling: C [n + 1] is the inclusive-exclusive prefix of the counts, rec.resampled is set.
void kld_host_resample(visfs_mcl* f, const Hdr& H, const std::vector<uint64_t>& C, Rec& rec);
// After an update that succeeded: the last KLD result, and the new active count.
void kld_commit(visfs_mcl* f, const Rec& rec, int32_t n_before);
// After an init or an upload that succeeded: hypotheses of the particles that were replaced (include/visfs_mcl_hyp.h) are gone.
void kld_particles_replaced(visfs_mcl* f);

}  // namespace mcl
