// The place-recognition objects (include/visfs_place.h) as the sources that work on them see them: ba_place.hip, which owns them, and
// ba_place_verify.hip, which runs the query's two launches in front of its own.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ba_host.hpp"
#include "ba_place.hpp"
#include "../../include/visfs_place.h"

namespace place {

// A describe of n key-points writes rows 0 .. n - 1 only, and visfs_place_db_add copies the whole block: rows from n on keep what
// an earlier, longer describe left, on the device and on the twin alike.  Every reader stops at the slot's count (Payload::n) or the
// set's n, and no hook shows a row beyond it.
struct SlotBlock {                         // what a store keeps of a set: the head of SetBlock
    uint32_t desc[kMaxPoints][kDescWords];
    uint8_t valid[kMaxPoints];
};
struct SetBlock {
    uint32_t desc[kMaxPoints][kDescWords];
    uint8_t valid[kMaxPoints];
    uint8_t bin[kMaxPoints];
    float xy[kMaxPoints][2];
};
struct Payload {                           // a slot's words, uploaded in one copy
    int32_t id[kMaxPoints];
    float xyz[kMaxPoints][3];
    int64_t key;
    int32_t n, pad;
};
static_assert(offsetof(SetBlock, valid) == offsetof(SlotBlock, valid) && sizeof(SlotBlock) == 16896, "a slot is the head of a set");
static_assert(sizeof(visfs_place_row) == 36 && sizeof(visfs_place_result) % 4 == 0, "the result block is written as words");

struct Counts4 {
    int32_t uploads = 0, launches = 0, downloads = 0, waits = 0;
    int read(int32_t* u, int32_t* l, int32_t* d, int32_t* w) const {
        if (u) *u = uploads;
        if (l) *l = launches;
        if (d) *d = downloads;
        if (w) *w = waits;
        return VISFS_BA_OK;
    }
};

}  // namespace place

struct visfs_place_set {
    std::string err;
    visfs_flow* flow = nullptr;
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    int32_t capacity = 0, n = 0;
    bool described = false;
    place::Counts4 counts;
    place::SetBlock* host = nullptr;       // the twin's set
    ::host::DeviceBuf<place::SetBlock> d_set;
    ::host::DeviceBuf<place::Table> d_table;
    ::host::PinnedBuf<float> h_xy;           // pinned: a call's key-points
    ::host::Event up_done;                   // behind the copy out of h_xy
    bool up_pending = false;

    ~visfs_place_set() {                   // before the members free what they own
        if (device) {
            (void)hipSetDevice(dev);
            if (stream) (void)hipStreamSynchronize(stream);
        }
        delete host;
    }
};

struct visfs_place_db {
    std::string err;
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    int32_t max_keyframes = 0, size = 0;
    place::Counts4 counts;
    std::vector<place::SlotBlock> hslots;  // the twin's store
    std::vector<place::Payload> hpay;
    ::host::DeviceBuf<place::SlotBlock> d_slots;
    ::host::DeviceBuf<place::Payload> d_pay;
    ::host::DeviceBuf<int32_t> d_match;      // [max_keyframes][512]
    ::host::DeviceBuf<int32_t> d_counts;
    ::host::DeviceBuf<place::Params> d_prm;
    ::host::DeviceBuf<visfs_place_result> d_result;
    ::host::PinnedBuf<char> h_io;            // pinned: a Payload going up, Params going up, the result coming down
    ::host::Event up_done;                   // behind the copy of a Payload out of h_io
    bool up_pending = false;

    ~visfs_place_db() {                    // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace place {

// The checks of visfs_place_query and the clipped range, in that call's order and with its codes; *why: a string literal.
int prepare_query(const visfs_place_db* db, const visfs_place_set* s, const visfs_place_params& p, Params* q, const char** why);
// k_place_match and k_place_rank on the store's stream: d_prm holds q already (stream order), R is where the ranking writes.
// Returns the number of launches issued, or -1 when one was refused.
int launch_query(const visfs_place_db* db, const visfs_place_set* s, const Params& q, const Params* d_prm, visfs_place_result* d_R);

}  // namespace place
