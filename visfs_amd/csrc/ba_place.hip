// Visual place recognition on the resident images of a visfs_flow object (include/visfs_place.h), two ways over
// the arithmetic of ba_place.hpp:
//   * the one-core twin (sets of host flow objects, stores made on NULL): describe_one, match_slot, rank_slots in sequence;
//   * device, on the stream of the owning handle:
//       k_place_describe  one wavefront per key-point: the 31 x 31 patch staged in LDS with the two moments summed on the way (integer
//                         wave reduction), the 27 x 27 box sums of 5 x 5 pixels kept in LDS as uint16, the 32 orientation scores by
//                         lanes 0-31 and an integer maximum, the 256 bits by four ballots (lane l takes tests l + 64 j)
//       k_place_match     one workgroup of 512 threads per slot in range.  First a thread owns an entry and walks the valid queries
//                         for the column minimum D * 1024 + i (the cross-check), then it owns a query and walks the valid entries for
//                         the nearest and the second nearest; the row walked is the same for every lane, so its address is
//                         wave-uniform.  No atomic but the count's.
//       k_place_rank      one workgroup: eight workgroup-wide maxima on count * 1024 + (1023 - slot), then the winners' rows in
//                         ascending query order by ballot prefix, written straight into the result block
// Every result is a minimum of integers or a count, so no schedule shows in the bytes.
#include "ba_place.hpp"
#include "ba_place_object.hpp"
#include "ba_flow_object.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_place.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

using namespace place;
using namespace host;

namespace place {

// ---------------------------------------------------------------- kernels
constexpr int kMatchT = 512, kRankT = 1024;
constexpr int kPatchStride = 32;

__global__ __launch_bounds__(64) void k_place_describe(const uint8_t* __restrict__ px, int w, int h, const Table* __restrict__ T,
                                                       SetBlock* __restrict__ set, int n) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    __shared__ uint8_t sP[kPatch * kPatchStride];
    __shared__ uint16_t sB[kBox * kBox];
    int cx, cy;
    if (!centre_of(set->xy[i][0], set->xy[i][1], w, h, &cx, &cy)) {       // the same for every lane
        if (lane < kDescWords) set->desc[i][lane] = 0u;
        if (lane == 0) { set->valid[i] = 0; set->bin[i] = 0; }
        return;
    }
    int32_t m10 = 0, m01 = 0;
    for (int q = lane; q < kPatch * kPatch; q += 64) {
        const int r = q / kPatch, c = q - r * kPatch;
        const int v = px[(int64_t)(cy - kMargin + r) * w + (cx - kMargin + c)];
        sP[r * kPatchStride + c] = (uint8_t)v;
        const int dx = c - kMargin, dy = r - kMargin;
        if (dx * dx + dy * dy <= kMargin * kMargin) { m10 += dx * v; m01 += dy * v; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { m10 += __shfl_xor(m10, o, 64); m01 += __shfl_xor(m01, o, 64); }
    __syncthreads();
    for (int q = lane; q < kBox * kBox; q += 64) {                        // the box about (u - 13, v - 13): patch rows v .. v + 4
        const int v = q / kBox, u = q - v * kBox;
        int s = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int k = 0; k < 5; ++k) s += sP[(v + j) * kPatchStride + u + k];
        sB[q] = (uint16_t)s;
    }
    __syncthreads();
    long long score = lane < kBins ? (long long)bin_score(T->rot[lane & (kBins - 1)], m10, m01) : (long long)INT64_MIN;
    int bin = lane;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long os = __shfl_xor(score, o, 64);
        const int ob = __shfl_xor(bin, o, 64);
        if (os > score || (os == score && ob < bin)) { score = os; bin = ob; }
    }
    const uint32_t* tests = reinterpret_cast<const uint32_t*>(&T->pts[bin][0][0]);       // test t: points 2t and 2t + 1, four bytes
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p = tests[lane + 64 * j];
        const int ax = (int8_t)(p & 0xff), ay = (int8_t)((p >> 8) & 0xff), bx = (int8_t)((p >> 16) & 0xff), by = (int8_t)(p >> 24);
        const bool bit = sB[(ay + kReach) * kBox + ax + kReach] < sB[(by + kReach) * kBox + bx + kReach];
        const unsigned long long b = __ballot(bit);
        if (lane == 0) { set->desc[i][2 * j] = (uint32_t)b; set->desc[i][2 * j + 1] = (uint32_t)(b >> 32); }
    }
    if (lane == 0) { set->valid[i] = 1; set->bin[i] = (uint8_t)bin; }
}

__global__ __launch_bounds__(kMatchT) void k_place_match(const SetBlock* __restrict__ set, int nq, const SlotBlock* __restrict__ slots,
                                                         const Payload* __restrict__ pay, const Params* __restrict__ prm,
                                                         int32_t* __restrict__ match, int32_t* __restrict__ counts) {
    const Params p = *prm;
    const int k = blockIdx.x, t = threadIdx.x;
    if (k >= p.n_slots) return;
    const SlotBlock& S = slots[p.first + k];
    const int ne = pay[p.first + k].n;
    __shared__ int32_t col[kMaxPoints];
    __shared__ int32_t s_count;
    if (t == 0) s_count = 0;
    int32_t m = 0x7fffffff;
    if (t < ne && S.valid[t]) {
        uint32_t e[kDescWords];
#pragma unroll
        for (int q = 0; q < kDescWords; ++q) e[q] = S.desc[t][q];
        for (int i = 0; i < nq; ++i) {
            if (!set->valid[i]) continue;
            const int32_t key = hamming(set->desc[i], e) * 1024 + i;
            m = key < m ? key : m;
        }
    }
    col[t] = m;
    __syncthreads();
    int32_t out = -1;
    if (t < nq && set->valid[t]) {
        uint32_t q8[kDescWords];
#pragma unroll
        for (int q = 0; q < kDescWords; ++q) q8[q] = set->desc[t][q];
        Nearest nn;
        for (int j = 0; j < ne; ++j) {
            if (!S.valid[j]) continue;
            nn.take(hamming(q8, S.desc[j]), j);
        }
        if (nn.best != 0x7fffffff) {
            const int j1 = nn.best & 1023;
            if (accepted(nn, t, col[j1], p)) out = pack_match(j1, nn.best >> 10);
        }
    }
    if (t < nq) match[k * kMaxPoints + t] = out;
    const unsigned long long b = __ballot(out >= 0);
    if ((t & 63) == 0 && b) atomicAdd(&s_count, (int32_t)__popcll(b));
    __syncthreads();
    if (t == 0) counts[k] = s_count;
}

__global__ __launch_bounds__(kRankT) void k_place_rank(const SetBlock* __restrict__ set, int nq, const Payload* __restrict__ pay,
                                                       const Params* __restrict__ prm, const int32_t* __restrict__ match,
                                                       const int32_t* __restrict__ counts, visfs_place_result* __restrict__ R) {
    const Params p = *prm;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ int32_t wmax[kRankT / 64];
    __shared__ int32_t s_cand[kMaxCandidates];
    __shared__ int32_t wcount[kRankT / 64];
    uint32_t* words = reinterpret_cast<uint32_t*>(R);
    for (int q = t; q < (int)(sizeof(visfs_place_result) / 4); q += kRankT) words[q] = 0u;
    __syncthreads();
    const int32_t cnt = t < p.n_slots ? counts[t] : 0;
    int32_t key = t < p.n_slots ? rank_key(cnt, p.first + t, p.min_matches) : -1;
    if (t < p.n_slots) R->count[t] = cnt;
    int n_cand = 0;
    for (int c = 0; c < kMaxCandidates; ++c) {
        int32_t m = key;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int32_t other = __shfl_xor(m, o, 64); m = other > m ? other : m; }
        if (lane == 0) wmax[wave] = m;
        __syncthreads();
        int32_t best = -1;
        for (int q = 0; q < kRankT / 64; ++q) best = wmax[q] > best ? wmax[q] : best;
        if (best >= 0 && key == best) { s_cand[c] = t; key = -1; }        // the keys of two slots differ
        __syncthreads();
        if (best < 0) break;                                             // the same for every thread
        ++n_cand;
    }
    if (t == 0) { R->status = VISFS_BA_OK; R->n_slots = p.n_slots; R->n_candidates = n_cand; R->first_slot = p.first; }
    for (int c = 0; c < n_cand; ++c) {
        const int k = s_cand[c], slot = p.first + k;
        const Payload& P = pay[slot];
        const int32_t mt = t < nq ? match[k * kMaxPoints + t] : -1;
        const unsigned long long b = __ballot(mt >= 0);
        if (lane == 0) wcount[wave] = (int32_t)__popcll(b);
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int q = 0; q < kRankT / 64; ++q) {
            if (q < wave) before += wcount[q];
            total += wcount[q];
        }
        if (mt >= 0) {
            visfs_place_row& r = R->row[c][before + __popcll(b & ((1ull << lane) - 1ull))];
            const int j1 = mt & 0xffff;
            r.query_index = t; r.db_index = j1; r.distance = mt >> 16; r.id = P.id[j1];
            r.from_xyz[0] = P.xyz[j1][0]; r.from_xyz[1] = P.xyz[j1][1]; r.from_xyz[2] = P.xyz[j1][2];
            r.to_xy[0] = set->xy[t][0]; r.to_xy[1] = set->xy[t][1];
        }
        if (t == 0) { R->candidate[c].slot = slot; R->candidate[c].count = total; R->candidate[c].key = P.key; }
        __syncthreads();
    }
}

}  // namespace place

namespace {

const Table& host_table() {
    static const Table* t = [] { Table* x = new Table(); (void)make_table(x); return x; }();
    return *t;
}

}  // namespace

// ---------------------------------------------------------------- the objects (ba_place_object.hpp)
namespace {

constexpr size_t kIoBytes = sizeof(visfs_place_result) > sizeof(Payload) ? sizeof(visfs_place_result) : sizeof(Payload);

int set_alloc(visfs_place_set* s) {
    HIP_TRY(s, hipSetDevice(s->dev));
    RC_TRY(s->d_set.alloc(s, 1));
    RC_TRY(s->d_table.alloc(s, 1));
    RC_TRY(s->h_xy.alloc(s, 2 * kMaxPoints));
    RC_TRY(s->up_done.create(s, hipEventDisableTiming));
    HIP_TRY(s, hipMemsetAsync(s->d_set.get(), 0, sizeof(SetBlock), s->stream));
    HIP_TRY(s, hipMemcpyAsync(s->d_table.get(), &host_table(), sizeof(Table), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(s, hipStreamSynchronize(s->stream));
    return VISFS_BA_OK;
}

int db_alloc(visfs_place_db* db) {
    const size_t K = (size_t)db->max_keyframes;
    HIP_TRY(db, hipSetDevice(db->dev));
    RC_TRY(db->d_slots.alloc(db, K));
    RC_TRY(db->d_pay.alloc(db, K));
    RC_TRY(db->d_match.alloc(db, K * kMaxPoints));
    RC_TRY(db->d_counts.alloc(db, K));
    RC_TRY(db->d_prm.alloc(db, 1));
    RC_TRY(db->d_result.alloc(db, 1));
    RC_TRY(db->h_io.alloc(db, kIoBytes));
    RC_TRY(db->up_done.create(db, hipEventDisableTiming));
    return VISFS_BA_OK;
}

// the pinned block is written again only when the copy out of it has finished (the kernels behind it are not waited for)
template <class T> int pinned_free(T* o) {
    if (!o->up_pending) return VISFS_BA_OK;
    HIP_TRY(o, hipEventSynchronize(o->up_done.get()));
    o->up_pending = false;
    return VISFS_BA_OK;
}

int flavour_text(const visfs_place_db* db, const visfs_place_set* s, const char** why) {
    if (db->device != s->device) { *why = "the set and the store are of different flavours"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (db->device && (db->dev != s->dev || db->stream != s->stream)) {
        *why = "the set and the store belong to different handles"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    if (!s->described) { *why = "the set was never described"; return VISFS_BA_ERR_NOT_LOADED; }
    return VISFS_BA_OK;
}

int same_flavour(visfs_place_db* db, const visfs_place_set* s) {
    const char* why = "";
    const int rc = flavour_text(db, s, &why);
    return rc == VISFS_BA_OK ? rc : fail(db, rc, why);
}

int check_params(const visfs_place_params& p, const char** why) {
    if (p.first_slot < 0 || p.last_slot < p.first_slot) { *why = "the slot range is not 0 <= first_slot <= last_slot"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p.max_distance < 0 || p.max_distance > 256) { *why = "max_distance must lie in 0 .. 256"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p.ratio_num < 1 || p.ratio_num > 1024 || p.ratio_den < 1 || p.ratio_den > 1024) {
        *why = "ratio_num and ratio_den must lie in 1 .. 1024"; return VISFS_BA_ERR_BAD_ARGUMENT;
    }
    if (p.min_matches < 0 || p.min_matches > kMaxPoints) { *why = "min_matches must lie in 0 .. 512"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    return VISFS_BA_OK;
}

void host_query(const visfs_place_db* db, const visfs_place_set* s, const Params& p, visfs_place_result* R) {
    std::memset(R, 0, sizeof(*R));
    const SetBlock& Q = *s->host;
    std::vector<int32_t> match((size_t)std::max(p.n_slots, 1) * kMaxPoints, -1);
    for (int k = 0; k < p.n_slots; ++k) {
        const SlotBlock& S = db->hslots[(size_t)(p.first + k)];
        R->count[k] = match_slot(&Q.desc[0][0], Q.valid, s->n, &S.desc[0][0], S.valid, db->hpay[(size_t)(p.first + k)].n, p,
                                 match.data() + (size_t)k * kMaxPoints);
    }
    int32_t cand[kMaxCandidates];
    const int n_cand = rank_slots(R->count, p, cand);
    R->status = VISFS_BA_OK; R->n_slots = p.n_slots; R->n_candidates = n_cand; R->first_slot = p.first;
    for (int c = 0; c < n_cand; ++c) {
        const int k = cand[c], slot = p.first + k;
        const Payload& P = db->hpay[(size_t)slot];
        int32_t rows = 0;
        for (int i = 0; i < s->n; ++i) {
            const int32_t mt = match[(size_t)k * kMaxPoints + i];
            if (mt < 0) continue;
            visfs_place_row& r = R->row[c][rows++];
            const int j1 = mt & 0xffff;
            r.query_index = i; r.db_index = j1; r.distance = mt >> 16; r.id = P.id[j1];
            std::memcpy(r.from_xyz, P.xyz[j1], sizeof r.from_xyz);
            std::memcpy(r.to_xy, Q.xy[i], sizeof r.to_xy);
        }
        R->candidate[c].slot = slot; R->candidate[c].count = rows; R->candidate[c].key = P.key;
    }
}

int device_query(visfs_place_db* db, const visfs_place_set* s, const Params& p, visfs_place_result* R) {
    HIP_TRY(db, hipSetDevice(db->dev));
    const int rc = pinned_free(db);
    if (rc != VISFS_BA_OK) return rc;
    std::memcpy(db->h_io.get(), &p, sizeof p);
    HIP_TRY(db, hipMemcpyAsync(db->d_prm.get(), db->h_io.get(), sizeof p, hipMemcpyHostToDevice, db->stream));
    if (launch_query(db, s, p, db->d_prm.get(), db->d_result.get()) != VISFS_PLACE_QUERY_LAUNCHES) {
        HIP_TRY(db, hipGetLastError());
        return fail(db, VISFS_BA_ERR_DEVICE, "a launch of the query was refused");
    }
    HIP_TRY(db, hipMemcpyAsync(db->h_io.get(), db->d_result.get(), sizeof(visfs_place_result), hipMemcpyDeviceToHost, db->stream));
    HIP_TRY(db, hipStreamSynchronize(db->stream));
    std::memcpy(R, db->h_io.get(), sizeof(*R));
    if (R->n_slots != p.n_slots || R->n_candidates < 0 || R->n_candidates > kMaxCandidates)
        return fail(db, VISFS_BA_ERR_DEVICE, "the ranking returned an impossible block");
    db->counts = Counts4{ 1, VISFS_PLACE_QUERY_LAUNCHES, 1, 1 };
    return VISFS_BA_OK;
}

}  // namespace

namespace place {

int prepare_query(const visfs_place_db* db, const visfs_place_set* s, const visfs_place_params& p, Params* q, const char** why) {
    int rc = check_params(p, why);
    if (rc != VISFS_BA_OK) return rc;
    rc = flavour_text(db, s, why);
    if (rc != VISFS_BA_OK) return rc;
    q->first = std::min(p.first_slot, db->size);
    q->n_slots = std::min(p.last_slot, db->size) - q->first;
    q->max_distance = p.max_distance; q->ratio_num = p.ratio_num; q->ratio_den = p.ratio_den; q->min_matches = p.min_matches;
    q->cross_check = p.cross_check ? 1 : 0;
    return VISFS_BA_OK;
}

int launch_query(const visfs_place_db* db, const visfs_place_set* s, const Params& p, const Params* d_prm, visfs_place_result* d_R) {
    hipLaunchKernelGGL(k_place_match, dim3((unsigned)std::max(p.n_slots, 1)), dim3(kMatchT), 0, db->stream, s->d_set.get(), s->n, db->d_slots.get(),
                       db->d_pay.get(), d_prm, db->d_match.get(), db->d_counts.get());
    if (hipPeekAtLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_place_rank, dim3(1), dim3(kRankT), 0, db->stream, s->d_set.get(), s->n, db->d_pay.get(), d_prm, db->d_match.get(), db->d_counts.get(), d_R);
    if (hipPeekAtLastError() != hipSuccess) return -1;
    return VISFS_PLACE_QUERY_LAUNCHES;
}

}  // namespace place

// ====================================================================== exported C ABI
extern "C" {

int visfs_place_abi_version(void) { return VISFS_PLACE_ABI_VERSION; }

void visfs_place_default_params(visfs_place_params* p) {
    if (!p) return;
    p->first_slot = 0; p->last_slot = kMaxKeyframes;
    p->max_distance = 64; p->ratio_num = 4; p->ratio_den = 5; p->min_matches = 40; p->cross_check = 1;
}

int visfs_place_set_create(visfs_flow* f, int32_t capacity, visfs_place_set** out) {
    if (!f || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(f, [&]() -> int {
        if (capacity < 1) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "capacity must be at least 1");
        if (capacity > kMaxPoints) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "capacity must not exceed 512");
        visfs_place_set* s = new visfs_place_set();
        s->flow = f; s->capacity = capacity; s->device = f->device; s->dev = f->dev; s->stream = f->stream;
        if (s->device) {
            const int rc = set_alloc(s);
            if (rc != VISFS_BA_OK) { f->err = s->err; delete s; return rc; }
        } else {
            s->host = new SetBlock();
            std::memset(s->host, 0, sizeof(SetBlock));
        }
        *out = s;
        return (int)VISFS_BA_OK;
    });
}

void visfs_place_set_destroy(visfs_place_set* s) { delete s; }

const char* visfs_place_set_last_error(const visfs_place_set* s) { return s ? s->err.c_str() : "null set"; }

int visfs_place_describe(visfs_place_set* s, int32_t slot, int32_t image, int32_t n, const float* xy) {
    if (!s || (n > 0 && !xy)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        visfs_flow* f = s->flow;
        if (slot < 0 || slot > 1 || image < 0 || image > 1) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "slot or image out of range");
        if (n < 0 || n > s->capacity) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "n must lie in 0 .. capacity");
        if (f->w < kPatch || f->h < kPatch) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "the image is smaller than 31 x 31");
        if (f->frames < (slot == VISFS_FLOW_SLOT_CURRENT ? 1 : 2)) return fail(s, VISFS_BA_ERR_NOT_LOADED, "no frame in that slot");
        const int sl = slot == VISFS_FLOW_SLOT_CURRENT ? f->cur : 1 - f->cur;
        if (!s->device) {
            SetBlock& B = *s->host;
            const Table& T = host_table();
            for (int i = 0; i < n; ++i) {
                B.xy[i][0] = xy[2 * i]; B.xy[i][1] = xy[2 * i + 1];
                describe_one(T, f->hpx[sl][image].data(), f->w, f->h, xy[2 * i], xy[2 * i + 1], reinterpret_cast<uint8_t*>(B.desc[i]), &B.valid[i],
                             &B.bin[i]);
            }
            s->n = n; s->described = true; s->counts = Counts4{};
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(s, hipSetDevice(s->dev));
        const int rc = pinned_free(s);
        if (rc != VISFS_BA_OK) return rc;
        s->described = false;
        const size_t bytes = sizeof(float) * 2 * (size_t)std::max(n, 1);
        if (n > 0) std::memcpy(s->h_xy.get(), xy, sizeof(float) * 2 * (size_t)n);
        else s->h_xy[0] = s->h_xy[1] = 0.0f;
        HIP_TRY(s, hipMemcpyAsync(&s->d_set->xy[0][0], s->h_xy.get(), bytes, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(s, hipEventRecord(s->up_done.get(), s->stream));
        s->up_pending = true;
        hipLaunchKernelGGL(k_place_describe, dim3((unsigned)std::max(n, 1)), dim3(64), 0, s->stream, f->dpx[sl][image], f->w, f->h, s->d_table.get(),
                           s->d_set.get(), n);
        HIP_TRY(s, hipGetLastError());
        s->n = n; s->described = true; s->counts = Counts4{ 1, 1, 0, 0 };
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_set_last_counts(const visfs_place_set* s, int32_t* uploads, int32_t* launches, int32_t* downloads, int32_t* waits) {
    if (!s) return VISFS_BA_ERR_BAD_ARGUMENT;
    return s->counts.read(uploads, launches, downloads, waits);
}

int visfs_place_set_download(visfs_place_set* s, int32_t* n, float* xy, uint8_t* desc, uint8_t* valid, uint8_t* bin) {
    if (!s) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        if (!s->described) return fail(s, VISFS_BA_ERR_NOT_LOADED, "no describe call to report on");
        if (n) *n = s->n;
        const size_t m = (size_t)s->n;
        if (m == 0 || (!xy && !desc && !valid && !bin)) return (int)VISFS_BA_OK;          // the count alone needs no wait
        if (!s->device) {
            const SetBlock& B = *s->host;
            if (xy) std::memcpy(xy, B.xy, m * 8);
            if (desc) std::memcpy(desc, B.desc, m * 32);
            if (valid) std::memcpy(valid, B.valid, m);
            if (bin) std::memcpy(bin, B.bin, m);
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(s, hipSetDevice(s->dev));
        if (xy) HIP_TRY(s, hipMemcpyAsync(xy, s->d_set->xy, m * 8, hipMemcpyDeviceToHost, s->stream));
        if (desc) HIP_TRY(s, hipMemcpyAsync(desc, s->d_set->desc, m * 32, hipMemcpyDeviceToHost, s->stream));
        if (valid) HIP_TRY(s, hipMemcpyAsync(valid, s->d_set->valid, m, hipMemcpyDeviceToHost, s->stream));
        if (bin) HIP_TRY(s, hipMemcpyAsync(bin, s->d_set->bin, m, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(s, hipStreamSynchronize(s->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_set_upload(visfs_place_set* s, int32_t n, const float* xy, const uint8_t* desc, const uint8_t* valid) {
    if (!s || (n > 0 && (!xy || !desc || !valid))) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(s, [&]() -> int {
        if (n < 0 || n > s->capacity) return fail(s, VISFS_BA_ERR_BAD_ARGUMENT, "n must lie in 0 .. capacity");
        const size_t m = (size_t)n;
        std::vector<char> mem(sizeof(SetBlock), 0);
        SetBlock* B = reinterpret_cast<SetBlock*>(mem.data());
        if (m > 0) {
            std::memcpy(B->xy, xy, m * 8);
            std::memcpy(B->desc, desc, m * 32);
            for (size_t i = 0; i < m; ++i) B->valid[i] = valid[i] ? 1 : 0;
        }
        if (s->device) {
            HIP_TRY(s, hipSetDevice(s->dev));
            HIP_TRY(s, hipMemcpyAsync(s->d_set.get(), B, sizeof(SetBlock), hipMemcpyHostToDevice, s->stream));
            HIP_TRY(s, hipStreamSynchronize(s->stream));
        } else {
            std::memcpy(s->host, B, sizeof(SetBlock));
        }
        s->n = n; s->described = true; s->counts = Counts4{};
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_db_create(visfs_ba_handle* h, int32_t max_keyframes, visfs_place_db** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    std::string why;
    const int rc = guarded(&why, [&]() -> int {
        if (max_keyframes < 1) { why = "max_keyframes must be at least 1"; return VISFS_BA_ERR_BAD_ARGUMENT; }
        if (max_keyframes > kMaxKeyframes) { why = "max_keyframes must not exceed 1024"; return VISFS_BA_ERR_UNSUPPORTED; }
        visfs_place_db* db = new visfs_place_db();
        db->max_keyframes = max_keyframes;
        if (h) {
            db->device = true; db->dev = visfs_internal_device(h); db->stream = visfs_internal_stream(h);
            const int r = db_alloc(db);
            if (r != VISFS_BA_OK) { why = db->err; delete db; return r; }
        } else {
            db->hslots.resize((size_t)max_keyframes);
            db->hpay.resize((size_t)max_keyframes);
        }
        *out = db;
        return (int)VISFS_BA_OK;
    });
    if (rc != VISFS_BA_OK && h) visfs_internal_set_error(h, why.c_str());
    return rc;
}

void visfs_place_db_destroy(visfs_place_db* db) { delete db; }

const char* visfs_place_db_last_error(const visfs_place_db* db) { return db ? db->err.c_str() : "null store"; }

int visfs_place_db_add(visfs_place_db* db, const visfs_place_set* s, const int32_t* ids, const float* xyz, int64_t key, int32_t* slot_out) {
    if (!db || !s || !slot_out) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(db, [&]() -> int {
        int rc = same_flavour(db, s);
        if (rc != VISFS_BA_OK) return rc;
        if (s->n > 0 && (!ids || !xyz)) return fail(db, VISFS_BA_ERR_BAD_ARGUMENT, "ids and xyz are needed for a set that is not empty");
        if (db->size >= db->max_keyframes) return fail(db, VISFS_BA_ERR_UNSUPPORTED, "the store is full");
        const int slot = db->size;
        Payload* P = db->device ? reinterpret_cast<Payload*>(db->h_io.get()) : &db->hpay[(size_t)slot];
        if (db->device) {
            HIP_TRY(db, hipSetDevice(db->dev));
            rc = pinned_free(db);
            if (rc != VISFS_BA_OK) return rc;
        }
        std::memset(P, 0, sizeof(Payload));
        if (s->n > 0) {
            std::memcpy(P->id, ids, sizeof(int32_t) * (size_t)s->n);
            std::memcpy(P->xyz, xyz, sizeof(float) * 3 * (size_t)s->n);
        }
        P->key = key; P->n = s->n;
        if (db->device) {
            HIP_TRY(db, hipMemcpyAsync(&db->d_slots[slot], s->d_set.get(), sizeof(SlotBlock), hipMemcpyDeviceToDevice, db->stream));
            HIP_TRY(db, hipMemcpyAsync(&db->d_pay[slot], P, sizeof(Payload), hipMemcpyHostToDevice, db->stream));
            HIP_TRY(db, hipEventRecord(db->up_done.get(), db->stream));
            db->up_pending = true;
        } else {
            std::memcpy(&db->hslots[(size_t)slot], s->host, sizeof(SlotBlock));
        }
        db->size = slot + 1;
        *slot_out = slot;
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_db_reset(visfs_place_db* db) {
    if (!db) return VISFS_BA_ERR_BAD_ARGUMENT;
    db->size = 0;
    return VISFS_BA_OK;
}

int visfs_place_db_size(const visfs_place_db* db, int32_t* n_slots) {
    if (!db || !n_slots) return VISFS_BA_ERR_BAD_ARGUMENT;
    *n_slots = db->size;
    return VISFS_BA_OK;
}

int visfs_place_query(visfs_place_db* db, const visfs_place_set* s, const visfs_place_params* p, visfs_place_result* result) {
    if (!db || !s || !p || !result) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(db, [&]() -> int {
        Params q;
        const char* why = "";
        const int rc = prepare_query(db, s, *p, &q, &why);
        if (rc != VISFS_BA_OK) return fail(db, rc, why);
        if (db->device) return device_query(db, s, q, result);
        host_query(db, s, q, result);
        db->counts = Counts4{};
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_last_counts(const visfs_place_db* db, int32_t* uploads, int32_t* launches, int32_t* downloads, int32_t* waits) {
    if (!db) return VISFS_BA_ERR_BAD_ARGUMENT;
    return db->counts.read(uploads, launches, downloads, waits);
}

int visfs_place_db_download(visfs_place_db* db, int32_t slot, int32_t* n, int64_t* key, uint8_t* desc, uint8_t* valid, int32_t* ids, float* xyz) {
    if (!db) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(db, [&]() -> int {
        if (slot < 0 || slot >= db->size) return fail(db, VISFS_BA_ERR_BAD_ARGUMENT, "no such slot");
        std::vector<char> pay_mem(sizeof(Payload)), slot_mem(sizeof(SlotBlock));
        Payload* P = reinterpret_cast<Payload*>(pay_mem.data());
        SlotBlock* S = reinterpret_cast<SlotBlock*>(slot_mem.data());
        if (db->device) {
            HIP_TRY(db, hipSetDevice(db->dev));
            HIP_TRY(db, hipMemcpyAsync(P, &db->d_pay[slot], sizeof(Payload), hipMemcpyDeviceToHost, db->stream));
            HIP_TRY(db, hipMemcpyAsync(S, &db->d_slots[slot], sizeof(SlotBlock), hipMemcpyDeviceToHost, db->stream));
            HIP_TRY(db, hipStreamSynchronize(db->stream));
        } else {
            std::memcpy(P, &db->hpay[(size_t)slot], sizeof(Payload));
            std::memcpy(S, &db->hslots[(size_t)slot], sizeof(SlotBlock));
        }
        if (P->n < 0 || P->n > kMaxPoints) return fail(db, VISFS_BA_ERR_DEVICE, "the slot holds an impossible count");
        const size_t m = (size_t)P->n;
        if (n) *n = P->n;
        if (key) *key = P->key;
        if (desc) std::memcpy(desc, S->desc, m * 32);
        if (valid) std::memcpy(valid, S->valid, m);
        if (ids) std::memcpy(ids, P->id, m * 4);
        if (xyz) std::memcpy(xyz, P->xyz, m * 12);
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_hook_pattern(int8_t* pts) {
    if (!pts) return VISFS_BA_ERR_BAD_ARGUMENT;
    std::memcpy(pts, host_table().pts, sizeof(host_table().pts));
    return VISFS_BA_OK;
}

}  // extern "C"
