// The laser pretreatment with its voxel filters on the GPU (include/visfs_scan_filter.h).
//
//   k_scan_filter  one workgroup of 1024 per scan (the scan is the grid dimension), everything of that scan in one launch:
//                  the classification of every point, the fixed voxel filter over the returns and the misses of every subdivision
//                  in ONE table pass (the list a point belongs to is part of what is compared), the order-preserving compactions,
//                  the range cut and the adaptive search, which loops inside the workgroup with its counts in LDS.
// The table is open-addressed, 2 n slots of point indices at least, in LDS (at most 32768 slots = 128 KiB of the CU's 160 KiB, a
// static allocation): a slot is claimed by compare-and-swap, keys are compared through the index found there, a key match lowers
// the slot with an atomic minimum.  After the barrier a slot holds the lowest index of its voxel, whatever the order of arrival
// was; the number of claims is the number of voxels.  Integer LDS atomics only; no workgroup waits for another.
// A call is one upload (headers and points), one launch, one download (records, range data, match clouds, hook bytes) and one
// wait.  The one-core twin walks the same definition (ba_scan_filter.hpp) in index order.
#include "ba_scan_filter.hpp"
#include "ba_submap.hpp"
#include "ba_host.hpp"

#include <cstring>
#include <new>
#include <string>
#include <vector>

#pragma clang fp contract(off)

using namespace sfilt;
using namespace host;

namespace sfilt {

struct KParams {
    visfs_scan_pretreat_params pre;
    double voxel_size, max_length, max_range;
    int32_t min_points;
};

// ---------------------------------------------------------------- workgroup helpers (every work item calls them, in step)

// Sum of v over the workgroup.  ws: [2][kWaves] in LDS, seq: calls so far (two buffers in turn: one barrier per call suffices, as
// nobody can be two calls ahead of anybody).
__device__ inline int32_t block_sum(int32_t v, int32_t* ws, int32_t& seq) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    int32_t* w = ws + (seq & 1) * kWaves;
    ++seq;
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
    __syncthreads();
    int32_t total = 0;
    for (int k = 0; k < kWaves; ++k) total += w[k];
    return total;
}

// One tile of an order-preserving compaction: the flagged work items before this one in the workgroup, and the tile's total.
__device__ inline int32_t tile_rank(bool flag, int32_t* ws, int32_t& seq, int32_t& total) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t* w = ws + (seq & 1) * kWaves;
    ++seq;
    if (lane == 0) w[wave] = __popcll(b);
    __syncthreads();
    int32_t before = 0;
    total = 0;
    for (int k = 0; k < kWaves; ++k) {
        const int32_t v = w[k];
        total += v;
        if (k < wave) before += v;
    }
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// Point i with `key` enters the table from slot h.  `meta` (fixed filter) adds the list to what is compared.  1: i claimed an
// empty slot, its voxel is new.  Ends: the table has twice as many slots as points.
__device__ inline int32_t table_insert(int32_t* table, uint32_t mask, uint32_t h, int32_t i, uint64_t key, const uint64_t* keys, const uint8_t* meta) {
    for (;;) {
        int32_t j = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (j == kEmpty) {
            j = atomicCAS(&table[h], kEmpty, i);
            if (j == kEmpty) return 1;
        }
        if (keys[j] == key && (!meta || (meta[j] & kListMask) == (meta[i] & kListMask))) {
            if (i < j) atomicMin(&table[h], i);
            return 0;
        }
        h = (h + 1u) & mask;
    }
}

__device__ inline void copy3(double* dst, const double* src) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; }

__global__ __launch_bounds__(kThreads) void k_scan_filter(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint8_t* __restrict__ work, KParams P) {
    __shared__ int32_t table[kMaxSlots];
    __shared__ uint8_t meta[kMaxPoints];
    __shared__ int32_t ws[2 * kWaves];
    __shared__ int32_t s_bad;

    const int32_t tid = (int32_t)threadIdx.x;
    const ScanHdr& H = reinterpret_cast<const ScanHdr*>(in)[blockIdx.x];
    DevRec& R = reinterpret_cast<DevRec*>(out)[blockIdx.x];
    const int32_t n = H.n, S = P.pre.num_subdivisions;
    const double* raw = reinterpret_cast<const double*>(in + H.in_pts);
    double* rm = reinterpret_cast<double*>(out + H.out_rm);
    double* match = reinterpret_cast<double*>(out + H.out_match);
    uint8_t* hook = out + H.out_hook;
    double* pts = reinterpret_cast<double*>(work + H.work_pts);
    uint64_t* keys = reinterpret_cast<uint64_t*>(work + H.work_keys);
    int32_t seq = 0;

    double T[12], o[3];
    for (int k = 0; k < 12; ++k) T[k] = H.T[k];
    {
        const double og[3] = {H.origin[0], H.origin[1], H.origin[2]};
        transform_xyz(T, og, o);
    }
    if (tid == 0) s_bad = 0;
    const bool fixed = P.voxel_size > 0.0;
    const int32_t slots0 = table_slots(n);
    if (fixed) for (int32_t h = tid; h < slots0; h += kThreads) table[h] = kEmpty;
    __syncthreads();

    // ---- 1. the class, the subdivision and the point every input point becomes; its voxel
    for (int32_t i = tid; i < n; i += kThreads) {
        const double p[3] = {raw[3 * (size_t)i], raw[3 * (size_t)i + 1], raw[3 * (size_t)i + 2]};
        double q[3], v[3];
        transform_xyz(T, p, q);
        const int cls = classify(P.pre, o, q, v);
        uint8_t m = (uint8_t)(cls | (sub_of(n, S, i) << kSubShift));
        copy3(pts + 3 * (size_t)i, v);
        if (cls != VISFS_SCAN_FILTER_DROPPED) {
            if (fixed) {
                uint64_t key;
                if (!voxel_key(v, P.voxel_size, key)) s_bad = 1;
                keys[i] = key;
            } else {
                m |= kKept;
            }
        }
        meta[i] = m;
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) { R.status = VISFS_BA_ERR_UNSUPPORTED; R.n_returns = R.n_misses = R.n_in_range = R.n_match = R.passes = 0; R.match_length = 0.0; }
        return;
    }

    // ---- 2. the fixed filter: every list of the scan through one table
    if (fixed) {
        const uint32_t mask = (uint32_t)slots0 - 1u;
        for (int32_t i = tid; i < n; i += kThreads) {
            const uint8_t m = meta[i];
            if ((m & kClassMask) == VISFS_SCAN_FILTER_DROPPED) continue;
            const int32_t list = 2 * (m >> kSubShift) + ((m & kClassMask) == VISFS_SCAN_FILTER_MISS);
            const uint64_t key = keys[i];
            (void)table_insert(table, mask, hash_slot(key, list, slots0), i, key, keys, meta);
        }
        __syncthreads();
        for (int32_t h = tid; h < slots0; h += kThreads) {
            const int32_t j = table[h];
            if (j != kEmpty) meta[j] |= kKept;             // one slot per voxel: no two work items meet at a byte
        }
        __syncthreads();
    }

    // ---- 3. returns and misses, each in order; the misses follow the returns
    int32_t cnt = 0;
    for (int32_t i = tid; i < n; i += kThreads) cnt += (meta[i] & (kKept | kClassMask)) == (kKept | VISFS_SCAN_FILTER_RETURN);
    const int32_t n_ret = block_sum(cnt, ws, seq);
    int32_t base_r = 0, base_m = 0;
    for (int32_t i0 = 0; i0 < n; i0 += kThreads) {
        const int32_t i = i0 + tid;
        const uint8_t m = i < n ? meta[i] : (uint8_t)0;
        const bool is_r = (m & kKept) && (m & kClassMask) == VISFS_SCAN_FILTER_RETURN;
        const bool is_m = (m & kKept) && (m & kClassMask) == VISFS_SCAN_FILTER_MISS;
        int32_t tot_r, tot_m;
        const int32_t pr = base_r + tile_rank(is_r, ws, seq, tot_r);
        const int32_t pm = base_m + tile_rank(is_m, ws, seq, tot_m);
        base_r += tot_r; base_m += tot_m;
        if (i < n) {
            const int32_t s = m >> kSubShift;
            if (i == sub_begin(n, S, s)) { R.off_ret[s] = pr; R.off_mis[s] = pm; }
            if (is_r) copy3(rm + 3 * (size_t)pr, pts + 3 * (size_t)i);
            if (is_m) copy3(rm + 3 * (size_t)(n_ret + pm), pts + 3 * (size_t)i);
            hook[i] = m;
        }
    }
    const int32_t n_mis = base_m;
    __syncthreads();

    // ---- 4. the filtered returns within the range: the cloud the adaptive filter sees, in pts
    int32_t n_in = 0;
    for (int32_t i0 = 0; i0 < n_ret; i0 += kThreads) {
        const int32_t i = i0 + tid;
        double p[3] = {0.0, 0.0, 0.0};
        if (i < n_ret) copy3(p, rm + 3 * (size_t)i);
        const bool f = i < n_ret && in_range(p, P.max_range);
        int32_t tot;
        const int32_t pos = n_in + tile_rank(f, ws, seq, tot);
        n_in += tot;
        if (f) copy3(pts + 3 * (size_t)pos, p);
    }
    __syncthreads();

    // ---- 5. the adaptive search: counts only
    const int32_t slots1 = table_slots(n_in);
    int32_t passes = 0;
    auto count_at = [&](double len, bool trace) -> int32_t {
        for (int32_t h = tid; h < slots1; h += kThreads) table[h] = kEmpty;
        for (int32_t i = tid; i < n_in; i += kThreads) {
            const double p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
            uint64_t key;
            if (!voxel_key(p, len, key)) s_bad = 1;
            keys[i] = key;
        }
        __syncthreads();
        if (s_bad) return -1;
        int32_t claims = 0;
        for (int32_t i = tid; i < n_in; i += kThreads) {
            const uint64_t key = keys[i];
            claims += table_insert(table, (uint32_t)slots1 - 1u, hash_slot(key, 0, slots1), i, key, keys, nullptr);
        }
        const int32_t c = block_sum(claims, ws, seq);
        if (trace) {
            if (tid == 0 && passes < kMaxTrace) { R.trace_length[passes] = len; R.trace_count[passes] = c; }
            ++passes;
        }
        return c;
    };
    double len = 0.0;
    if (P.max_length > 0.0) len = adaptive_search(P.max_length, P.min_points, n_in, [&](double l) { return count_at(l, true); });

    // ---- 6. the match cloud: the search's result once more, this time with its points
    int32_t n_match = n_in;
    if (len > 0.0) {
        const int32_t c = count_at(len, false);
        for (int32_t i = tid; i < n_in; i += kThreads) meta[i] = 0;
        __syncthreads();
        if (c >= 0)
            for (int32_t h = tid; h < slots1; h += kThreads) {
                const int32_t j = table[h];
                if (j != kEmpty) meta[j] = 1;
            }
        __syncthreads();
        n_match = 0;
        for (int32_t i0 = 0; i0 < n_in; i0 += kThreads) {
            const int32_t i = i0 + tid;
            const bool f = i < n_in && meta[i] != 0;
            int32_t tot;
            const int32_t pos = n_match + tile_rank(f, ws, seq, tot);
            n_match += tot;
            if (f) copy3(match + 3 * (size_t)pos, pts + 3 * (size_t)i);
        }
    } else if (len == 0.0) {
        for (int32_t i = tid; i < n_in; i += kThreads) copy3(match + 3 * (size_t)i, pts + 3 * (size_t)i);
    }
    if (tid == 0) {
        if (len < 0.0) {
            R.status = VISFS_BA_ERR_UNSUPPORTED; R.n_returns = R.n_misses = R.n_in_range = R.n_match = R.passes = 0; R.match_length = 0.0;
        } else {
            R.status = VISFS_BA_OK; R.n_returns = n_ret; R.n_misses = n_mis; R.n_in_range = n_in; R.n_match = n_match; R.passes = passes;
            R.match_length = len;
        }
        R.pad0 = R.pad1 = 0;
        R.origin[0] = o[0]; R.origin[1] = o[1]; R.origin[2] = o[2];
    }
}

// ---------------------------------------------------------------- the one-core twin

// The voxel filter over the points idx[0 .. cnt) of `p` ([..][3]) at length len: kept[k] = no earlier point of the list shares the
// voxel.  The number kept, or -1 when a voxel index is out of range.  The table holds keys; any set would do.
int32_t host_filter(const double* p, const int32_t* idx, int32_t cnt, double len, std::vector<uint64_t>& table, uint8_t* kept) {
    const int32_t slots = table_slots(cnt);
    table.assign((size_t)slots, ~0ull);
    int32_t c = 0;
    bool ok = true;
    for (int32_t k = 0; k < cnt; ++k) {
        const int32_t i = idx ? idx[k] : k;
        uint64_t key;
        if (!voxel_key(p + 3 * (size_t)i, len, key)) { ok = false; continue; }
        uint32_t h = hash_slot(key, 0, slots);
        while (table[h] != ~0ull && table[h] != key) h = (h + 1u) & (uint32_t)(slots - 1);
        const bool fresh = table[h] == ~0ull;
        table[h] = key;
        if (kept) kept[k] = fresh;
        c += fresh;
    }
    return ok ? c : -1;
}

void host_scan(const uint8_t* in, uint8_t* out, int32_t b, const KParams& P) {
    const ScanHdr& H = reinterpret_cast<const ScanHdr*>(in)[b];
    DevRec& R = reinterpret_cast<DevRec*>(out)[b];
    const int32_t n = H.n, S = P.pre.num_subdivisions;
    const double* raw = reinterpret_cast<const double*>(in + H.in_pts);
    double* rm = reinterpret_cast<double*>(out + H.out_rm);
    double* match = reinterpret_cast<double*>(out + H.out_match);
    uint8_t* hook = out + H.out_hook;
    std::memset(&R, 0, sizeof R);
    transform_xyz(H.T, H.origin, R.origin);
    auto refuse = [&]() {
        const double o[3] = {R.origin[0], R.origin[1], R.origin[2]};
        std::memset(&R, 0, sizeof R);
        R.status = VISFS_BA_ERR_UNSUPPORTED;
        for (int c = 0; c < 3; ++c) R.origin[c] = o[c];
    };
    std::vector<double> pts(3 * (size_t)n + 3);
    std::vector<uint8_t> meta((size_t)n + 1), kept((size_t)n + 1);
    std::vector<int32_t> idx((size_t)n + 1);
    std::vector<uint64_t> table;
    for (int32_t i = 0; i < n; ++i) {
        double q[3];
        transform_xyz(H.T, raw + 3 * (size_t)i, q);
        const int cls = classify(P.pre, R.origin, q, pts.data() + 3 * (size_t)i);
        meta[(size_t)i] = (uint8_t)(cls | (sub_of(n, S, i) << kSubShift));
        if (cls != VISFS_SCAN_FILTER_DROPPED && !(P.voxel_size > 0.0)) meta[(size_t)i] |= kKept;
    }
    if (P.voxel_size > 0.0)
        for (int32_t s = 0; s < S; ++s)
            for (int cls = VISFS_SCAN_FILTER_RETURN; cls <= VISFS_SCAN_FILTER_MISS; ++cls) {
                int32_t cnt = 0;
                for (int32_t i = sub_begin(n, S, s); i < sub_begin(n, S, s + 1); ++i)
                    if ((meta[(size_t)i] & kClassMask) == cls) idx[(size_t)cnt++] = i;
                if (host_filter(pts.data(), idx.data(), cnt, P.voxel_size, table, kept.data()) < 0) return refuse();
                for (int32_t k = 0; k < cnt; ++k) if (kept[(size_t)k]) meta[(size_t)idx[(size_t)k]] |= kKept;
            }
    int32_t n_ret = 0, n_mis = 0;
    for (int32_t i = 0; i < n; ++i) n_ret += (meta[(size_t)i] & kKept) && (meta[(size_t)i] & kClassMask) == VISFS_SCAN_FILTER_RETURN;
    int32_t pr = 0;
    for (int32_t i = 0; i < n; ++i) {
        const uint8_t m = meta[(size_t)i];
        const int32_t s = m >> kSubShift;
        if (i == sub_begin(n, S, s)) { R.off_ret[s] = pr; R.off_mis[s] = n_mis; }
        if (m & kKept) {
            if ((m & kClassMask) == VISFS_SCAN_FILTER_RETURN) { for (int c = 0; c < 3; ++c) rm[3 * (size_t)pr + c] = pts[3 * (size_t)i + c]; ++pr; }
            else { for (int c = 0; c < 3; ++c) rm[3 * (size_t)(n_ret + n_mis) + c] = pts[3 * (size_t)i + c]; ++n_mis; }
        }
        hook[i] = m;
    }
    int32_t n_in = 0;
    for (int32_t i = 0; i < n_ret; ++i)
        if (in_range(rm + 3 * (size_t)i, P.max_range)) { for (int c = 0; c < 3; ++c) pts[3 * (size_t)n_in + c] = rm[3 * (size_t)i + c]; ++n_in; }
    int32_t passes = 0;
    double len = 0.0;
    if (P.max_length > 0.0)
        len = adaptive_search(P.max_length, P.min_points, n_in, [&](double l) -> int32_t {
            const int32_t c = host_filter(pts.data(), nullptr, n_in, l, table, nullptr);
            if (c < 0) return -1;
            if (passes < kMaxTrace) { R.trace_length[passes] = l; R.trace_count[passes] = c; }
            ++passes;
            return c;
        });
    if (len < 0.0) return refuse();
    int32_t n_match = n_in;
    if (len > 0.0) {
        if (host_filter(pts.data(), nullptr, n_in, len, table, kept.data()) < 0) return refuse();
        n_match = 0;
        for (int32_t i = 0; i < n_in; ++i)
            if (kept[(size_t)i]) { for (int c = 0; c < 3; ++c) match[3 * (size_t)n_match + c] = pts[3 * (size_t)i + c]; ++n_match; }
    } else {
        for (int32_t i = 0; i < 3 * n_in; ++i) match[i] = pts[(size_t)i];
    }
    R.status = VISFS_BA_OK; R.n_returns = n_ret; R.n_misses = n_mis; R.n_in_range = n_in; R.n_match = n_match; R.passes = passes;
    R.match_length = len;
}

}  // namespace sfilt

struct visfs_scan_filter {
    bool device = false;
    int dev = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // the last successful call
    int32_t m = 0, S = 1;
    std::vector<ScanHdr> hdr;
    std::vector<visfs_scan_filter_record> recs;
    std::vector<uint8_t> h_in_v, h_out_v;         // twin
    Staged<uint8_t> in, res;                      // device: a call's scans and its results, bytes
    DeviceBuf<uint8_t> d_work;
    host::Counts counts;
    const uint8_t* out() const { return device ? res.h.get() : h_out_v.data(); }

    ~visfs_scan_filter() {                        // before the members free what they own
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

size_t pad8(size_t v) { return (v + 7) & ~(size_t)7; }

// Room for the call's three blocks; growing a block drops the results that lay in it.
int device_room(visfs_scan_filter* f, size_t in_bytes, size_t out_bytes, size_t work_bytes) {
    HIP_TRY(f, hipSetDevice(f->dev));
    RC_TRY(f->in.reserve(f, in_bytes, in_bytes));
    if (f->res.cap() < out_bytes) f->m = 0;
    RC_TRY(f->res.reserve(f, out_bytes, out_bytes));
    return f->d_work.grow(f, work_bytes);
}

bool finite_n(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// The public record of scan b from what its workgroup (or the twin) left.
visfs_scan_filter_record record_from(const DevRec& R, const ScanHdr& H, int32_t S) {
    visfs_scan_filter_record r;
    std::memset(&r, 0, sizeof r);
    r.status = R.status;
    if (R.status != VISFS_BA_OK) return r;
    for (int32_t s = 0; s < S; ++s) r.n_range_data += sub_begin(H.n, S, s) != sub_begin(H.n, S, s + 1);
    r.n_returns = R.n_returns; r.n_misses = R.n_misses; r.n_in_range = R.n_in_range; r.n_match = R.n_match; r.passes = R.passes;
    r.match_length = R.match_length;
    return r;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_scan_filter_abi_version(void) { return VISFS_SCAN_FILTER_ABI_VERSION; }

void visfs_scan_filter_default_params(visfs_scan_filter_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    visfs_scan_pretreat_default_params(&p->pretreat);
    p->voxel_size = 0.025;
    p->adaptive_max_length = 0.5;
    p->adaptive_min_num_points = 200;
    p->adaptive_max_range = 50.0;
}

int visfs_scan_filter_create(visfs_ba_handle* h, visfs_scan_filter** out) {
    if (!out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(nullptr, [&]() -> int {
        visfs_scan_filter* f = new visfs_scan_filter();
        if (h) { f->device = true; f->dev = visfs_internal_device(h); f->stream = visfs_internal_stream(h); }
        *out = f;
        return (int)VISFS_BA_OK;
    });
}

void visfs_scan_filter_destroy(visfs_scan_filter* f) { delete f; }

const char* visfs_scan_filter_last_error(const visfs_scan_filter* f) { return f ? f->err.c_str() : "null filter"; }

int visfs_scan_filter_process(visfs_scan_filter* f, const visfs_scan_filter_params* p, int32_t m, const visfs_scan_filter_scan* scans,
                              visfs_scan_filter_record* records) {
    if (!f || !p || m < 0 || (m > 0 && !scans)) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        // ---- every refusal, before anything is touched
        if (p->pretreat.num_subdivisions < 1) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "num_subdivisions must be at least 1");
        if (!(p->voxel_size >= 0.0) || !(p->adaptive_max_length >= 0.0) || !(p->adaptive_max_range >= 0.0) || !std::isfinite(p->voxel_size) ||
            !std::isfinite(p->adaptive_max_length) || !std::isfinite(p->adaptive_max_range))
            return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "voxel_size, adaptive_max_length and adaptive_max_range must be finite and not negative");
        if (p->adaptive_min_num_points < 0) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "adaptive_min_num_points must not be negative");
        if (m > VISFS_SCAN_FILTER_MAX_SCANS) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "more than 64 scans");
        if (p->pretreat.num_subdivisions > VISFS_SCAN_FILTER_MAX_SUBDIVISIONS) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "more than 16 subdivisions");
        for (int32_t b = 0; b < m; ++b) {
            if (scans[b].n < 0 || (scans[b].n > 0 && !scans[b].points_xyz)) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "a scan without points");
            if (scans[b].n > VISFS_SCAN_FILTER_MAX_POINTS) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "a scan of more than 16384 points");
        }
        for (int32_t b = 0; b < m; ++b)
            if (!finite_n(scans[b].T_laser_to_camera, 12) || !finite_n(scans[b].origin, 3) || !finite_n(scans[b].points_xyz, 3 * (size_t)scans[b].n))
                return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "a point, transform or origin is not finite");

        // ---- the layout of the three blocks
        std::vector<ScanHdr> hdr((size_t)m);
        size_t in_bytes = pad8((size_t)m * sizeof(ScanHdr)), out_bytes = pad8((size_t)m * sizeof(DevRec)), work_bytes = 0;
        for (int32_t b = 0; b < m; ++b) {
            ScanHdr& H = hdr[(size_t)b];
            std::memset(&H, 0, sizeof H);
            std::memcpy(H.T, scans[b].T_laser_to_camera, sizeof H.T);
            std::memcpy(H.origin, scans[b].origin, sizeof H.origin);
            H.n = scans[b].n;
            const size_t n = (size_t)H.n;
            H.in_pts = (int64_t)in_bytes; in_bytes += 24 * n;
            H.out_rm = (int64_t)out_bytes; out_bytes += 24 * n;
            H.out_match = (int64_t)out_bytes; out_bytes += 24 * n;
            H.out_hook = (int64_t)out_bytes; out_bytes += pad8(n);
            H.work_pts = (int64_t)work_bytes; work_bytes += 24 * n;
            H.work_keys = (int64_t)work_bytes; work_bytes += 8 * n;
        }
        KParams K;
        std::memset(&K, 0, sizeof K);
        K.pre = p->pretreat; K.voxel_size = p->voxel_size; K.max_length = p->adaptive_max_length; K.max_range = p->adaptive_max_range;
        K.min_points = p->adaptive_min_num_points;

        uint8_t* in;
        uint8_t* out;
        if (f->device) {
            if (m > 0) { const int rc = device_room(f, in_bytes, out_bytes, work_bytes ? work_bytes : 8); if (rc != VISFS_BA_OK) return rc; }
            in = f->in.h.get(); out = f->res.h.get();
        } else {
            f->h_in_v.resize(in_bytes); f->h_out_v.resize(out_bytes);
            in = f->h_in_v.data(); out = f->h_out_v.data();
        }
        f->m = 0;                                                               // the last results are being overwritten from here on
        f->counts = {};
        if (m > 0) {
            std::memcpy(in, hdr.data(), (size_t)m * sizeof(ScanHdr));
            for (int32_t b = 0; b < m; ++b)
                if (hdr[(size_t)b].n) std::memcpy(in + hdr[(size_t)b].in_pts, scans[b].points_xyz, 24 * (size_t)hdr[(size_t)b].n);
            if (f->device) {
                HIP_TRY(f, hipMemcpyAsync(f->in.d.get(), in, in_bytes, hipMemcpyHostToDevice, f->stream));
                hipLaunchKernelGGL(k_scan_filter, dim3((unsigned)m), dim3(kThreads), 0, f->stream, f->in.d.get(), f->res.d.get(), f->d_work.get(), K);
                HIP_TRY(f, hipGetLastError());
                HIP_TRY(f, hipMemcpyAsync(out, f->res.d.get(), out_bytes, hipMemcpyDeviceToHost, f->stream));
                HIP_TRY(f, hipStreamSynchronize(f->stream));
                f->counts = { 1, 2, 1 };
            } else {
                for (int32_t b = 0; b < m; ++b) host_scan(in, out, b, K);
            }
        }
        f->recs.resize((size_t)m);
        for (int32_t b = 0; b < m; ++b) {
            f->recs[(size_t)b] = record_from(reinterpret_cast<const DevRec*>(out)[b], hdr[(size_t)b], K.pre.num_subdivisions);
            if (records) records[b] = f->recs[(size_t)b];
        }
        f->hdr.swap(hdr);
        f->S = K.pre.num_subdivisions;
        f->m = m;
        return (int)VISFS_BA_OK;
    });
}

int visfs_scan_filter_num_scans(const visfs_scan_filter* f, int32_t* m) {
    if (!f || !m) return VISFS_BA_ERR_BAD_ARGUMENT;
    *m = f->m;
    return VISFS_BA_OK;
}

int visfs_scan_filter_record_of(const visfs_scan_filter* f, int32_t scan, visfs_scan_filter_record* record) {
    if (!f || !record || scan < 0 || scan >= f->m) return VISFS_BA_ERR_BAD_ARGUMENT;
    *record = f->recs[(size_t)scan];
    return VISFS_BA_OK;
}

int visfs_scan_filter_range_data(const visfs_scan_filter* f, int32_t scan, int32_t cap, visfs_range_data* rd_out, int32_t* n_out) {
    if (!f || !n_out || cap < 0 || (cap > 0 && !rd_out) || scan < 0 || scan >= f->m) return VISFS_BA_ERR_BAD_ARGUMENT;
    const visfs_scan_filter_record& r = f->recs[(size_t)scan];
    *n_out = r.n_range_data;
    if (r.status != VISFS_BA_OK) return VISFS_BA_OK;
    const ScanHdr& H = f->hdr[(size_t)scan];
    const DevRec& R = reinterpret_cast<const DevRec*>(f->out())[scan];
    const double* rm = reinterpret_cast<const double*>(f->out() + H.out_rm);
    int32_t k = 0, prev = -1;
    visfs_range_data last;
    std::memset(&last, 0, sizeof last);
    for (int32_t s = 0; s <= f->S; ++s) {
        if (s < f->S && sub_begin(H.n, f->S, s) == sub_begin(H.n, f->S, s + 1)) continue;
        const int32_t at_r = s < f->S ? R.off_ret[s] : R.n_returns, at_m = s < f->S ? R.off_mis[s] : R.n_misses;
        if (prev >= 0) {
            last.n_returns = at_r - R.off_ret[prev]; last.n_misses = at_m - R.off_mis[prev];
            if (k < cap) rd_out[k] = last;
            ++k;
        }
        if (s == f->S) break;
        for (int c = 0; c < 3; ++c) last.origin[c] = R.origin[c];
        last.returns = rm + 3 * (size_t)at_r;
        last.misses = rm + 3 * ((size_t)R.n_returns + (size_t)at_m);
        prev = s;
    }
    return VISFS_BA_OK;
}

int visfs_scan_filter_match_cloud(const visfs_scan_filter* f, int32_t scan, const double** xyz, int32_t* n) {
    if (!f || !xyz || !n || scan < 0 || scan >= f->m) return VISFS_BA_ERR_BAD_ARGUMENT;
    const visfs_scan_filter_record& r = f->recs[(size_t)scan];
    *n = r.n_match;
    *xyz = r.n_match ? reinterpret_cast<const double*>(f->out() + f->hdr[(size_t)scan].out_match) : nullptr;
    return VISFS_BA_OK;
}

int visfs_scan_filter_download(const visfs_scan_filter* f, int32_t scan, uint8_t* point_class, uint8_t* subdivision, uint8_t* kept,
                               double* trace_length, int32_t* trace_count, int32_t* n_trace) {
    if (!f || scan < 0 || scan >= f->m) return VISFS_BA_ERR_BAD_ARGUMENT;
    const visfs_scan_filter_record& r = f->recs[(size_t)scan];
    const ScanHdr& H = f->hdr[(size_t)scan];
    const DevRec& R = reinterpret_cast<const DevRec*>(f->out())[scan];
    const uint8_t* hook = f->out() + H.out_hook;
    const bool ok = r.status == VISFS_BA_OK;
    for (int32_t i = 0; i < H.n; ++i) {
        const uint8_t m = ok ? hook[i] : (uint8_t)0;
        if (point_class) point_class[i] = m & kClassMask;
        if (subdivision) subdivision[i] = (uint8_t)(m >> kSubShift);
        if (kept) kept[i] = (m & kKept) ? 1 : 0;
    }
    const int32_t nt = ok ? (r.passes < kMaxTrace ? r.passes : kMaxTrace) : 0;
    for (int32_t k = 0; k < kMaxTrace; ++k) {
        if (trace_length) trace_length[k] = k < nt ? R.trace_length[k] : 0.0;
        if (trace_count) trace_count[k] = k < nt ? R.trace_count[k] : 0;
    }
    if (n_trace) *n_trace = nt;
    return VISFS_BA_OK;
}

int visfs_scan_filter_hook_slot(const int32_t voxel[3], int32_t list, int32_t count, int32_t* slots, int32_t* slot) {
    if (!voxel || count < 0 || count > VISFS_SCAN_FILTER_MAX_POINTS || list < 0 || list >= 2 * VISFS_SCAN_FILTER_MAX_SUBDIVISIONS) return VISFS_BA_ERR_BAD_ARGUMENT;
    uint64_t key = 0;
    for (int c = 0; c < 3; ++c) {
        if (voxel[c] < -VISFS_SCAN_FILTER_MAX_VOXEL || voxel[c] > VISFS_SCAN_FILTER_MAX_VOXEL) return VISFS_BA_ERR_UNSUPPORTED;
        key |= (uint64_t)((int64_t)voxel[c] + 1048576) << (21 * c);
    }
    const int32_t s = table_slots(count);
    if (slots) *slots = s;
    if (slot) *slot = (int32_t)hash_slot(key, list, s);
    return VISFS_BA_OK;
}

int visfs_scan_filter_last_counts(const visfs_scan_filter* f, int32_t* launches, int32_t* copies, int32_t* waits) {
    return f ? f->counts.read(launches, copies, waits) : (int)VISFS_BA_ERR_BAD_ARGUMENT;
}

}  // extern "C"
