// KLD-adaptive particle counts of the Monte-Carlo localiser (include/visfs_mcl_kld.h).
//
// A KLD update is the update of ba_mcl.hip on the n active particles (k_mcl_weight, k_mcl_sums, k_mcl_finish with N = n), and
//   k_mcl_kld_resample  in k_mcl_resample's place: one workgroup of 1024.  It returns at once when the flag is clear; else it scans
//                   the workgroup totals of k_mcl_finish, clears an open-addressed table of draw indices in LDS (two slots per
//                   draw), runs the `cap` draws (their ancestors by two binary searches, their bins), inserts every draw (a slot
//                   is claimed by compare-and-swap and lowered by an atomic minimum, so it ends at the lowest draw of its bin
//                   whatever the schedule), counts the bins in draw order by ballots, takes the stop n* by an integer minimum and
//                   copies the n* ancestors into the other buffer at stride n*.
// Integer LDS atomics only; no work item waits for another (a probe ends because the table is never full).  The one-core twin runs
// the definition's sequential loop with a std::set of bins.
// On a filter with hypotheses (include/visfs_mcl_hyp.h) the launch is the kernel's second instantiation,
// which clusters the new set's bins behind step 7 (hyp_tail of ba_mcl_hyp.hpp); the first is the kernel as it was.
#include "ba_mcl_state.hpp"
#include "ba_mcl_kld.hpp"
#include "ba_mcl_hyp.hpp"
#include "ba_host.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <new>
#include <set>

#pragma clang fp contract(off)

using namespace mcl;
using namespace host;

namespace mcl {

struct Hyp;

struct Kld {
    visfs_mcl_kld_params p;
    std::vector<int32_t> h_limit;             // [N + 1], both flavours
    int32_t hash_bits = -1;                   // -1: the table's full width
    DeviceBuf<int32_t> d_limit;
    DeviceBuf<int32_t> d_work;                // [5 N]
    DeviceBuf<KldRec> d_rec;
    PinnedBuf<KldRec> h_rec;                  // pinned
    int32_t pending[3] = { 0, 0, 0 };         // n_after, bins, limit of the update that is running
    visfs_mcl_kld_result last;
    bool have_last = false;
    Hyp* hyp = nullptr;                       // null: no hypotheses (include/visfs_mcl_hyp.h)
};

// The hypotheses of section 9v on a KLD filter.
struct Hyp {
    DeviceBuf<int32_t> d_work;                // [kHypWorkInts N]
    DeviceBuf<double> d_cs;                   // [2 N]
    DeviceBuf<HypRec> d_rec;                  // takes the place of Kld::d_rec
    PinnedBuf<HypRec> h_rec;                  // pinned
    HypBlock pending;                         // of the update that is running
    std::vector<int32_t> h_label;             // the twin's labels of the last resampling
    visfs_mcl_hyp_result last;                // all zero while there are none
    int32_t rounds = 0;
};

__device__ inline uint64_t shfl_up64(uint64_t v, int d) {
    const int lo = __shfl_up((int)(uint32_t)(v & 0xFFFFFFFFull), d), hi = __shfl_up((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo;
}

// Draw i of bin (b[0], b[1], b[2]) enters the table from slot h; returns the slot of its bin.  A slot only ever holds draws of one
// bin, and every draw of a bin walks the same chain past the same other bins, so a bin has one slot.
__device__ inline uint32_t kld_insert(int32_t* table, uint32_t mask, uint32_t h, int32_t i, const int32_t* b, const int32_t* bins) {
    for (;;) {
        int32_t j = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (j == kKldEmpty) {
            j = atomicCAS(&table[h], kKldEmpty, i);
            if (j == kKldEmpty) return h;
        }
        const int32_t* o = bins + 3 * (size_t)j;
        if (o[0] == b[0] && o[1] == b[1] && o[2] == b[2]) {
            if (i < j) atomicMin(&table[h], i);
            return h;
        }
        h = (h + 1u) & mask;
    }
}

// Two instantiations: <false> is the KLD resampling alone; <true> adds the hypotheses of section 9v (ba_mcl_hyp.hpp) behind the new
// set, and its rec is the head of a HypRec.
template <bool HYP>
__global__ __launch_bounds__(kKldThreads) void k_mcl_kld_resample(const Hdr* __restrict__ up, KldRec* __restrict__ rec, const double* __restrict__ st,
                                                                  double* __restrict__ out, const uint64_t* __restrict__ C,
                                                                  const uint64_t* __restrict__ bsum, int32_t blocks, int32_t* __restrict__ anc, KldArgs A,
                                                                  HypArgs G) {
    __shared__ int32_t table[kKldMaxSlots];
    __shared__ uint64_t sc[kKldMaxBlocks];                                 // the exclusive offsets of k_mcl_finish's workgroups
    __shared__ uint64_t s_K;
    __shared__ int32_t ws[2 * kKldWaves];
    __shared__ int32_t s_stop;
    if (rec->r.resampled == 0) return;                                     // the same in every work item, and before every barrier
    const Hdr& H = *up;
    const int32_t n = H.N, cap = A.cap, tid = (int32_t)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* w_anc = A.work;
    int32_t* w_slot = A.work + (size_t)cap;
    int32_t* w_bin = A.work + 2 * (size_t)cap;

    // ---- 1. the scan of the workgroup totals (at most 64: one wavefront), 2. the empty table
    if (wave == 0) {
        const uint64_t v = lane < blocks ? bsum[lane] : 0;
        uint64_t inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t a = shfl_up64(inc, d);
            if (lane >= d) inc += a;
        }
        sc[lane] = inc - v;
        if (lane == 63) s_K = inc;
    }
    for (int32_t h = tid; h < A.slots; h += kKldThreads) table[h] = kKldEmpty;
    if (tid == 0) s_stop = cap;
    __syncthreads();
    const uint64_t K = s_K;
    if (K == 0) {                                                          // cannot happen with normalised weights; never divide by it
        if (tid == 0) rec->r.resampled = 0;
        return;
    }

    // ---- 3. the draws: the ancestor and its bin
    for (int32_t i = tid; i < cap; i += kKldThreads) {
        const uint64_t u = key(H.seed, H.update, (uint64_t)i, kKldDraw) % K;
        int32_t lo = 0, hi = blocks - 1;                                   // the last workgroup whose offset is at most u
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (sc[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const uint64_t base = sc[lo];
        int32_t l = lo * kThreads, h = l + kThreads - 1;
        if (h > n - 1) h = n - 1;
        while (l < h) {                                                    // ... and its last particle whose prefix is at most u
            const int32_t mid = (l + h + 1) >> 1;
            if (base + C[mid] <= u) l = mid; else h = mid - 1;
        }
        w_anc[i] = l;
        w_bin[3 * (size_t)i] = bin_of(st[l], A.bin_xy);
        w_bin[3 * (size_t)i + 1] = bin_of(st[(size_t)n + l], A.bin_xy);
        w_bin[3 * (size_t)i + 2] = bin_of(st[2 * (size_t)n + l], A.bin_yaw);
    }
    __syncthreads();                                                       // every draw's bin is written before any is compared

    // ---- 4. the table: every slot ends at the lowest draw of its bin
    const uint32_t mask = (uint32_t)A.slots - 1u;
    for (int32_t i = tid; i < cap; i += kKldThreads) {
        const int32_t b[3] = { w_bin[3 * (size_t)i], w_bin[3 * (size_t)i + 1], w_bin[3 * (size_t)i + 2] };
        const uint32_t home = (uint32_t)bin_hash(b[0], b[1], b[2]) & (uint32_t)A.home_mask;
        w_slot[i] = (int32_t)kld_insert(table, mask, home, i, b, w_bin);
    }
    __syncthreads();

    // ---- 5. first_i and its prefix k in draw order, 6. the stop: the smallest m = i + 1 above limit[k_m]
    int32_t k_base = 0, cand_m = 0, cand_k = 0;
    for (int32_t r = 0; r * kKldThreads < cap; ++r) {
        const int32_t i = r * kKldThreads + tid;
        const bool first = i < cap && table[w_slot[i]] == i;
        const unsigned long long bal = __ballot(first);
        int32_t* w = ws + (r & 1) * kKldWaves;                             // two buffers in turn: one barrier a round suffices
        if (lane == 0) w[wave] = __popcll(bal);
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int q = 0; q < kKldWaves; ++q) {
            const int32_t v = w[q];
            total += v;
            if (q < wave) before += v;
        }
        const int32_t k = k_base + before + __popcll(bal & ((2ull << lane) - 1ull));     // the bins among the draws 0 .. i
        k_base += total;
        if (i < cap && cand_m == 0) {
            const bool over = i + 1 > A.limit[k];
            if (over || i == cap - 1) { cand_m = i + 1; cand_k = k; }
            if (over) atomicMin(&s_stop, i + 1);
        }
    }
    __syncthreads();
    const int32_t n_new = s_stop;                                          // cap when no draw count exceeded its limit
    if (cand_m == n_new) {                                                 // one work item: the draw the loop stopped at
        rec->n_after = n_new; rec->bins = cand_k; rec->limit = A.limit[cand_k]; rec->pad = 0;
        rec->r.K = K;
    }

    // ---- 7. the new set, packed at stride n*
    const double inv = 1.0 / (double)n_new;
    for (int32_t i = tid; i < n_new; i += kKldThreads) {
        const int32_t a = w_anc[i];
        out[i] = st[a]; out[(size_t)n_new + i] = st[(size_t)n + a]; out[2 * (size_t)n_new + i] = st[2 * (size_t)n + a];
        out[3 * (size_t)n_new + i] = inv;
        anc[i] = a;
    }
    if constexpr (HYP) {
        __shared__ int32_t s_bins;
        if (cand_m == n_new) s_bins = cand_k;                              // the bins of the new set, from the one work item that knows
        __syncthreads();                                                   // ... and the new set is written before its poses are read
        hyp_tail(table, mask, (uint32_t)A.home_mask, w_slot, w_bin, n_new, s_bins, cap, out, G, &reinterpret_cast<HypRec*>(rec)->h);
    }
}

// Waits for the stream, then the members of the Kld and of its Hyp free what they own.
void kld_free(visfs_mcl* f) {
    Kld* k = f->kld;
    if (!k) return;
    if (f->device) {
        (void)hipSetDevice(f->dev);
        if (f->stream) (void)hipStreamSynchronize(f->stream);
    }
    delete k->hyp;
    delete k;
    f->kld = nullptr;
}

Rec* kld_device_rec(visfs_mcl* f) { return f->kld->hyp ? &f->kld->hyp->d_rec->k.r : &f->kld->d_rec->r; }

void kld_particles_replaced(visfs_mcl* f) {
    Hyp* h = f->kld->hyp;
    if (!h) return;
    std::memset(&h->last, 0, sizeof h->last);
    h->rounds = 0;
}

int kld_device_resample(visfs_mcl* f, const Hdr* up, const double* st, double* out, int32_t blocks, Rec& rec) {
    Kld* k = f->kld;
    KldArgs A;
    std::memset(&A, 0, sizeof A);
    A.bin_xy = k->p.bin_xy; A.bin_yaw = k->p.bin_yaw;
    A.limit = k->d_limit.get(); A.work = k->d_work.get();
    A.cap = f->N; A.slots = kld_slots(f->N);
    int32_t width = 0;
    while ((1 << width) < A.slots) ++width;
    const int32_t bits = k->hash_bits < 0 || k->hash_bits > width ? width : k->hash_bits;
    A.home_mask = (int32_t)((1u << bits) - 1u);
    Hyp* h = k->hyp;                                                       // the same launch with the hypotheses; their block comes down behind KldRec
    HypArgs G = HypArgs();
    if (h) { G.work = h->d_work.get(); G.cs = h->d_cs.get(); }
    const auto kernel = h ? k_mcl_kld_resample<true> : k_mcl_kld_resample<false>;
    KldRec* d_rec = h ? &h->d_rec->k : k->d_rec.get();
    KldRec* h_rec = h ? &h->h_rec->k : k->h_rec.get();
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kKldThreads), 0, f->stream, up, d_rec, st, out, f->d_C.get(), f->d_bsum.get(), blocks, f->d_anc.get(), A, G);
    HIP_TRY(f, hipGetLastError());
    HIP_TRY(f, hipMemcpyAsync(h_rec, d_rec, h ? sizeof(HypRec) : sizeof(KldRec), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    rec = h_rec->r;
    k->pending[0] = h_rec->n_after; k->pending[1] = h_rec->bins; k->pending[2] = h_rec->limit;
    if (h) h->pending = h->h_rec->h;
    return VISFS_BA_OK;
}

void kld_host_resample(visfs_mcl* f, const Hdr& H, const std::vector<uint64_t>& C, Rec& rec) {
    Kld* k = f->kld;
    const size_t n = (size_t)H.N;
    const int32_t cap = f->N;
    const uint64_t K = C[n];
    const double *X = f->h_st[f->cur].data(), *Y = X + n, *A = Y + n;
    std::set<std::array<int32_t, 3>> seen;
    std::vector<int32_t> a_of;
    int32_t bins = 0, m = 0;
    for (int32_t i = 0; i < cap; ++i) {                                    // AMCL's loop: draw, insert, stop once the count exceeds the limit
        const uint64_t u = key(H.seed, H.update, (uint64_t)i, kKldDraw) % K;
        const size_t a = (size_t)(std::upper_bound(C.begin(), C.begin() + (ptrdiff_t)n, u) - C.begin()) - 1;   // the last a with C_a <= u
        if (seen.insert({ bin_of(X[a], k->p.bin_xy), bin_of(Y[a], k->p.bin_xy), bin_of(A[a], k->p.bin_yaw) }).second) ++bins;
        a_of.push_back((int32_t)a);
        m = i + 1;
        if (m > k->h_limit[(size_t)bins]) break;
    }
    const size_t ns = (size_t)m;
    const double inv = 1.0 / (double)m;
    std::vector<double>& out = f->h_st[f->cur ^ 1];
    for (size_t i = 0; i < ns; ++i) {
        const size_t a = (size_t)a_of[i];
        out[i] = X[a]; out[ns + i] = Y[a]; out[2 * ns + i] = A[a]; out[3 * ns + i] = inv;
        f->h_anc[i] = (int32_t)a;
    }
    rec.K = K; rec.r0 = 0;
    k->pending[0] = m; k->pending[1] = bins; k->pending[2] = k->h_limit[(size_t)bins];
    if (Hyp* h = k->hyp) hyp_host(out.data(), out.data() + ns, out.data() + 2 * ns, m, k->p.bin_xy, k->p.bin_yaw, h->h_label, h->pending);
}

void kld_commit(visfs_mcl* f, const Rec& rec, int32_t n_before) {
    Kld* k = f->kld;
    k->last.n_before = n_before;
    if (rec.resampled) {
        k->last.n_after = k->pending[0]; k->last.bins = k->pending[1]; k->last.limit = k->pending[2];
        f->n = k->pending[0];
        if (Hyp* h = k->hyp) {
            hyp_finish(h->pending, k->pending[0], f->update, h->last);
            h->rounds = h->pending.rounds;
        }
    } else {
        if (k->hyp) k->hyp->last.fresh = 0;                                // the last hypotheses stay readable
        k->last.n_after = n_before; k->last.bins = 0; k->last.limit = 0;
    }
    k->have_last = true;
}

}  // namespace mcl

// ====================================================================== exported C ABI
extern "C" {

int visfs_mcl_kld_abi_version(void) { return VISFS_MCL_KLD_ABI_VERSION; }

void visfs_mcl_kld_default_params(visfs_mcl_kld_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->min_particles = 100; p->kld_err = 0.01; p->kld_z = 0.99;
    p->bin_xy = 0.5; p->bin_yaw = kPi / 18.0;
}

int visfs_mcl_kld_enable(visfs_mcl* f, const visfs_mcl_kld_params* p) {
    if (!f || !p) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(f, [&]() -> int {
        if (p->min_particles < 1 || p->min_particles > f->N) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "min_particles must lie in 1 .. N");
        if (!finite_pos(p->kld_err) || !finite_pos(p->kld_z) || !finite_pos(p->bin_xy) || !finite_pos(p->bin_yaw) || !(p->kld_err < 1.0))
            return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "kld_err, kld_z, bin_xy and bin_yaw must be finite and positive, kld_err below 1");
        if (f->N > VISFS_MCL_KLD_MAX_PARTICLES) return fail(f, VISFS_BA_ERR_UNSUPPORTED, "a KLD filter holds at most 16384 particles");
        std::vector<int32_t> limit;
        kld_limits(*p, f->N, limit);
        Kld* k = f->kld;
        const bool fresh = k == nullptr;
        if (fresh) k = new Kld();
        auto push = [&]() -> int {
            if (!f->device) return (int)VISFS_BA_OK;
            const size_t N = (size_t)f->N;
            HIP_TRY(f, hipSetDevice(f->dev));
            if (fresh) {
                RC_TRY(k->d_limit.alloc(f, N + 1));
                RC_TRY(k->d_work.alloc(f, 5 * N));
                RC_TRY(k->d_rec.alloc(f, 1));
                RC_TRY(k->h_rec.alloc(f, 1));
            }
            HIP_TRY(f, hipMemcpyAsync(k->d_limit.get(), limit.data(), (N + 1) * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
            HIP_TRY(f, hipStreamSynchronize(f->stream));                               // `limit` is pageable and leaves scope
            return (int)VISFS_BA_OK;
        };
        const int rc = push();
        if (rc != VISFS_BA_OK) {
            if (fresh) { f->kld = k; kld_free(f); }
            return rc;
        }
        k->p = *p;
        k->h_limit.swap(limit);
        f->kld = k;
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_kld_last(const visfs_mcl* f, visfs_mcl_kld_result* r) {
    if (!f || !r) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld || !f->kld->have_last) { std::memset(r, 0, sizeof *r); return VISFS_BA_ERR_BAD_ARGUMENT; }
    *r = f->kld->last;
    return VISFS_BA_OK;
}

int32_t visfs_mcl_kld_count(const visfs_mcl* f) { return f ? f->n : 0; }

int visfs_mcl_kld_upload(visfs_mcl* f, int32_t n, const double* x, const double* y, const double* yaw, const double* w) {
    if (!f || !x || !y || !yaw || !w) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the filter is no KLD filter");
    if (n < 1 || n > f->N) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the count must lie in 1 .. N");
    return upload_n(f, n, x, y, yaw, w);
}

int visfs_mcl_kld_limits(visfs_mcl* f, int32_t* limit) {
    if (!f || !limit) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the filter is no KLD filter");
    return guarded(f, [&]() -> int {
        const size_t bytes = ((size_t)f->N + 1) * sizeof(int32_t);
        if (!f->device) { std::memcpy(limit, f->kld->h_limit.data(), bytes); return (int)VISFS_BA_OK; }
        HIP_TRY(f, hipSetDevice(f->dev));                                              // what the device holds, not the host's copy
        HIP_TRY(f, hipMemcpyAsync(limit, f->kld->d_limit.get(), bytes, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_kld_hook_set_hash_bits(visfs_mcl* f, int32_t bits) {
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the filter is no KLD filter");
    if (bits < -1) return VISFS_BA_ERR_BAD_ARGUMENT;
    f->kld->hash_bits = bits;
    return VISFS_BA_OK;
}

// ---------------------------------------------------------------------- include/visfs_mcl_hyp.h
int visfs_mcl_hyp_abi_version(void) { return VISFS_MCL_HYP_ABI_VERSION; }

int visfs_mcl_hyp_enable(visfs_mcl* f) {
    if (!f) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "the filter is no KLD filter");
    if (f->kld->hyp) return VISFS_BA_OK;
    return guarded(f, [&]() -> int {
        Hyp* h = new Hyp();
        std::memset(&h->pending, 0, sizeof h->pending);
        std::memset(&h->last, 0, sizeof h->last);
        auto push = [&]() -> int {
            if (!f->device) return (int)VISFS_BA_OK;
            const size_t N = (size_t)f->N;
            HIP_TRY(f, hipSetDevice(f->dev));
            RC_TRY(h->d_work.alloc(f, (size_t)kHypWorkInts * N));
            RC_TRY(h->d_cs.alloc(f, 2 * N));
            RC_TRY(h->d_rec.alloc(f, 1));
            RC_TRY(h->h_rec.alloc(f, 1));
            HIP_TRY(f, hipMemsetAsync(h->d_rec.get(), 0, sizeof(HypRec), f->stream));
            HIP_TRY(f, hipStreamSynchronize(f->stream));
            return (int)VISFS_BA_OK;
        };
        const int rc = push();
        if (rc != VISFS_BA_OK) { delete h; return rc; }
        f->kld->hyp = h;
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_hyp_last(const visfs_mcl* f, visfs_mcl_hyp_result* r) {
    if (!f || !r) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld || !f->kld->hyp) { std::memset(r, 0, sizeof *r); return VISFS_BA_ERR_BAD_ARGUMENT; }
    *r = f->kld->hyp->last;
    return VISFS_BA_OK;
}

int visfs_mcl_hyp_download_labels(visfs_mcl* f, int32_t* label) {
    if (!f || !label) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld || !f->kld->hyp) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "hypotheses are not enabled");
    Hyp* h = f->kld->hyp;
    if (h->last.n_hypotheses == 0) return fail(f, VISFS_BA_ERR_BAD_ARGUMENT, "there are no hypotheses since the particles were replaced");
    return guarded(f, [&]() -> int {
        const size_t bytes = (size_t)h->last.n * sizeof(int32_t);
        if (!f->device) { std::memcpy(label, h->h_label.data(), bytes); return (int)VISFS_BA_OK; }
        HIP_TRY(f, hipSetDevice(f->dev));
        HIP_TRY(f, hipMemcpyAsync(label, h->d_work.get(), bytes, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(f, hipStreamSynchronize(f->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_mcl_hyp_hook_rounds(const visfs_mcl* f, int32_t* rounds) {
    if (!f || !rounds) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!f->kld || !f->kld->hyp) { *rounds = 0; return VISFS_BA_ERR_BAD_ARGUMENT; }
    *rounds = f->kld->hyp->rounds;
    return VISFS_BA_OK;
}

int visfs_mcl_kld_hook_bins(int32_t n, const double* v, double size, int32_t* bins) {
    if (n < 0 || (n > 0 && (!v || !bins)) || !finite_pos(size)) return VISFS_BA_ERR_BAD_ARGUMENT;
    for (int32_t i = 0; i < n; ++i) {
        if (!std::isfinite(v[i])) return VISFS_BA_ERR_BAD_ARGUMENT;
        bins[i] = bin_of(v[i], size);
    }
    return VISFS_BA_OK;
}

}  // extern "C"
