// AMCL's pose hypotheses on the KLD filter (include/visfs_mcl_hyp.h): the record, the tail that
// k_mcl_kld_resample<true> of ba_mcl_kld.hip runs after the new set is written, the one-core twin and the host's finish.
//
// The device and the twin agree byte for byte: the clusters, their labels, counts and ranks are integers that do not depend on the
// schedule (a label is the lowest draw index of a component), and each of the seven sums of a hypothesis is the adjacent-pair tree
// of section 9t over the new set in index order, an element outside the hypothesis entering as +0.0.
#pragma once
#pragma clang fp contract(off)

#include "ba_mcl_kld.hpp"

#include "../../include/visfs_mcl_hyp.h"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>

namespace mcl {

constexpr int kHypSums = 7;                   // x, y, cos, sin, xx, xy, yy
constexpr int kHypNbr = 26;                   // the neighbours of a bin
constexpr int kHypWorkInts = 4 + kHypNbr;     // per draw: label, count, bins, degree, the neighbours' draws
constexpr int kHypBlock = VISFS_MCL_KLD_MAX_PARTICLES / kKldThreads;   // the draws a work item holds at the most: 16

struct HypEntry {
    int32_t label, count, bins, pad;
    double sums[kHypSums];
};

// What a resampling adds to the record.
struct HypBlock {
    int32_t n_clusters, n_hyp, rounds, pad;
    HypEntry hyp[VISFS_MCL_HYP_MAX];
};

// What an update of a filter with hypotheses downloads: k_mcl_kld_resample<true> writes h (only when it resamples).
struct HypRec {
    KldRec k;
    HypBlock h;
};

// What k_mcl_kld_resample<true> is told beside KldArgs.
struct HypArgs {
    int32_t* work;                            // [kHypWorkInts cap]
    double* cs;                               // [2 cap]: cos and sin of the new set's yaws
};

// The seven terms of a particle (cos c, sin s of its yaw).
__host__ __device__ inline void hyp_terms(double x, double y, double c, double s, double t[kHypSums]) {
    t[0] = x; t[1] = y; t[2] = c; t[3] = s; t[4] = x * x; t[5] = x * y; t[6] = y * y;
}

#if defined(__HIPCC__)

// The adjacent-pair tree of one term over the B elements from i0 (B = 1, 2, 4, 8 or 16, i0 a multiple of it).  The term of draw i
// is a[i], times b[i] when b is set; bit j of `in` tells whether draw i0 + j belongs to the hypothesis, every other element is +0.0.
// The loads of a block are issued together.  a and b are written by other work items of the launch before a barrier: no __restrict__.
__device__ inline double hyp_block_tree(int32_t i0, int32_t B, uint32_t in, const double* a, const double* b) {
    double v[kHypBlock];
#pragma unroll
    for (int j = 0; j < kHypBlock; ++j) {
        v[j] = 0.0;
        if (j < B && ((in >> j) & 1u)) v[j] = b ? a[i0 + j] * b[i0 + j] : a[i0 + j];
    }
#pragma unroll
    for (int s = 1; s < kHypBlock; s <<= 1) {
        if (s < B) {                                                       // the same in every work item
#pragma unroll
            for (int j = 0; j < kHypBlock; j += 2 * s) v[j] = v[j] + v[j + s];
        }
    }
    return v[0];
}

__device__ inline double hyp_shfl_xor(double v, int m) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const int lo = __shfl_xor((int)(uint32_t)(u & 0xFFFFFFFFull), m), hi = __shfl_xor((int)(uint32_t)(u >> 32), m);
    return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo));
}

// The labels and counts in device memory change under integer atomics, which act in the L2: every read of them goes there too.
__device__ inline int32_t hyp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void hyp_lower(int32_t* p, int32_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The draw of the bin (bx, by, bz) in the finished table, or -1: a probe ends at an empty slot, the table being at most half full.
__device__ inline int32_t hyp_find(const int32_t* table, uint32_t mask, uint32_t home_mask, const int32_t* __restrict__ bins, int32_t n_new,
                                   int32_t bx, int32_t by, int32_t bz) {
    uint32_t h = (uint32_t)bin_hash(bx, by, bz) & home_mask;
    for (;;) {
        const int32_t j = table[h];
        if (j == kKldEmpty) return -1;
        const int32_t* o = bins + 3 * (size_t)j;
        if (o[0] == bx && o[1] == by && o[2] == bz) return j < n_new ? j : -1;     // a bin first drawn at or after n* is not of the new set
        h = (h + 1u) & mask;
    }
}

// The tail of k_mcl_kld_resample<true>: every work item of the one workgroup calls it after the new set is written.  `table` is the
// finished table (slot -> lowest draw of its bin), w_slot and w_bin the draws' slots and bins, n_bins the bins of the new set.
__device__ inline void hyp_tail(const int32_t* table, uint32_t mask, uint32_t home_mask, const int32_t* __restrict__ w_slot,
                                const int32_t* __restrict__ w_bin, int32_t n_new, int32_t n_bins, int32_t cap, const double* out,
                                const HypArgs G, HypBlock* __restrict__ hb) {
    __shared__ double sh[VISFS_MCL_HYP_MAX][kKldWaves][kHypSums];
    __shared__ uint32_t s_key[VISFS_MCL_HYP_MAX];
    __shared__ int32_t s_flag[2];
    __shared__ int32_t s_clusters;
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* lab = G.work;                                                 // by draw: the label of its bin (during the rounds: of the bins' lowest draws)
    int32_t* cnt = G.work + (size_t)cap;                                   // by label
    int32_t* bct = G.work + 2 * (size_t)cap;                               // by label
    int32_t* deg = G.work + 3 * (size_t)cap;                               // by lowest draw: its bin's neighbours that exist ...
    int32_t* nbr = G.work + 4 * (size_t)cap;                               // ... and their lowest draws, [kHypNbr][cap]

    // ---- 8. every bin of the new set starts as its own label and finds its neighbours once; cos and sin of every yaw
    if (tid < VISFS_MCL_HYP_MAX) s_key[tid] = 0;
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; s_clusters = 0; }
    uint32_t lows = 0;                                                     // bit j: draw tid + 1024 j is the lowest of its bin
    for (int32_t i = tid; i < n_new; i += kKldThreads) {
        lab[i] = i; cnt[i] = 0; bct[i] = 0;
        double s, c;
        sincos_any(out[2 * (size_t)n_new + i], s, c);
        G.cs[i] = c; G.cs[(size_t)cap + i] = s;
        int32_t d = 0;
        if (table[w_slot[i]] == i) {                                       // the lowest draw of its bin
            lows |= 1u << (i / kKldThreads);
            const int32_t bx = w_bin[3 * (size_t)i], by = w_bin[3 * (size_t)i + 1], bz = w_bin[3 * (size_t)i + 2];
            for (int32_t q = 0; q < 27; ++q) {
                if (q == 13) continue;
                const int32_t j = hyp_find(table, mask, home_mask, w_bin, n_new, bx + q % 3 - 1, by + (q / 3) % 3 - 1, bz + q / 9 - 1);   // |index| <= 2^24: no overflow
                if (j >= 0) nbr[(size_t)d++ * cap + i] = j;
            }
        }
        deg[i] = d;
    }
    __syncthreads();

    // ---- 9. rounds of minimum-label propagation with hooking, then one pointer jump; at most n_bins rounds.  A label only falls
    // and is always the lowest draw of a bin of the same component; a round without a change leaves every component at its minimum.
    int32_t rounds = 0;
    for (int32_t r = 0; r < n_bins; ++r) {
        bool changed = false;
        for (uint32_t todo = lows; todo; todo &= todo - 1u) {
            const int32_t i = tid + (__ffs((int)todo) - 1) * kKldThreads;
            const int32_t old = hyp_load(&lab[i]), d = deg[i];
            int32_t m = old;
            for (int32_t q = 0; q < d; ++q) {
                const int32_t v = hyp_load(&lab[nbr[(size_t)q * cap + i]]);
                if (v < m) m = v;
            }
            if (m < old) { hyp_lower(&lab[old], m); hyp_lower(&lab[i], m); changed = true; }
        }
        __syncthreads();
        if (tid == 0) s_flag[(r + 1) & 1] = 0;                             // the next round's flag: last read before the barrier above
        for (uint32_t todo = lows; todo; todo &= todo - 1u) {
            const int32_t i = tid + (__ffs((int)todo) - 1) * kKldThreads;
            const int32_t l = hyp_load(&lab[i]), ll = hyp_load(&lab[l]);
            if (ll < l) { hyp_lower(&lab[i], ll); changed = true; }
        }
        if (changed) atomicOr(&s_flag[r & 1], 1);
        __syncthreads();
        ++rounds;
        if (s_flag[r & 1] == 0) break;                                     // the same in every work item
    }

    // ---- 10. every draw's label; the counts by integer atomics, one add for each of a wavefront's first four labels
    int32_t roots = 0;
    for (int32_t i0 = 0; i0 < n_new; i0 += kKldThreads) {
        const int32_t i = i0 + tid;
        const bool live = i < n_new;
        int32_t L = -1;
        bool low = false;
        if (live) {
            const int32_t rep = table[w_slot[i]];
            low = rep == i;
            L = hyp_load(&lab[rep]);
            if (!low) lab[i] = L;                                          // no other work item reads a draw that is not the lowest of its bin
            else if (L == i) ++roots;
        }
        unsigned long long todo = __ballot(live);
        for (int pass = 0; pass < 4 && todo; ++pass) {                     // the wavefront's first labels, one add each; the same in every lane
            const int32_t L0 = __shfl(L, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(live && L == L0);
            const unsigned long long firsts = __ballot(live && L == L0 && low);
            if (lane == __ffsll((long long)same) - 1) {
                atomicAdd(&cnt[L0], (int32_t)__popcll(same));
                if (firsts) atomicAdd(&bct[L0], (int32_t)__popcll(firsts));
            }
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) {                                       // many labels in one wavefront: the rest add for themselves
            atomicAdd(&cnt[L], 1);
            if (low) atomicAdd(&bct[L], 1);
        }
    }
    if (roots) atomicAdd(&s_clusters, roots);
    __syncthreads();

    // ---- 11. the ranks: eight maxima of (count, ~label) over the clusters below the last maximum
    uint32_t keys[kHypBlock];                                              // of the clusters whose lowest draw is this work item's; 0: none
#pragma unroll
    for (int j = 0; j < kHypBlock; ++j) {
        const int32_t i = tid + j * kKldThreads;
        keys[j] = 0;
        if (i < n_new && hyp_load(&lab[i]) == i)                           // only a cluster's lowest draw carries its own index
            keys[j] = ((uint32_t)hyp_load(&cnt[i]) << 14) | (uint32_t)(VISFS_MCL_KLD_MAX_PARTICLES - 1 - i);
    }
    uint32_t prev = 0xFFFFFFFFu;
    int32_t n_hyp = 0;
    for (int32_t q = 0; q < VISFS_MCL_HYP_MAX; ++q) {
        uint32_t best = 0;
#pragma unroll
        for (int j = 0; j < kHypBlock; ++j)
            if (keys[j] < prev && keys[j] > best) best = keys[j];
        for (int m = 1; m < 64; m <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)best, m);
            if (o > best) best = o;
        }
        if (lane == 0 && best) atomicMax(&s_key[q], best);
        __syncthreads();
        prev = s_key[q];
        if (prev == 0) break;                                              // the same in every work item
        ++n_hyp;
    }

    // ---- 12. the seven sums of every hypothesis: an aligned block per work item, xor shuffles, the wave values through LDS
    int32_t P = 1;
    while (P < n_new) P *= 2;
    const int32_t B = P > kKldThreads ? P / kKldThreads : 1;               // 1, 2, 4, 8 or 16
    const int32_t i0 = tid * B;
    for (int32_t q = 0; q < n_hyp; ++q) {
        const int32_t L = VISFS_MCL_KLD_MAX_PARTICLES - 1 - (int32_t)(s_key[q] & (uint32_t)(VISFS_MCL_KLD_MAX_PARTICLES - 1));
        uint32_t in = 0;                                                   // which draws of the block belong to the hypothesis
        for (int32_t j = 0; j < B; ++j)
            if (i0 + j < n_new && hyp_load(&lab[i0 + j]) == L) in |= 1u << j;
#pragma unroll 1
        for (int k = 0; k < kHypSums; ++k) {                               // x, y, cos, sin, xx, xy, yy: one block of loads serves every k
            const double* ys = out + (size_t)n_new;
            const double* a = k == 2 ? G.cs : k == 3 ? G.cs + (size_t)cap : (k == 1 || k == 6) ? ys : out;
            const double* b = k < 4 ? nullptr : k == 4 ? out : ys;
            double t = in ? hyp_block_tree(i0, B, in, a, b) : 0.0;         // a block without a particle of the hypothesis sums to +0.0
            for (int m = 1; m < 64; m <<= 1) {
                if (m * B >= P) break;                                     // the tree ends at P elements
                t = t + hyp_shfl_xor(t, m);
            }
            if (lane == 0) sh[q][wave][k] = t;
        }
    }
    __syncthreads();
    if (tid < VISFS_MCL_HYP_MAX * kHypSums) {
        const int32_t q = tid / kHypSums, k = tid % kHypSums;
        double v = 0.0;
        if (q < n_hyp) {
            double a[kKldWaves];
            for (int w = 0; w < kKldWaves; ++w) a[w] = sh[q][w][k];
            for (int s = 1; s < kKldWaves; s <<= 1)
                if (s * 64 * B < P)
                    for (int w = 0; w < kKldWaves; w += 2 * s) a[w] = a[w] + a[w + s];
            v = a[0];
        }
        hb->hyp[q].sums[k] = v;
    }
    if (tid < VISFS_MCL_HYP_MAX) {
        HypEntry& e = hb->hyp[tid];
        const uint32_t key = s_key[tid];
        const int32_t L = VISFS_MCL_KLD_MAX_PARTICLES - 1 - (int32_t)(key & (uint32_t)(VISFS_MCL_KLD_MAX_PARTICLES - 1));
        const bool on = tid < n_hyp;
        e.label = on ? L : 0; e.count = on ? (int32_t)(key >> 14) : 0; e.bins = on ? hyp_load(&bct[L]) : 0; e.pad = 0;
    }
    if (tid == 0) { hb->n_clusters = s_clusters; hb->n_hyp = n_hyp; hb->rounds = rounds; hb->pad = 0; }
}

#endif  // __HIPCC__

// ---------------------------------------------------------------- host only

// The twin: the definition on the new set (x, y, yaw, each [n]) with a std::map of bin triples and a flood fill.
inline void hyp_host(const double* x, const double* y, const double* yaw, int32_t n, double bin_xy, double bin_yaw, std::vector<int32_t>& label,
                     HypBlock& hb) {
    using Bin = std::array<int32_t, 3>;
    std::memset(&hb, 0, sizeof hb);
    const size_t ns = (size_t)n;
    std::vector<Bin> bin_of_draw(ns);
    std::map<Bin, int32_t> lowest;                                         // the lowest draw of every bin
    for (size_t i = 0; i < ns; ++i) {
        bin_of_draw[i] = { bin_of(x[i], bin_xy), bin_of(y[i], bin_xy), bin_of(yaw[i], bin_yaw) };
        lowest.emplace(bin_of_draw[i], (int32_t)i);                        // keeps the first
    }
    std::map<Bin, int32_t> label_of;
    std::vector<int32_t> count(ns, 0), bins(ns, 0);
    for (size_t i = 0; i < ns; ++i) {                                      // ascending draws: an unlabelled bin's lowest draw is its component's lowest
        if (lowest[bin_of_draw[i]] != (int32_t)i || label_of.count(bin_of_draw[i])) continue;
        std::vector<Bin> todo{ bin_of_draw[i] };
        label_of[bin_of_draw[i]] = (int32_t)i;
        while (!todo.empty()) {
            const Bin b = todo.back();
            todo.pop_back();
            ++bins[i];
            for (int32_t q = 0; q < 27; ++q) {
                const Bin c = { b[0] + q % 3 - 1, b[1] + (q / 3) % 3 - 1, b[2] + q / 9 - 1 };      // |index| <= 2^24: no overflow
                if (lowest.count(c) && !label_of.count(c)) { label_of[c] = (int32_t)i; todo.push_back(c); }
            }
        }
    }
    label.resize(ns);
    std::vector<int32_t> roots;
    for (size_t i = 0; i < ns; ++i) {
        label[i] = label_of[bin_of_draw[i]];
        if (count[(size_t)label[i]]++ == 0) roots.push_back(label[i]);
    }
    std::sort(roots.begin(), roots.end(), [&](int32_t a, int32_t b) { return count[(size_t)a] != count[(size_t)b] ? count[(size_t)a] > count[(size_t)b] : a < b; });
    hb.n_clusters = (int32_t)roots.size();
    hb.n_hyp = std::min<int32_t>(hb.n_clusters, VISFS_MCL_HYP_MAX);
    const size_t P = (size_t)pow2_at_least(n);
    std::vector<double> terms[kHypSums];
    for (int32_t q = 0; q < hb.n_hyp; ++q) {
        HypEntry& e = hb.hyp[q];
        e.label = roots[(size_t)q]; e.count = count[(size_t)e.label]; e.bins = bins[(size_t)e.label];
        for (auto& v : terms) v.assign(P, 0.0);
        for (size_t i = 0; i < ns; ++i) {
            if (label[i] != e.label) continue;
            double s, c, t[kHypSums];
            sincos_any(yaw[i], s, c);
            hyp_terms(x[i], y[i], c, s, t);
            for (int k = 0; k < kHypSums; ++k) terms[k][i] = t[k];
        }
        for (int k = 0; k < kHypSums; ++k) e.sums[k] = tree_sum(terms[k]);
    }
}

// The host's end, shared by the device path and the twin: section 9t's formulas with the count in W's place.
inline void hyp_finish(const HypBlock& hb, int32_t n, int64_t update, visfs_mcl_hyp_result& out) {
    std::memset(&out, 0, sizeof out);
    out.fresh = 1; out.n_clusters = hb.n_clusters; out.n_hypotheses = hb.n_hyp; out.n = n; out.update = update;
    for (int32_t q = 0; q < hb.n_hyp && q < VISFS_MCL_HYP_MAX; ++q) {
        const HypEntry& e = hb.hyp[q];
        visfs_mcl_hypothesis& h = out.hyp[q];
        const double* S = e.sums;
        const double W = (double)e.count;
        h.label = e.label; h.count = e.count; h.bins = e.bins;
        h.weight = W / (double)n;
        const double mx = S[0] / W, my = S[1] / W, mc = S[2] / W, ms = S[3] / W;
        h.mean[0] = mx; h.mean[1] = my; h.mean[2] = std::atan2(S[3], S[2]);
        h.covariance[0] = S[4] / W - mx * mx;
        h.covariance[1] = h.covariance[3] = S[5] / W - mx * my;
        h.covariance[4] = S[6] / W - my * my;
        const double len = std::sqrt(mc * mc + ms * ms);
        h.covariance[8] = len < 1.0 ? (len > 0.0 ? -2.0 * std::log(len) : HUGE_VAL) : 0.0;
    }
}

}  // namespace mcl
