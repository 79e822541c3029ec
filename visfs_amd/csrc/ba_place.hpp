// ba_place.hpp — the arithmetic of visual place recognition (include/visfs_place.h), shared by the HIP kernels of
// ba_place.hip and the one-core twin: the pattern, a key-point's centre, the orientation score, the Hamming distance, the accept
// rule and the ranking key, and the twin itself over plain arrays.  Integers throughout behind the lrintf of a centre.  The file
// needs nothing of HIP: a host compiler takes it as it is (tools/place_sanitize.cpp).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PLACE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PLACE_HD inline
#endif

namespace place {

constexpr int kMaxPoints = 512;        // key-points of a set, entries of a slot
constexpr int kMaxKeyframes = 1024;
constexpr int kMaxCandidates = 8;
constexpr int kDescWords = 8;          // 256 bits
constexpr int kBins = 32;
constexpr int kPatternPoints = 512;    // two per test
constexpr int kMargin = 15;            // 13 (a rotated point) + 2 (its 5 x 5 box); the moments' disc has the same radius
constexpr int kPatch = 31;             // 2 * kMargin + 1
constexpr int kReach = 13;             // no rotated point lies further out in either axis
constexpr int kBox = 27;               // 2 * kReach + 1 box sums a side
constexpr int kNoSecond = 257;

// rint(16384 cos(2 pi k / 32)), rint(16384 sin(2 pi k / 32)): literals, the checker of the tests holds the same 64 numbers
struct CosSin { int16_t c, s; };
constexpr CosSin kRot[kBins] = {
    { 16384, 0 }, { 16069, 3196 }, { 15137, 6270 }, { 13623, 9102 }, { 11585, 11585 }, { 9102, 13623 }, { 6270, 15137 }, { 3196, 16069 },
    { 0, 16384 }, { -3196, 16069 }, { -6270, 15137 }, { -9102, 13623 }, { -11585, 11585 }, { -13623, 9102 }, { -15137, 6270 }, { -16069, 3196 },
    { -16384, 0 }, { -16069, -3196 }, { -15137, -6270 }, { -13623, -9102 }, { -11585, -11585 }, { -9102, -13623 }, { -6270, -15137 }, { -3196, -16069 },
    { 0, -16384 }, { 3196, -16069 }, { 6270, -15137 }, { 9102, -13623 }, { 11585, -11585 }, { 13623, -9102 }, { 15137, -6270 }, { 16069, -3196 },
};

// What the device holds of the definition: the rotated points and the 32 rotations.  Made once on the host.
struct Table {
    int8_t pts[kBins][kPatternPoints][2];
    CosSin rot[kBins];
};

struct Params { int32_t first, n_slots, max_distance, ratio_num, ratio_den, min_matches, cross_check; };

// the splitmix64 finaliser, as ba_pnp.hpp has it
PLACE_HD uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Returns false if a rotated point left [-kReach, kReach] (it does not: the tests hold the table to that).
inline bool make_table(Table* t) {
    int base[kPatternPoints][2];
    int kept = 0;
    for (uint64_t c = 0; kept < kPatternPoints; ++c) {
        const uint64_t h = mix64(0x9E3779B97F4A7C15ull * (c + 1));
        const int x = (int)(h & 31) - 16, y = (int)((h >> 8) & 31) - 16;
        if (x * x + y * y > 169) continue;
        base[kept][0] = x; base[kept][1] = y;
        ++kept;
    }
    bool inside = true;
    for (int k = 0; k < kBins; ++k) {
        t->rot[k] = kRot[k];
        const int c = kRot[k].c, s = kRot[k].s;
        for (int p = 0; p < kPatternPoints; ++p) {
            const int x = base[p][0], y = base[p][1];
            const int xr = (x * c - y * s + 8192) >> 14, yr = (x * s + y * c + 8192) >> 14;
            inside = inside && xr >= -kReach && xr <= kReach && yr >= -kReach && yr <= kReach;
            t->pts[k][p][0] = (int8_t)xr; t->pts[k][p][1] = (int8_t)yr;
        }
    }
    return inside;
}

// lrintf rounds half to even in the default rounding mode, on the host and on the device
PLACE_HD bool centre_of(float x, float y, int w, int h, int* cx, int* cy) {
    if (!(x - x == 0.0f) || !(y - y == 0.0f)) return false;                                   // NaN or infinite
    if (!(x >= -1.0f && x <= (float)w && y >= -1.0f && y <= (float)h)) return false;          // outside the image, so not valid by the rule below: keeps lrintf in range
    const long ix = lrintf(x), iy = lrintf(y);
    if (ix < kMargin || ix > w - 1 - kMargin || iy < kMargin || iy > h - 1 - kMargin) return false;
    *cx = (int)ix; *cy = (int)iy;
    return true;
}

PLACE_HD int64_t bin_score(const CosSin r, int32_t m10, int32_t m01) { return (int64_t)m10 * r.c + (int64_t)m01 * r.s; }

PLACE_HD int hamming(const uint32_t* a, const uint32_t* b) {
    int d = 0;
    for (int k = 0; k < kDescWords; ++k) d += __builtin_popcount(a[k] ^ b[k]);
    return d;
}

// A row's running nearest and second nearest: best = D * 1024 + j of the nearest, d2 = the smallest D of the others.
struct Nearest {
    int32_t best = 0x7fffffff, d2 = kNoSecond;
    PLACE_HD void take(int d, int j) {
        const int32_t key = d * 1024 + j;
        if (key < best) { if (best != 0x7fffffff) d2 = best >> 10; best = key; }
        else if (d < d2) d2 = d;
    }
};

// column_min: the smallest D(i', j1) * 1024 + i' over the valid queries
PLACE_HD bool accepted(const Nearest& nn, int i, int32_t column_min, const Params& p) {
    if (nn.best == 0x7fffffff) return false;
    const int d1 = nn.best >> 10;
    if (d1 > p.max_distance) return false;
    if (!(d1 * p.ratio_den < nn.d2 * p.ratio_num)) return false;
    return !p.cross_check || column_min == d1 * 1024 + i;
}

// a slot's place in the ranking: greater is better; -1: not a candidate
PLACE_HD int32_t rank_key(int32_t count, int32_t slot, int32_t min_matches) { return count >= min_matches ? count * 1024 + (1023 - slot) : -1; }

// an accepted match as the matcher leaves it for the ranking: db index | distance << 16, -1: not accepted
PLACE_HD int32_t pack_match(int j1, int d1) { return j1 | (d1 << 16); }

// ---------------------------------------------------------------------------------------------------------------- the one-core twin
// One key-point: desc[32], *valid, *bin.  px: level 0, w x h, rows of w bytes.
inline void describe_one(const Table& T, const uint8_t* px, int w, int h, float x, float y, uint8_t* desc, uint8_t* valid, uint8_t* bin) {
    std::memset(desc, 0, 32);
    *valid = 0; *bin = 0;
    int cx, cy;
    if (!centre_of(x, y, w, h, &cx, &cy)) return;
    int32_t m10 = 0, m01 = 0;
    for (int dy = -kMargin; dy <= kMargin; ++dy)
        for (int dx = -kMargin; dx <= kMargin; ++dx) {
            if (dx * dx + dy * dy > kMargin * kMargin) continue;
            const int v = px[(int64_t)(cy + dy) * w + cx + dx];
            m10 += dx * v; m01 += dy * v;
        }
    int best = 0;
    int64_t best_score = bin_score(T.rot[0], m10, m01);
    for (int k = 1; k < kBins; ++k) {
        const int64_t s = bin_score(T.rot[k], m10, m01);
        if (s > best_score) { best_score = s; best = k; }
    }
    const auto box = [&](int u, int v) {
        int s = 0;
        for (int j = -2; j <= 2; ++j)
            for (int i = -2; i <= 2; ++i) s += px[(int64_t)(cy + v + j) * w + cx + u + i];
        return s;
    };
    for (int t = 0; t < 256; ++t) {
        const int8_t* a = T.pts[best][2 * t];
        const int8_t* b = T.pts[best][2 * t + 1];
        if (box(a[0], a[1]) < box(b[0], b[1])) desc[t >> 3] |= (uint8_t)(1u << (t & 7));
    }
    *valid = 1; *bin = (uint8_t)best;
}

// One slot: match[i] (pack_match or -1) for the nq queries against the ne entries; returns the count.  Descriptors as 8 words a row.
inline int32_t match_slot(const uint32_t* qdesc, const uint8_t* qvalid, int nq, const uint32_t* edesc, const uint8_t* evalid, int ne,
                          const Params& p, int32_t* match) {
    int32_t col[kMaxPoints];
    for (int j = 0; j < ne; ++j) {
        int32_t m = 0x7fffffff;
        if (evalid[j])
            for (int i = 0; i < nq; ++i) {
                if (!qvalid[i]) continue;
                const int32_t key = hamming(qdesc + 8 * i, edesc + 8 * j) * 1024 + i;
                if (key < m) m = key;
            }
        col[j] = m;
    }
    int32_t count = 0;
    for (int i = 0; i < nq; ++i) {
        match[i] = -1;
        if (!qvalid[i]) continue;
        Nearest nn;
        for (int j = 0; j < ne; ++j)
            if (evalid[j]) nn.take(hamming(qdesc + 8 * i, edesc + 8 * j), j);
        if (nn.best == 0x7fffffff) continue;
        const int j1 = nn.best & 1023;
        if (accepted(nn, i, col[j1], p)) { match[i] = pack_match(j1, nn.best >> 10); ++count; }
    }
    return count;
}

// The candidates of counts[0 .. n_slots) (slot first + k): cand[c] = k, best first; returns how many.
inline int rank_slots(const int32_t* counts, const Params& p, int32_t* cand) {
    int n = 0;
    bool taken[kMaxKeyframes] = {};
    for (; n < kMaxCandidates; ++n) {
        int32_t best = -1, at = -1;
        for (int k = 0; k < p.n_slots; ++k) {
            if (taken[k]) continue;
            const int32_t key = rank_key(counts[k], p.first + k, p.min_matches);
            if (key > best) { best = key; at = k; }
        }
        if (at < 0) break;
        taken[at] = true;
        cand[n] = at;
    }
    return n;
}

}  // namespace place
