// place_sanitize.cpp — the one-core twin of visual place recognition (visfs_amd/csrc/ba_place.hpp, include/visfs_place.h) under the
// address and undefined-behaviour sanitizers: a stand-alone program that drives describe, add and query at their edge shapes.  It
// needs no GPU and no HIP and is no part of the library; build it from the repository root with a host compiler:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ivisfs_amd/csrc tools/place_sanitize.cpp
//       -o place_sanitize && ./place_sanitize
//
// The twin's functions work on plain arrays; the store here is a vector of the same blocks the library keeps.  Prints one line per
// case and "ok"; any finding of a sanitizer ends it with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>

#include "ba_place.hpp"

namespace {

using namespace place;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

struct Rng {
    uint64_t s;
    uint64_t next() { return mix64(s += 0x9E3779B97F4A7C15ull); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct Set {                               // exactly n rows, so a step past the end is a finding
    int n = 0;
    std::vector<float> xy;
    std::vector<uint32_t> desc;
    std::vector<uint8_t> valid, bin;
};

struct Slot { Set set; std::vector<int32_t> ids; std::vector<float> xyz; int64_t key = 0; };

void describe(const Table& T, const std::vector<uint8_t>& img, int w, int h, const std::vector<float>& xy, Set* s) {
    s->n = (int)xy.size() / 2;
    s->xy = xy;
    s->desc.assign((size_t)s->n * 8, 0u); s->valid.assign((size_t)s->n, 0); s->bin.assign((size_t)s->n, 0);
    for (int i = 0; i < s->n; ++i)
        describe_one(T, img.data(), w, h, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], reinterpret_cast<uint8_t*>(s->desc.data() + 8 * (size_t)i),
                     &s->valid[(size_t)i], &s->bin[(size_t)i]);
}

// the query of the library's twin over the slots [first, last): counts, candidates and the rows' indices
struct Answer { std::vector<int32_t> count; std::vector<int32_t> cand; std::vector<std::vector<int32_t>> rows; };

int query(const Set& q, const std::vector<Slot>& slots, int first, int last, Params p, Answer* a) {
    p.first = first; p.n_slots = last - first;
    a->count.assign((size_t)p.n_slots, 0);
    std::vector<std::vector<int32_t>> match((size_t)p.n_slots);
    for (int k = 0; k < p.n_slots; ++k) {
        const Set& e = slots[(size_t)(first + k)].set;
        match[(size_t)k].assign((size_t)q.n, -1);
        a->count[(size_t)k] = match_slot(q.desc.data(), q.valid.data(), q.n, e.desc.data(), e.valid.data(), e.n, p, match[(size_t)k].data());
        int32_t seen = 0;
        for (int32_t m : match[(size_t)k]) {
            if (m < 0) continue;
            ++seen;
            CHECK((m & 0xffff) < e.n && (m >> 16) <= p.max_distance && e.valid[(size_t)(m & 0xffff)]);
        }
        CHECK(seen == a->count[(size_t)k]);
    }
    int32_t cand[kMaxCandidates];
    const int n = rank_slots(a->count.data(), p, cand);
    CHECK(n >= 0 && n <= kMaxCandidates);
    a->cand.assign(cand, cand + n);
    a->rows.clear();
    for (int c = 0; c < n; ++c) {
        CHECK(cand[c] >= 0 && cand[c] < p.n_slots && a->count[(size_t)cand[c]] >= p.min_matches);
        if (c > 0) {
            const int32_t a0 = a->count[(size_t)cand[c - 1]], a1 = a->count[(size_t)cand[c]];
            CHECK(a0 > a1 || (a0 == a1 && cand[c - 1] < cand[c]));
        }
        a->rows.push_back(match[(size_t)cand[c]]);
    }
    return 0;
}

int run() {
    auto table = std::make_unique<Table>();
    CHECK(make_table(table.get()));
    const Table& T = *table;
    for (int k = 0; k < kBins; ++k)
        for (int t = 0; t < 256; ++t)
            CHECK(T.pts[k][2 * t][0] != T.pts[k][2 * t + 1][0] || T.pts[k][2 * t][1] != T.pts[k][2 * t + 1][1]);
    std::printf("pattern: 32 bins, no test of two equal points, reach 13\n");

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    Params prm{ 0, 0, 64, 4, 5, 1, 1 };
    for (const auto& size : { std::pair<int, int>{ 160, 120 }, { 161, 121 }, { 31, 31 } }) {
        const int w = size.first, h = size.second;
        Rng rng{ (uint64_t)w };
        std::vector<uint8_t> img((size_t)w * h);                        // exactly w * h bytes: a read past an edge is a finding
        for (auto& v : img) v = (uint8_t)(rng.next() & 0xff);
        for (int n : { 0, 1, 63, 64, 65, 511, 512 }) {
            std::vector<float> xy;
            const float edge[] = { 14.f, 15.f, 14.5f, 15.5f, (float)(w - 16), (float)(w - 15), (float)w - 15.5f, (float)(h - 16), (float)(h - 15), nan, inf,
                                   -inf, -1e9f, 1e9f, 3e38f, -0.f };
            for (int i = 0; i < n; ++i) {
                if (i < 256) { xy.push_back(edge[i % 16]); xy.push_back(edge[(i / 16) % 16]); }
                else { xy.push_back((float)(rng.uni() * (w + 8) - 4)); xy.push_back((float)(rng.uni() * (h + 8) - 4)); }
            }
            Set s;
            describe(T, img, w, h, xy, &s);
            int valid = 0;
            for (int i = 0; i < n; ++i) {
                int cx, cy;
                const bool in = centre_of(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], w, h, &cx, &cy);
                CHECK(in == (s.valid[(size_t)i] != 0) && s.bin[(size_t)i] < kBins);
                if (in) CHECK(cx >= 15 && cx <= w - 16 && cy >= 15 && cy <= h - 16);
                valid += in;
            }
            if (n >= 63) CHECK(valid > 0);
            std::printf("describe %d x %d, n %d: %d valid\n", w, h, n, valid);
        }
    }

    // a constant image: bin 0, no bit set
    {
        std::vector<uint8_t> img(64 * 64, 200);
        Set s;
        describe(T, img, 64, 64, { 32.f, 32.f, 15.f, 48.f }, &s);
        CHECK(s.valid[0] && s.valid[1] && s.bin[0] == 0 && s.bin[1] == 0);
        for (uint32_t v : s.desc) CHECK(v == 0u);
        std::printf("constant image: bin 0, all bits zero\n");
    }

    // the store: 1, 2, 63, 64, 65 and 1024 slots of few entries; then slots of 0, 1 and 512 entries against 512 queries
    Rng rng{ 99 };
    const auto random_set = [&](int n, int invalid_every) {
        Set s;
        s.n = n; s.xy.assign((size_t)n * 2, 1.0f); s.desc.resize((size_t)n * 8); s.valid.assign((size_t)n, 1); s.bin.assign((size_t)n, 0);
        for (auto& v : s.desc) v = (uint32_t)rng.next();
        if (invalid_every > 0)
            for (int i = invalid_every - 1; i < n; i += invalid_every) { s.valid[(size_t)i] = 0; for (int k = 0; k < 8; ++k) s.desc[8 * (size_t)i + k] = 0u; }
        return s;
    };
    const auto add = [&](std::vector<Slot>& slots, const Set& s, int64_t key) {
        Slot sl;
        sl.set = s; sl.key = key; sl.ids.assign((size_t)s.n, 7); sl.xyz.assign((size_t)s.n * 3, 0.5f);
        slots.push_back(sl);
    };
    for (int n_slots : { 1, 2, 63, 64, 65, 1024 }) {
        const Set q = random_set(40, 9);
        std::vector<Slot> slots;
        for (int k = 0; k < n_slots; ++k) {
            Set e = random_set(12, k % 3 == 0 ? 5 : 0);
            if (k % 5 == 0 || k == n_slots - 1)
                for (int j = 0; j < 6 + (k == n_slots - 1 ? 4 : 0); ++j)
                    for (int b = 0; b < 8; ++b) e.desc[8 * (size_t)(j + 1) + b] = q.desc[8 * (size_t)j + b] ^ (b == 0 ? 0x111u : 0u);
            add(slots, e, k);
        }
        Answer a;
        prm.min_matches = 3;
        CHECK(query(q, slots, 0, n_slots, prm, &a) == 0);
        CHECK((int)a.cand.size() == (n_slots >= 63 ? 8 : n_slots) && a.cand[0] == n_slots - 1);
        Answer none;
        CHECK(query(q, slots, n_slots, n_slots, prm, &none) == 0 && none.cand.empty());
        if (n_slots > 2) { CHECK(query(q, slots, 1, n_slots - 1, prm, &a) == 0 && a.cand[0] + 1 != n_slots - 1); }
        std::printf("query over %d slots: %zu candidates\n", n_slots, a.cand.size());
    }
    {
        const Set q = random_set(512, 17);
        std::vector<Slot> slots;
        add(slots, random_set(0, 0), 1);
        Set one = random_set(1, 0);
        for (int b = 0; b < 8; ++b) one.desc[(size_t)b] = q.desc[8 * 5 + (size_t)b];
        add(slots, one, 2);
        Set full = q;                                                   // every query meets itself: distance 0, d2 > 0
        add(slots, full, 3);
        Set twice = random_set(512, 0);                                 // every entry twice: d1 = d2, nothing passes
        for (int j = 0; j < 256; ++j)
            for (int b = 0; b < 8; ++b) twice.desc[8 * (size_t)(256 + j) + b] = twice.desc[8 * (size_t)j + b] = q.desc[8 * (size_t)j + b];
        add(slots, twice, 4);
        for (int cross : { 1, 0 })
            for (int maxd : { 0, 64, 256 }) {
                Answer a;
                prm.min_matches = 1; prm.cross_check = cross; prm.max_distance = maxd;
                CHECK(query(q, slots, 0, 4, prm, &a) == 0);
                int valid = 0;
                for (uint8_t v : q.valid) valid += v;
                CHECK(a.count[0] == 0 && a.count[2] == valid && !a.cand.empty());
                if (maxd <= 64) {                                       // beyond it random descriptors (about 128 apart) come into reach
                    CHECK(a.count[1] == 1 && a.count[3] == 0);
                    CHECK(a.cand.size() == 2 && a.cand[0] == 2 && a.cand[1] == 1);
                }
            }
        Set nothing = random_set(512, 1);                               // no valid query
        Answer a;
        CHECK(query(nothing, slots, 0, 4, prm, &a) == 0 && a.cand.empty());
        prm.min_matches = 0;
        CHECK(query(nothing, slots, 0, 4, prm, &a) == 0 && a.cand.size() == 4 && a.cand[0] == 0 && a.cand[3] == 3);
        std::printf("slots of 0, 1 and 512 entries against 512 queries, duplicates, no valid query\n");
    }
    return 0;
}

}  // namespace

int main() {
    const int rc = run();
    if (rc == 0) std::printf("ok\n");
    return rc;
}
