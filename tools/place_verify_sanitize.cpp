// place_verify_sanitize.cpp — the guided search of the verified place query (visfs_amd/csrc/ba_place_verify.hpp,
// include/visfs_place_verify.h) under the address and undefined-behaviour sanitizers: a stand-alone program that drives the window
// test, the picks, the keeps and the twin at their edge shapes.  It needs no GPU and no HIP and is no part of the library; build it
// from the repository root with a host compiler:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ivisfs_amd/csrc
//       tools/place_verify_sanitize.cpp -o place_verify_sanitize && ./place_verify_sanitize
//
// The arrays here hold exactly the rows a case has, so a step past an end is a finding.  Prints one line per case and "ok"; any
// finding of a sanitizer ends it with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "ba_place_verify.hpp"

namespace {

using namespace place_verify;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

struct Rng {
    uint64_t s;
    uint64_t next() { return place::mix64(s += 0x9E3779B97F4A7C15ull); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct Case {                              // ne entries with their projections, nq queries
    int ne = 0, nq = 0;
    std::vector<double> pu, pv;
    std::vector<uint8_t> ok, qvalid;
    std::vector<uint32_t> edesc, qdesc;
    std::vector<float> qxy;
};

// every entry has a query of its own at `offset` px from its projection, `flips` bits away
Case paired(Rng& rng, int n, double offset, int flips) {
    Case c;
    c.ne = c.nq = n;
    c.pu.resize((size_t)n); c.pv.resize((size_t)n); c.ok.assign((size_t)n, 1); c.qvalid.assign((size_t)n, 1);
    c.edesc.resize((size_t)n * 8); c.qdesc.resize((size_t)n * 8); c.qxy.resize((size_t)n * 2);
    for (int j = 0; j < n; ++j) {
        c.pu[(size_t)j] = 20.0 * (j % 32) + rng.uni(); c.pv[(size_t)j] = 20.0 * (j / 32) + rng.uni();       // 20 px apart: windows do not meet
        for (int k = 0; k < 8; ++k) c.edesc[8 * (size_t)j + k] = c.qdesc[8 * (size_t)j + k] = (uint32_t)rng.next();
        for (int b = 0; b < flips; ++b) c.qdesc[8 * (size_t)j + (b % 8)] ^= 1u << (b / 8);
        c.qxy[2 * (size_t)j] = (float)(c.pu[(size_t)j] + offset); c.qxy[2 * (size_t)j + 1] = (float)c.pv[(size_t)j];
    }
    return c;
}

int run_twin(const Case& c, float radius, int maxd, std::vector<int32_t>* pick, std::vector<int32_t>* keep) {
    pick->assign(kMaxPoints, 12345); keep->assign(kMaxPoints, 12345);
    return guided_twin(c.pu.data(), c.pv.data(), c.ok.data(), c.edesc.data(), c.ne, c.qdesc.data(), c.qvalid.data(), c.qxy.data(), c.nq,
                       radius2(radius), maxd, pick->data(), keep->data());
}

int run() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const float inf = std::numeric_limits<float>::infinity();
    // the window: closed, in double, nothing that is not finite inside
    CHECK(in_window(100.0, 50.0, 103.0f, 54.0f, radius2(5.0f)));
    CHECK(!in_window(100.0, 50.0, 103.0f, 54.0f, radius2(std::nextafter(5.0f, 0.0f))));
    CHECK(in_window(17.25, 9.5, 17.25f, 9.5f, radius2(0.0f)) && !in_window(17.25 + 1e-9, 9.5, 17.25f, 9.5f, radius2(0.0f)));
    CHECK(!in_window(nan, 1.0, 1.0f, 1.0f, radius2(6.0f)) && !in_window(1.0, 1.0, inf, 1.0f, radius2(6.0f)) && !in_window(1.0, 1.0, 1.0f, -inf, radius2(6.0f)));
    CHECK(in_window(1e300, 0.0, 0.0f, 0.0f, radius2(6.0f)) == false);                      // the square overflows to +inf: outside
    std::printf("window: closed at the radius, radius 0, not finite\n");

    Rng rng{ 7 };
    std::vector<int32_t> pick, keep;
    for (int n : { 0, 1, 63, 64, 65, 511, 512 }) {
        const Case c = paired(rng, n, 1.0, 6);
        CHECK(run_twin(c, 6.0f, 64, &pick, &keep) == n);
        for (int j = 0; j < kMaxPoints; ++j) {
            CHECK(pick[(size_t)j] == (j < n ? pair_key(6, j) : kNone));
            CHECK(keep[(size_t)j] == (j < n ? pair_key(6, j) : kNone));
        }
        CHECK(run_twin(c, 0.5f, 64, &pick, &keep) == 0);                                   // 1 px away: outside a radius of 0.5
        CHECK(run_twin(c, 6.0f, 5, &pick, &keep) == 0);                                    // 6 bits away: beyond a distance of 5
        CHECK(run_twin(c, 6.0f, 6, &pick, &keep) == n && run_twin(c, 6.0f, 256, &pick, &keep) == n);
        std::printf("paired, n %d\n", n);
    }
    {
        Case c = paired(rng, 64, 1.0, 3);                                                  // entries that are not ok, queries that are not valid
        for (int j = 0; j < 64; j += 4) c.ok[(size_t)j] = 0;
        for (int i = 1; i < 64; i += 4) c.qvalid[(size_t)i] = 0;
        CHECK(run_twin(c, 6.0f, 64, &pick, &keep) == 32);
        for (int j = 0; j < 64; ++j) CHECK((pick[(size_t)j] != kNone) == (j % 4 >= 2));
        c.pu[2] = nan;                                                                     // (the library drops such an entry before; here it is in no window)
        CHECK(run_twin(c, 6.0f, 64, &pick, &keep) == 31);
        std::printf("invalid entries and queries\n");
    }
    {
        Case c = paired(rng, 8, 0.0, 2);                                                   // ties: two entries on one query, two queries in one window
        c.pu[5] = c.pu[1]; c.pv[5] = c.pv[1];
        for (int k = 0; k < 8; ++k) c.edesc[8 * 5 + (size_t)k] = c.edesc[8 * 1 + (size_t)k];
        c.qxy[2 * 6] = c.qxy[2 * 2] + 1.5f; c.qxy[2 * 6 + 1] = c.qxy[2 * 2 + 1];
        for (int k = 0; k < 8; ++k) c.qdesc[8 * 6 + (size_t)k] = c.qdesc[8 * 2 + (size_t)k];
        CHECK(run_twin(c, 6.0f, 64, &pick, &keep) == 6);                                   // queries 0 1 2 3 4 7
        CHECK(pick[1] == pick[5] && pick[1] == pair_key(2, 1) && keep[1] == pair_key(2, 1));      // the lower j
        CHECK(pick[2] == pair_key(2, 2) && keep[6] == kNone && pick[6] == kNone && keep[5] == kNone);      // the lower i
        std::printf("ties: the lower entry, the lower query\n");
    }
    {
        Case c = paired(rng, 512, 0.0, 0);                                                 // every query in every window: 512 x 512 distances
        for (int j = 0; j < 512; ++j) { c.pu[(size_t)j] = 5.0; c.pv[(size_t)j] = 5.0; c.qxy[2 * (size_t)j] = 5.0f; c.qxy[2 * (size_t)j + 1] = 5.0f; }
        CHECK(run_twin(c, 0.0f, 0, &pick, &keep) == 512);
        for (int j = 0; j < 512; ++j) CHECK(pick[(size_t)j] == pair_key(0, j) && keep[(size_t)j] == pair_key(0, j));
        CHECK(run_twin(c, 0.0f, 256, &pick, &keep) == 512);
        std::printf("512 entries on one pixel\n");
    }
    return 0;
}

}  // namespace

int main() {
    const int rc = run();
    if (rc == 0) std::printf("ok\n");
    return rc;
}
