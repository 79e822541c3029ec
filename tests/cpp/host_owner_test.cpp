// The owner types of the shared host layer (visfs_amd/csrc/ba_host.hpp: DeviceBuf, PinnedBuf, Staged, Event) without a device and
// without the HIP runtime: this program defines the few runtime entry points the owners call itself, on malloc/free, with a table
// of the live blocks and a switch that fails the k-th call from now.  A free that is made to fail still lets the block go and
// reports the error, as hipFree does when it hands on the error of earlier work on the device.
// Prints a line per failed check; exits with their count.
//
// The same file is the sanitized stand-alone check (run by hand, never under pytest; profiles/owners_sanitize.log):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I<rocm>/include -Ivisfs_amd/csrc tests/cpp/host_owner_test.cpp -o host_owner_san && ./host_owner_san
#include "ba_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>

using namespace host;

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// ---------------------------------------------------------------- the runtime of this program
enum Kind { kDevice, kPinned, kEvent };
struct Runtime {
    std::map<void*, Kind> live;
    int calls = 0, allocs = 0, frees = 0, bad_frees = 0;      // bad: of a block that is not live, or through the wrong call
    int fail_in = 0;                                          // > 0: the fail_in-th call from now fails ...
    int fail_run = 1;                                         // ... and with it this many calls in a row
    size_t last_bytes = 0;
    unsigned last_flags = 0;
    std::string order;                                        // one letter per call: D d P p E e (capitals allocate)

    bool fails() {
        ++calls;
        if (fail_in == 0 || --fail_in > 0) return false;
        if (--fail_run > 0) fail_in = 1; else fail_run = 1;
        return true;
    }
    hipError_t make(void** p, size_t bytes, Kind k, char letter) {
        order += letter;
        if (fails()) return hipErrorOutOfMemory;
        *p = std::malloc(bytes ? bytes : 1);
        live[*p] = k; ++allocs; last_bytes = bytes;
        return hipSuccess;
    }
    hipError_t drop(void* p, Kind k, char letter) {
        order += letter;
        const bool failed = fails();
        if (p) {
            auto it = live.find(p);
            if (it == live.end() || it->second != k) ++bad_frees;
            else { live.erase(it); std::free(p); ++frees; }
        }
        return failed ? hipErrorInvalidValue : hipSuccess;
    }
    void reset() { CHECK(live.empty()); *this = Runtime(); }
} rt;

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return rt.make(p, bytes, kDevice, 'D'); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) { rt.last_flags = flags; return rt.make(p, bytes, kPinned, 'P'); }
hipError_t hipFree(void* p) { return rt.drop(p, kDevice, 'd'); }
hipError_t hipHostFree(void* p) { return rt.drop(p, kPinned, 'p'); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { rt.last_flags = flags; return rt.make(reinterpret_cast<void**>(e), 1, kEvent, 'E'); }
hipError_t hipEventDestroy(hipEvent_t e) { return rt.drop(e, kEvent, 'e'); }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipSuccess ? "no error" : "invalid argument"; }
}

namespace {

struct Object { std::string err; };

template <class B> bool holds(const B& b) { return b.get() && rt.live.count(const_cast<void*>(static_cast<const void*>(b.get()))) == 1; }
template <class B> bool empty(const B& b) { return !b && b.get() == nullptr && b.cap() == 0; }
// what every owner must keep at any moment: a null pointer goes with capacity 0, a set one is a live block
template <class B> bool sound(const B& b) { return b.get() ? (holds(b) && b.cap() > 0) : b.cap() == 0; }

template <class B> void test_buf(const char* alloc_name, const char* free_name, char A, char F) {
    const std::string sA(1, A), sF(1, F);
    Object o;
    {   // alloc then destroy frees once
        B b;
        CHECK(empty(b));
        CHECK(b.alloc(&o, 10) == VISFS_BA_OK && holds(b) && b.cap() == 10 && bool(b));
        CHECK(rt.last_bytes == 10 * sizeof(*b.get()));
    }
    CHECK(rt.order == sA + sF && rt.allocs == 1 && rt.frees == 1 && rt.bad_frees == 0);
    rt.reset();
    {   // a move leaves the source empty; the block is freed once, by the one that holds it
        B a;
        CHECK(a.alloc(&o, 4) == VISFS_BA_OK);
        const void* p = a.get();
        B b(std::move(a));
        CHECK(empty(a) && b.get() == p && b.cap() == 4);
        B c;
        CHECK(c.alloc(&o, 2) == VISFS_BA_OK);
        c = std::move(b);                                      // frees what c held
        CHECK(empty(b) && c.get() == p && c.cap() == 4 && rt.frees == 1 && rt.live.size() == 1);
    }
    CHECK(rt.allocs == 2 && rt.frees == 2 && rt.bad_frees == 0);
    rt.reset();
    {   // a release that fails still empties the owner and reports the error; nothing is freed twice
        B b;
        CHECK(b.alloc(&o, 3) == VISFS_BA_OK);
        rt.fail_in = 1;
        o.err.clear();
        CHECK(b.release(&o) == VISFS_BA_ERR_DEVICE && empty(b));
        CHECK(o.err == std::string(free_name) + ": invalid argument");
        CHECK(b.release(&o) == VISFS_BA_OK && empty(b));       // nothing to do, no call
    }
    CHECK(rt.calls == 2 && rt.bad_frees == 0);
    rt.reset();
    {   // a failed allocation: the text names the call and the bytes, the owner is empty
        B b;
        rt.fail_in = 1;
        CHECK(b.alloc(&o, 5) == VISFS_BA_ERR_DEVICE && empty(b));
        CHECK(o.err == std::string(alloc_name) + "(" + std::to_string(5 * sizeof(*b.get())) + " bytes): out of memory");
        CHECK(b.alloc(nullptr, 5) == VISFS_BA_OK && holds(b));         // the null sink drops the text
    }
    rt.reset();
    {   // grow below the capacity does nothing; above it frees, then allocates need + extra
        B b;
        CHECK(b.grow(&o, 8, 4) == VISFS_BA_OK && b.cap() == 12 && rt.order == sA);
        const void* p = b.get();
        CHECK(b.grow(&o, 12, 100) == VISFS_BA_OK && b.get() == p && b.cap() == 12 && rt.calls == 1);
        CHECK(b.grow(&o, 0) == VISFS_BA_OK && rt.calls == 1);
        CHECK(b.grow(&o, 13, 2) == VISFS_BA_OK && b.cap() == 15 && rt.order == sA + sF + sA);
        CHECK(rt.last_bytes == 15 * sizeof(*b.get()) && rt.live.size() == 1 && holds(b));
    }
    CHECK(rt.bad_frees == 0);
    rt.reset();
    // every call of a grow failing in turn: no block is live that the owner does not hold, none is freed twice, null goes with 0
    for (int k = 1; k <= 2; ++k) {
        {
            B b;
            CHECK(b.alloc(&o, 4) == VISFS_BA_OK);
            rt.fail_in = k;
            CHECK(b.grow(&o, 9, 1) == VISFS_BA_ERR_DEVICE);
            CHECK(empty(b) && rt.live.empty() && rt.bad_frees == 0);
            CHECK(b.grow(&o, 9, 1) == VISFS_BA_OK && b.cap() == 10 && holds(b) && rt.live.size() == 1);   // the next call starts clean
        }
        CHECK(rt.bad_frees == 0);
        rt.reset();
    }
}

using Pair = Staged<double>;
bool pair_sound(const Pair& s) {                               // all or nothing, and nothing else alive
    const bool both = holds(s.h) && holds(s.d) && s.h.cap() == s.d.cap() && s.cap() > 0 && rt.live.size() == 2;
    const bool none = empty(s.h) && empty(s.d) && s.cap() == 0 && rt.live.empty();
    return both || none;
}

void test_staged() {
    Object o;
    {   // reserve, destroy: each half freed once; the caller's capacity is what is allocated
        Pair s;
        bool grew = false;
        CHECK(s.reserve(&o, 10, 16, &grew) == VISFS_BA_OK && grew && s.cap() == 16 && pair_sound(s));
        CHECK(rt.order == "PD" && rt.last_flags == hipHostMallocDefault);
        CHECK(s.reserve(&o, 16, 99, &grew) == VISFS_BA_OK && !grew && s.cap() == 16 && rt.calls == 2);       // below the capacity: nothing
        CHECK(s.reserve(&o, 17, 40, &grew) == VISFS_BA_OK && grew && s.cap() == 40 && pair_sound(s));
        CHECK(rt.order == "PDpdPD");                           // the objects' order: both frees, then both allocations
        CHECK(s.reserve(&o, 0, 0) == VISFS_BA_OK && rt.calls == 6);
    }
    CHECK(rt.allocs == 4 && rt.frees == 4 && rt.bad_frees == 0);
    rt.reset();
    {   // a move leaves the source empty
        Pair a;
        CHECK(a.reserve(&o, 1, 1) == VISFS_BA_OK);
        Pair b(std::move(a));
        CHECK(empty(a.h) && empty(a.d) && a.cap() == 0 && pair_sound(b));
    }
    rt.reset();
    {   // a release that fails still empties both halves and reports the first error
        Pair s;
        CHECK(s.reserve(&o, 2, 2) == VISFS_BA_OK);
        rt.fail_in = 1;
        CHECK(s.release(&o) == VISFS_BA_ERR_DEVICE && o.err == "hipHostFree: invalid argument" && pair_sound(s) && s.cap() == 0);
    }
    CHECK(rt.bad_frees == 0);
    rt.reset();
    {   // both frees fail: both halves are empty all the same, and the text is the first failure's
        Pair s;
        CHECK(s.reserve(&o, 2, 2) == VISFS_BA_OK);
        rt.fail_in = 1; rt.fail_run = 2;
        CHECK(s.release(&o) == VISFS_BA_ERR_DEVICE && o.err == "hipHostFree: invalid argument" && pair_sound(s) && s.cap() == 0);
        CHECK(rt.order == "PDpd" && rt.fail_in == 0 && rt.fail_run == 1);
        CHECK(s.reserve(&o, 2, 2) == VISFS_BA_OK);
        rt.fail_in = 1; rt.fail_run = 2;
        o.err.clear();
        CHECK(s.reserve(&o, 3, 3) == VISFS_BA_ERR_DEVICE && o.err == "hipHostFree: invalid argument" && pair_sound(s) && s.cap() == 0);
    }
    CHECK(rt.bad_frees == 0);
    rt.reset();
    // each of the four calls of a growing reserve failing in turn, then each of the two of a first reserve
    for (int k = 1; k <= 4; ++k) {
        {
            Pair s;
            bool grew = false;
            CHECK(s.reserve(&o, 4, 4) == VISFS_BA_OK);
            rt.fail_in = k;
            CHECK(s.reserve(&o, 5, 8, &grew) == VISFS_BA_ERR_DEVICE && grew);
            CHECK(pair_sound(s) && s.cap() == 0 && rt.bad_frees == 0);
            CHECK(s.reserve(&o, 5, 8, &grew) == VISFS_BA_OK && grew && s.cap() == 8 && pair_sound(s));       // the next call reallocates
        }
        CHECK(rt.bad_frees == 0);
        rt.reset();
    }
    for (int k = 1; k <= 2; ++k) {
        {
            Pair s;
            rt.fail_in = k;
            CHECK(s.reserve(&o, 3, 3) == VISFS_BA_ERR_DEVICE && pair_sound(s) && s.cap() == 0);
        }
        CHECK(rt.bad_frees == 0);
        rt.reset();
    }
}

void test_event() {
    Object o;
    {
        Event e;
        CHECK(!e && e.get() == nullptr);
        CHECK(e.create(&o, hipEventDisableTiming) == VISFS_BA_OK && e && rt.live.count(e.get()) == 1 && rt.last_flags == hipEventDisableTiming);
        Event f(std::move(e));
        CHECK(!e && f && rt.live.size() == 1);
        Event g;
        g = std::move(f);
        CHECK(!f && g && rt.live.size() == 1);
    }
    CHECK(rt.order == "Ee" && rt.bad_frees == 0);
    rt.reset();
    {
        Event e;
        rt.fail_in = 1;
        CHECK(e.create(&o, 0) == VISFS_BA_ERR_DEVICE && !e && o.err == "hipEventCreateWithFlags: out of memory");
    }
    CHECK(rt.order == "E" && rt.bad_frees == 0);
    rt.reset();
}

// ---------------------------------------------------------------- the shapes that went wrong with raw pointers
// The corner discs: the pinned half is freed, the free of the device half fails.  The pointers used to stay set over a freed block,
// the next call wrote through it and the release freed it again.
void regression_disc_reserve_second_free_fails() {
    Object o;
    {
        Staged<char> disc;
        CHECK(disc.reserve(&o, 100, 16384) == VISFS_BA_OK);
        rt.fail_in = 2;                                        // hipHostFree passes, hipFree fails
        CHECK(disc.reserve(&o, 20000, 40000) == VISFS_BA_ERR_DEVICE && o.err == "hipFree: invalid argument");
        CHECK(!disc.h && !disc.d && disc.cap() == 0 && rt.live.empty());
        CHECK(disc.reserve(&o, 20000, 40000) == VISFS_BA_OK && disc.cap() == 40000);     // the next call reallocates
    }                                                          // corners_release
    CHECK(rt.bad_frees == 0);
    rt.reset();
}

// grow() on raw pointers left *p set when the free failed.
void regression_grow_failed_free_leaves_null() {
    Object o;
    {
        DeviceBuf<int32_t> sums;
        CHECK(sums.grow(&o, 10, 5) == VISFS_BA_OK);
        rt.fail_in = 1;
        CHECK(sums.grow(&o, 100, 50) == VISFS_BA_ERR_DEVICE && sums.get() == nullptr && sums.cap() == 0 && sound(sums));
    }
    CHECK(rt.bad_frees == 0);
    rt.reset();
}

// The matcher's record and its pinned copy are made together behind one test.  The test looked at the device half only, so after a
// failed pinned allocation every later call skipped the block and wrote through a null pointer.
template <class S> int record_pair(S sink, DeviceBuf<double>& d_rec, PinnedBuf<double>& h_rec) {
    if (!d_rec || !h_rec) {
        RC_TRY(d_rec.alloc(sink, 1));
        RC_TRY(h_rec.alloc(sink, 1));
    }
    return VISFS_BA_OK;
}
void regression_record_pair_pinned_half_fails() {
    Object o;
    {
        DeviceBuf<double> d_rec;
        PinnedBuf<double> h_rec;
        rt.fail_in = 2;
        CHECK(record_pair(&o, d_rec, h_rec) == VISFS_BA_ERR_DEVICE && d_rec && !h_rec);
        CHECK(record_pair(&o, d_rec, h_rec) == VISFS_BA_OK && holds(d_rec) && holds(h_rec) && rt.live.size() == 2);      // made again, nothing left behind
        CHECK(record_pair(&o, d_rec, h_rec) == VISFS_BA_OK && rt.calls == 5);                                              // D P(fails) d D P, then nothing
    }
    CHECK(rt.order == "DPdDPpd" && rt.bad_frees == 0);
    rt.reset();
}

}  // namespace

int main() {
    test_buf<DeviceBuf<float>>("hipMalloc", "hipFree", 'D', 'd');
    test_buf<PinnedBuf<uint64_t>>("hipHostMalloc", "hipHostFree", 'P', 'p');
    test_staged();
    test_event();
    regression_disc_reserve_second_free_fails();
    regression_grow_failed_free_leaves_null();
    regression_record_pair_pinned_half_fails();
    CHECK(rt.live.empty());
    std::printf("%d failed\n", failures);
    return failures;
}
