// The host plumbing every GPU object of the library shares: where the text of a failure goes, the check of a
// HIP call, the guard that keeps exceptions inside the C ABI, and a few small helpers.  Host code only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <exception>
#include <new>
#include <string>

#include "../../include/visfs_ba.h"

namespace host __attribute__((visibility("hidden"))) {      // nothing of it is exported by the library

// ---- where the text of a failure goes: an object with a std::string `err` (a null pointer drops the text), a string, or nowhere.
// A sink of another kind brings its own overload in its own namespace (the tracker's CallFault, the opaque sub-maps of
// ba_submap_access.hpp): HIP_TRY and guarded find it there.
template <class T> void set_error(T* obj, const std::string& text) { if (obj) obj->err = text; }
inline void set_error(std::string* s, const std::string& text) { if (s) *s = text; }
inline void set_error(std::nullptr_t, const std::string&) {}

template <class T> int fail(T* obj, int rc, const std::string& why) { obj->err = why; return rc; }

// Leaves the calling function with VISFS_BA_ERR_DEVICE when a HIP call fails, its text "<the call as written>: <HIP's message>" in `sink`.
#define HIP_TRY(sink, expr)                                                                   \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            using host::set_error;                                                            \
            set_error((sink), std::string(#expr) + ": " + hipGetErrorString(e_));             \
            return VISFS_BA_ERR_DEVICE;                                                       \
        }                                                                                     \
    } while (0)

// Leaves the calling function with the code of a step of the library's own that did not return VISFS_BA_OK (its text is written already).
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_ != VISFS_BA_OK) return rc_; } while (0)

// No exception may cross the C ABI: host allocations (std::vector, std::string, std::thread) can throw.  Writing the text can throw
// as well, so that is guarded too.
template <class S, class F> int guarded(S sink, F&& f) noexcept {
    const auto say = [&](const char* text) noexcept { try { set_error(sink, text); } catch (...) {} return (int)VISFS_BA_ERR_DEVICE; };
    try { return f(); }
    catch (const std::bad_alloc&) { return say("out of host memory"); }
    catch (const std::exception& e) { return say(e.what()); }
    catch (...) { return say("unexpected exception"); }
}

// ---- small helpers
inline size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
inline unsigned blocks_for(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// ---- owners of what an object allocates.  Move-only; none of them switches the device or waits for a stream: the object does that
// in its destructor's body, which runs before its members' destructors.  A failed call leaves VISFS_BA_ERR_DEVICE and the text
// "<runtime call>(<bytes> bytes): <HIP's message>" (frees and events: "<runtime call>: <HIP's message>").
template <class S> int hip_failed(S sink, const char* call, hipError_t e, const size_t* bytes = nullptr) {
    set_error(sink, std::string(call) + (bytes ? "(" + std::to_string(*bytes) + " bytes)" : std::string()) + ": " + hipGetErrorString(e));
    return VISFS_BA_ERR_DEVICE;
}

struct DeviceMem {
    static constexpr const char* kAlloc = "hipMalloc";
    static constexpr const char* kFree = "hipFree";
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
};
struct PinnedMem {
    static constexpr const char* kAlloc = "hipHostMalloc";
    static constexpr const char* kFree = "hipHostFree";
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void* p) { return hipHostFree(p); }
};

// A block of `cap()` items of T.  `Mem` only tells the two kinds apart and is never named by an object: objects write DeviceBuf<T>
// and PinnedBuf<T>, and there is no allocator to pass.
template <class T, class Mem> class Buf {
    T* p_ = nullptr;
    size_t cap_ = 0;
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { (void)release(nullptr); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Buf() { (void)release(nullptr); }

    T* get() const { return p_; }
    T* operator->() const { return p_; }
    T& operator*() const { return *p_; }
    T& operator[](size_t i) const { return p_[i]; }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

    // Empty before a failed free is reported: the block is never reached, or freed, a second time.
    template <class S> int release(S sink) {
        if (!p_) { cap_ = 0; return VISFS_BA_OK; }
        T* const old = p_;
        p_ = nullptr; cap_ = 0;
        const hipError_t e = Mem::free(old);
        return e == hipSuccess ? VISFS_BA_OK : hip_failed(sink, Mem::kFree, e);
    }
    // A new block of `n` items; what was held is released first.
    template <class S> int alloc(S sink, size_t n) {
        if (const int rc = release(sink)) return rc;
        const size_t bytes = n * sizeof(T);
        void* q = nullptr;
        const hipError_t e = Mem::alloc(&q, bytes);
        if (e != hipSuccess) return hip_failed(sink, Mem::kAlloc, e, &bytes);
        p_ = static_cast<T*>(q); cap_ = q ? n : 0;
        return VISFS_BA_OK;
    }
    // At least `need` items (`need + extra` are allocated); what it held is gone when it had to grow.
    template <class S> int grow(S sink, size_t need, size_t extra = 0) { return cap_ >= need ? (int)VISFS_BA_OK : alloc(sink, need + extra); }
};
template <class T> using DeviceBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

// A pinned source `h` and its device copy `d` under one capacity.  All or nothing: after a failed reserve both are empty.
template <class T> struct Staged {
    PinnedBuf<T> h;
    DeviceBuf<T> d;
    size_t cap() const { return d.cap(); }
    // At least `need` items; when that takes new blocks they have `n` items (the caller's growth rule) and *grew says so.
    template <class S> int reserve(S sink, size_t need, size_t n, bool* grew = nullptr) {
        if (grew) *grew = false;
        if (cap() >= need) return VISFS_BA_OK;
        if (grew) *grew = true;
        int rc = release(sink);
        if (rc == VISFS_BA_OK) rc = h.alloc(sink, n);
        if (rc == VISFS_BA_OK) rc = d.alloc(sink, n);
        if (rc != VISFS_BA_OK) { (void)h.release(nullptr); (void)d.release(nullptr); }
        return rc;
    }
    // Both halves go, whatever the frees say; the first failure is the one reported.
    template <class S> int release(S sink) {
        const int rc = h.release(sink);
        const int rd = d.release(rc == VISFS_BA_OK ? sink : S(nullptr));
        return rc != VISFS_BA_OK ? rc : rd;
    }
};

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { if (e_) (void)hipEventDestroy(e_); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    template <class S> int create(S sink, unsigned flags) {
        if (e_) { const hipEvent_t old = e_; e_ = nullptr; (void)hipEventDestroy(old); }
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) { e_ = nullptr; return hip_failed(sink, "hipEventCreateWithFlags", e); }
        return VISFS_BA_OK;
    }
};

// what a call issued, as the *_last_counts exports report it
struct Counts {
    int32_t launches = 0, copies = 0, waits = 0;
    int read(int32_t* l, int32_t* c, int32_t* w) const {
        if (l) *l = launches;
        if (c) *c = copies;
        if (w) *w = waits;
        return VISFS_BA_OK;
    }
};

}  // namespace host
