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

// A device array of at least `need` items (`need + extra` are allocated); what it held is gone when it had to grow.
template <class S, class T> int grow(S sink, T** p, size_t* cap, size_t need, size_t extra = 0) {
    if (*cap >= need) return VISFS_BA_OK;
    if (*p) HIP_TRY(sink, hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(sink, hipMalloc(reinterpret_cast<void**>(p), (need + extra) * sizeof(T)));
    *cap = need + extra;
    return VISFS_BA_OK;
}

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
