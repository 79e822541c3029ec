// The shared host layer of the GPU objects (visfs_amd/csrc/ba_host.hpp) without a device: the check of a HIP call on each kind of
// sink, the guard of the C ABI for each kind of exception, and the small helpers.  Prints a line per failed check; exits with their count.
#include "ba_host.hpp"

#include <cstdio>
#include <stdexcept>
#include <string>

using namespace host;

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Object { std::string err; };

template <class S> int checked(S sink, bool fails, bool* after) {
    if (fails) HIP_TRY(sink, hipErrorInvalidValue);
    else HIP_TRY(sink, hipSuccess);
    *after = true;
    return VISFS_BA_OK;
}

const char* const kInvalid = "hipErrorInvalidValue: invalid argument";

void test_checks() {
    Object o;
    bool after = false;
    CHECK(checked(&o, true, &after) == VISFS_BA_ERR_DEVICE);
    CHECK(o.err == kInvalid);
    CHECK(!after);

    std::string text;
    CHECK(checked(&text, true, &after) == VISFS_BA_ERR_DEVICE);
    CHECK(text == kInvalid);
    CHECK(!after);

    CHECK(checked(nullptr, true, &after) == VISFS_BA_ERR_DEVICE);
    CHECK(!after);

    o.err = "untouched"; text = "untouched";
    CHECK(checked(&o, false, &after) == VISFS_BA_OK);
    CHECK(after && o.err == "untouched");
    after = false;
    CHECK(checked(&text, false, &after) == VISFS_BA_OK);
    CHECK(after && text == "untouched");
    after = false;
    CHECK(checked(nullptr, false, &after) == VISFS_BA_OK);
    CHECK(after);
}

void test_guarded() {
    Object o;
    CHECK(guarded(&o, []() -> int { throw std::bad_alloc(); }) == VISFS_BA_ERR_DEVICE);
    CHECK(o.err == "out of host memory");
    CHECK(guarded(&o, []() -> int { throw std::runtime_error("x"); }) == VISFS_BA_ERR_DEVICE);
    CHECK(o.err == "x");
    CHECK(guarded(&o, []() -> int { throw 7; }) == VISFS_BA_ERR_DEVICE);
    CHECK(o.err == "unexpected exception");

    std::string text;
    CHECK(guarded(&text, []() -> int { throw std::runtime_error("y"); }) == VISFS_BA_ERR_DEVICE);
    CHECK(text == "y");

    Object* none = nullptr;                                                // a null object and the null sink: nothing to write to
    CHECK(guarded(none, []() -> int { throw std::bad_alloc(); }) == VISFS_BA_ERR_DEVICE);
    CHECK(guarded(none, []() -> int { throw std::runtime_error("x"); }) == VISFS_BA_ERR_DEVICE);
    CHECK(guarded(none, []() -> int { throw 7; }) == VISFS_BA_ERR_DEVICE);
    CHECK(guarded(nullptr, []() -> int { throw std::bad_alloc(); }) == VISFS_BA_ERR_DEVICE);
    CHECK(guarded(nullptr, []() -> int { throw std::runtime_error("x"); }) == VISFS_BA_ERR_DEVICE);
    CHECK(guarded(nullptr, []() -> int { throw 7; }) == VISFS_BA_ERR_DEVICE);

    o.err = "untouched";
    CHECK(guarded(&o, []() -> int { return 3; }) == 3);
    CHECK(guarded(nullptr, []() -> int { return 3; }) == 3);
    CHECK(o.err == "untouched");
}

void test_helpers() {
    Object o;
    CHECK(fail(&o, VISFS_BA_ERR_BAD_ARGUMENT, "why") == VISFS_BA_ERR_BAD_ARGUMENT && o.err == "why");

    const Counts c{ 5, 6, 7 };
    int32_t l = -1, p = -1, w = -1;
    CHECK(c.read(&l, &p, &w) == VISFS_BA_OK && l == 5 && p == 6 && w == 7);
    l = p = w = -1;
    CHECK(c.read(nullptr, &p, nullptr) == VISFS_BA_OK && l == -1 && p == 6 && w == -1);
    l = p = w = -1;
    CHECK(c.read(&l, nullptr, &w) == VISFS_BA_OK && l == 5 && p == -1 && w == 7);
    CHECK(c.read(nullptr, nullptr, nullptr) == VISFS_BA_OK);
    const Counts zero{};
    CHECK(zero.launches == 0 && zero.copies == 0 && zero.waits == 0);

    CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512);
    CHECK(blocks_for(0, 256) == 0 && blocks_for(1, 256) == 1 && blocks_for(256, 256) == 1 && blocks_for(257, 256) == 2);
}

}  // namespace

int main() {
    test_checks();
    test_guarded();
    test_helpers();
    std::printf("%d failed\n", failures);
    return failures;
}
