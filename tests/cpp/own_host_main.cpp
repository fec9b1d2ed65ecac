// own_host_main.cpp -- the owners of HIP resources (zig-flac_amd/csrc/fg_own.hpp) on the host.  A
// stand-alone program, built by tests/test_own_host.py with -fsanitize=address,undefined against
// the stand-in tests/cpp/hipstub/hip/hip_runtime.h, whose allocations are host memory and whose
// calls are counted and logged: what DevBuf::grow calls and in which order, what a failed
// allocation and a move leave behind, where fit places the arrays of a Carve, and that everything
// allocated or created is released exactly once.  Prints "ok", or one line per failed check.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "../../zig-flac_amd/csrc/fg_own.hpp"

static int failures = 0;
#define CHECK(x)                                                                     \
    do {                                                                             \
        if (!(x)) {                                                                  \
            std::printf("line %d (n = %llu): %s\n", __LINE__, (unsigned long long)n, #x); \
            failures++;                                                              \
        }                                                                            \
    } while (0)

// the calls since the last take_log()
static std::string take_log() { return std::exchange(hipstub::log, std::string()); }

static void grow_cases(uint64_t n) {
    const hipStream_t st = (hipStream_t)1;
    fg::DevBuf<uint32_t> b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    // the first grow: one allocation of exactly n elements, or nothing at all for none
    CHECK(b.grow(n) == hipSuccess);
    CHECK(take_log() == (n ? "m" : ""));
    CHECK(b.cap() == n && (b.get() != nullptr) == (n != 0));
    if (n) std::memset(b.get(), 0xA5, n * sizeof(uint32_t));
    // within capacity: no call, with a stream or without
    uint32_t *const was = b.get();
    CHECK(b.grow(n, &st) == hipSuccess && b.grow(n ? n - 1 : 0) == hipSuccess && b.grow(0, &st) == hipSuccess);
    CHECK(take_log().empty() && b.get() == was && b.cap() == n);
    // beyond it, with a stream: the stream drains, the old buffer goes, the new one comes
    CHECK(b.grow(n + 1, &st) == hipSuccess);
    CHECK(take_log() == (n ? "sfm" : "sm"));
    CHECK(b.cap() == n + 1 && b.get() != nullptr);
    std::memset(b.get(), 0x5A, (n + 1) * sizeof(uint32_t));
    // without one: no wait
    CHECK(b.grow(n + 2) == hipSuccess);
    CHECK(take_log() == "fm" && b.cap() == n + 2);
    // a failed allocation leaves nothing, and the next grow starts afresh
    hipstub::fail_at = 1;
    CHECK(b.grow(n + 3, &st) == hipErrorOutOfMemory);
    CHECK(take_log() == "sfm" && b.get() == nullptr && b.cap() == 0);
    CHECK(b.grow(n + 3, &st) == hipSuccess);
    CHECK(take_log() == "sm" && b.get() != nullptr && b.cap() == n + 3);
}

static void move_cases(uint64_t n) {
    const int m0 = hipstub::mallocs, f0 = hipstub::frees;
    {
        fg::DevBuf<uint32_t> a, c;
        CHECK(a.grow(n + 1) == hipSuccess && c.grow(n + 2) == hipSuccess);
        uint32_t *const pa = a.get();
        fg::DevBuf<uint32_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == n + 1);
        CHECK(hipstub::frees == f0);
        c = std::move(b);  // what c held is freed here, once
        CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == n + 1);
        CHECK(hipstub::frees == f0 + 1);
    }
    CHECK(hipstub::mallocs == m0 + 2 && hipstub::frees == f0 + 2);
    take_log();
}

static void fit_cases(uint64_t n) {
    const hipStream_t st = (hipStream_t)1;
    fg::DevBuf<uint8_t> buf;
    uint64_t *a = nullptr;
    uint32_t *b = nullptr;
    uint8_t *c = nullptr;
    uint64_t used = 0;
    auto carve = [&](uint8_t *base) {  // 8-byte members first
        fg::Carve v{base};
        v.take(n, a, b);
        return used = v.take(n, c);
    };
    CHECK(fg::fit(buf, carve, &st) == hipSuccess);
    CHECK(take_log() == (n ? "sm" : ""));
    const uint64_t size = carve(nullptr);  // the size pass: no base, no pointers
    CHECK(a == nullptr && b == nullptr && c == nullptr);
    CHECK(carve(buf.get()) == size && buf.cap() == size && used == size);
    if (n == 0) {
        CHECK(size == 0 && buf.get() == nullptr && a == nullptr && b == nullptr && c == nullptr);
        return;
    }
    uint8_t *const lo = buf.get(), *const hi = lo + buf.cap();
    CHECK((uint8_t *)a == lo && (uint8_t *)(a + n) <= (uint8_t *)b && (uint8_t *)(b + n) <= c && c + n <= hi);
    CHECK((uintptr_t)a % 256 == 0 && (uintptr_t)b % 256 == 0 && (uintptr_t)c % 256 == 0);
    std::memset(a, 1, n * sizeof *a);  // every array is writable over its whole length
    std::memset(b, 2, n * sizeof *b);
    std::memset(c, 3, n * sizeof *c);
    // a carve that fits is placed in the buffer as it is
    uint8_t *d = nullptr;
    CHECK(fg::fit(buf, [&](uint8_t *base) { return fg::Carve{base}.take(n, d); }, &st) == hipSuccess);
    CHECK(take_log().empty() && d == lo);
    // a failed fit places nothing
    hipstub::fail_at = 1;
    CHECK(fg::fit(buf, [&](uint8_t *base) { return fg::Carve{base}.take(size + 1, d); }) == hipErrorOutOfMemory);
    CHECK(take_log() == "fm" && d == nullptr && buf.get() == nullptr && buf.cap() == 0);
}

static void handle_cases(uint64_t n) {
    const int d0 = hipstub::destroyed;
    {
        fg::Stream s, t;
        fg::Event e[2];
        CHECK(!s && !e[0]);
        CHECK(s.create() == hipSuccess && e[0].create() == hipSuccess && e[1].create(2u) == hipSuccess);
        const hipStream_t raw = s.get();
        t = std::move(s);
        CHECK(!s && t.get() == raw && e[0] && e[1] && e[0].get() != e[1].get());
        fg::Event f(std::move(e[0]));
        CHECK(!e[0] && f);
        CHECK(hipstub::destroyed == d0);
    }
    CHECK(hipstub::destroyed == d0 + 3);  // the empty ones destroy nothing
}

int main() {
    for (uint64_t n : {0, 1, 255, 256, 257}) {
        grow_cases(n);
        move_cases(n);
        fit_cases(n);
    }
    handle_cases(0);
    const uint64_t n = 0;
    CHECK(hipstub::mallocs == hipstub::frees && hipstub::mallocs > 0);
    CHECK(hipstub::made == hipstub::destroyed);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
