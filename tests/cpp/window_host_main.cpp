// window_host_main.cpp -- the scalar rules of the sample-window decode (fg_window.hpp) run entirely
// on the host: the block size at a frame's offset and the positions they sum to, the cover of a
// window over a position slice, and the unit decomposition of the copy.  A stand-alone program,
// built by tests/test_window_host.py with -fsanitize=address,undefined.
//
//   window_host_main positions BLOB N  (OFFSET BITS RATE FRAMES SIZE x FRAMES) x N
//       BLOB holds the streams at their OFFSETs (any alignment; the file is read into an allocation
//       of exactly its size, so a read past a stream that ends the blob is a sanitizer error).
//       Every stream's frames get a slice of one position table, GUARD entries apart.
//       Prints {"streams": [{"positions": [...], "total": T}], "untouched": bool}.
//   window_host_main cover N BLOCK x N  M (START COUNT) x M
//       Positions from the block sizes; every window's cover against a plain linear search (exit 1
//       on a difference).  Prints {"covers": [[first_frame, n_frames, span, skip, n_samples]]}.
//   window_host_main copy
//       Every source alignment 0-15, destination alignment 0-15 and length 0-48: the copy by the
//       plan (bytes, whole 16-byte units through load_unit, bytes) into a guarded buffer against
//       memcpy; the source allocation ends at the 8-byte boundary after its last byte.
//       Prints {"cases": count}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_window.hpp"

using namespace fg;
using namespace fg::window;

namespace {

constexpr uint64_t GUARD = 3, FILL = 0xA5A5A5A5A5A5A5A5ull;

uint64_t u64(const char *s) { return std::strtoull(s, nullptr, 10); }

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "window_host_main: %s\n", what);
    std::exit(1);
}

int run_positions(int argc, char **argv) {
    if (argc < 4) fail("usage");
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) fail("cannot open the blob");
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t *blob = (uint8_t *)std::malloc(size > 0 ? (size_t)size : 1u);
    if (size > 0 && std::fread(blob, 1, (size_t)size, f) != (size_t)size) fail("short read");
    std::fclose(f);
    const uint32_t n = (uint32_t)u64(argv[3]);
    struct Stream {
        uint64_t first, frames;
        uint32_t bits, rate;
    };
    std::vector<Stream> streams;
    std::vector<uint64_t> f_off;
    std::vector<uint32_t> f_bytes;
    int a = 4;
    for (uint32_t s = 0; s < n; s++) {
        if (a + 4 > argc) fail("usage");
        uint64_t at = u64(argv[a]);
        Stream st{f_off.size() + GUARD, u64(argv[a + 3]), (uint32_t)u64(argv[a + 1]), (uint32_t)u64(argv[a + 2])};
        a += 4;
        f_off.resize(st.first, FILL);
        f_bytes.resize(st.first, 0xA5A5A5A5u);
        for (uint64_t i = 0; i < st.frames; i++, a++) {
            if (a >= argc) fail("usage");
            f_off.push_back(at);
            f_bytes.push_back((uint32_t)u64(argv[a]));
            at += f_bytes.back();
        }
        if (at > (uint64_t)size) fail("a stream passes the blob");
        streams.push_back(st);
    }
    f_off.resize(f_off.size() + GUARD, FILL);
    std::vector<uint64_t> pos(f_off.size(), FILL), totals(n, FILL);
    for (uint32_t s = 0; s < n; s++) {
        const Stream &st = streams[s];
        // k_pos_blocks: one lane per entry
        for (uint64_t i = 0; i < st.frames; i++)
            pos[st.first + i] = block_at(blob + f_off[st.first + i], f_bytes[st.first + i], st.bits, st.rate);
        // k_pos_scan: 256 entries an iteration, a carried total
        uint64_t carry = 0;
        for (uint64_t i0 = 0; i0 < st.frames; i0 += 256u) {
            uint64_t run = 0;
            for (uint64_t i = i0; i < st.frames && i < i0 + 256u; i++) {
                const uint64_t x = pos[st.first + i];
                pos[st.first + i] = carry + run;
                run += x;
            }
            carry += run;
        }
        totals[s] = carry;
    }
    std::vector<bool> owned(pos.size(), false);
    std::printf("{\"streams\": [");
    for (uint32_t s = 0; s < n; s++) {
        std::printf("%s{\"positions\": [", s ? ", " : "");
        for (uint64_t i = 0; i < streams[s].frames; i++) {
            owned[streams[s].first + i] = true;
            std::printf("%s%llu", i ? ", " : "", (unsigned long long)pos[streams[s].first + i]);
        }
        std::printf("], \"total\": %llu}", (unsigned long long)totals[s]);
    }
    bool untouched = true;
    for (size_t i = 0; i < pos.size(); i++)
        if (!owned[i] && pos[i] != FILL) untouched = false;
    std::printf("], \"untouched\": %s}\n", untouched ? "true" : "false");
    std::free(blob);
    return 0;
}

int run_cover(int argc, char **argv) {
    if (argc < 3) fail("usage");
    int a = 2;
    const uint64_t n = u64(argv[a++]);
    // exactly n entries: a search that looks at pos[n] is a sanitizer error
    uint64_t *pos = (uint64_t *)std::malloc(n ? n * 8u : 1u);
    std::vector<uint64_t> blocks;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (a >= argc) fail("usage");
        pos[i] = total;
        blocks.push_back(u64(argv[a++]));
        total += blocks.back();
    }
    if (a >= argc) fail("usage");
    const uint64_t m = u64(argv[a++]);
    std::printf("{\"covers\": [");
    for (uint64_t w = 0; w < m; w++, a += 2) {
        if (a + 2 > argc) fail("usage");
        const uint64_t start = u64(argv[a]), count = u64(argv[a + 1]);
        const Cover c = cover(pos, n, total, start, count);
        // the plain rule: frame i covers the window if it holds one of the samples [start, end)
        const uint64_t left = start < total ? total - start : 0u;
        const uint64_t take = count < left ? count : left, end = start + take;
        uint64_t first = 0, frames = 0, span = 0;
        for (uint64_t i = 0, at = 0; i < n && take; at += blocks[i], i++) {
            if (at + blocks[i] <= start || at >= end) continue;
            if (!frames) first = i;
            frames++;
            span += blocks[i];
        }
        const uint64_t skip = frames ? start - pos[first] : 0u;
        if (c.status != WIN_OK || c.first_frame != first || c.n_frames != frames || c.span != span || c.skip != skip ||
            c.n_samples != take)
            fail("a cover differs from the linear search");
        std::printf("%s[%llu, %u, %llu, %llu, %llu]", w ? ", " : "", (unsigned long long)c.first_frame, c.n_frames,
                    (unsigned long long)c.span, (unsigned long long)c.skip, (unsigned long long)c.n_samples);
    }
    std::printf("]}\n");
    std::free(pos);
    return 0;
}

int run_copy() {
    constexpr uint32_t PAD = 32;
    uint32_t cases = 0;
    for (uint32_t sa = 0; sa < 16u; sa++)
        for (uint32_t da = 0; da < 16u; da++)
            for (uint32_t len = 0; len <= 48u; len++, cases++) {
                void *sp = nullptr, *dp = nullptr;
                const size_t src_size = ((size_t)sa + len + 7u) & ~(size_t)7u;  // ends at the 8-byte boundary after the last byte
                if (posix_memalign(&sp, 16, src_size ? src_size : 8u) || posix_memalign(&dp, 16, 2u * PAD + 64u + 16u))
                    fail("no memory");
                uint8_t *src = (uint8_t *)sp + sa, *base = (uint8_t *)dp, *dst = base + PAD + da;
                for (size_t i = 0; i < src_size; i++) ((uint8_t *)sp)[i] = (uint8_t)(i * 37u + sa * 5u + len + 1u);
                std::vector<uint8_t> want(2u * PAD + 64u + 16u, 0xA5);
                std::memset(base, 0xA5, want.size());
                if (len) std::memcpy(want.data() + PAD + da, src, len);
                const CopyPlan p = copy_plan((uint64_t)(uintptr_t)dst, len);
                if (p.head > 15u || p.tail > 15u || p.head + 16u * p.units + p.tail != len) fail("the plan does not add up");
                if ((p.units || p.tail) && ((uintptr_t)(dst + p.head) & 15u)) fail("a unit is not aligned");
                for (uint32_t t = 0; t < p.head; t++) dst[t] = src[t];
                for (uint64_t u = 0; u < p.units; u++) {
                    uint64_t q[2];
                    load_unit(src + p.head + 16u * u, q[0], q[1]);
                    std::memcpy(__builtin_assume_aligned(dst + p.head + 16u * u, 16), q, 16);
                }
                for (uint32_t t = 0; t < p.tail; t++) {
                    const uint64_t at = p.head + 16u * p.units + t;
                    dst[at] = src[at];
                }
                if (std::memcmp(base, want.data(), want.size()) != 0) fail("the copy differs from memcpy");
                std::free(sp);
                std::free(dp);
            }
    std::printf("{\"cases\": %u}\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: window_host_main positions|cover|copy ...");
    if (!std::strcmp(argv[1], "positions")) return run_positions(argc, argv);
    if (!std::strcmp(argv[1], "cover")) return run_cover(argc, argv);
    if (!std::strcmp(argv[1], "copy")) return run_copy();
    fail("unknown mode");
}
