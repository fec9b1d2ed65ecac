// quantize_host_main.cpp -- the scalar rules of turning tensor elements into the encoder's PCM
// (fg_quantize.hpp) run entirely on the host.  A stand-alone program, built by
// tests/test_quantize_host.py with -fsanitize=address,undefined.
//
//   quantize_host_main sample BITS FORMAT IN OUT
//       IN: elements of FORMAT (0 i32, 1 f32, 2 f16, 3 bf16) as little-endian u32 bit patterns, the
//       16-bit ones in the low half.  OUT gets 8 bytes an element: the sample of BITS bits (i32) and
//       whether it was clipped (u32).  Prints {"count": n, "clipped": total}.
//   quantize_host_main roundtrip BITS FORMAT FIRST LAST STEP
//       Every sample s of BITS bits from FIRST to LAST in steps of STEP, and LAST: s through
//       deliver::element and back through sample_of.  Prints {"count": n, "bad": samples that did
//       not come back as themselves or came back clipped}.
//   quantize_host_main rows FORMAT IN OUT (C B T PLANAR STRIDE) ...
//       IN: a pool of elements as in `sample`.  For every case a stream of T samples of C channels
//       of B bytes, planar with STRIDE elements between planes or interleaved, whose source is the
//       first elements of the pool in an allocation of exactly the elements it has, is written unit
//       by unit by the kernel's own writer (convert_unit over write_unit) into a buffer with 64 guard
//       bytes of 0xA5 on both sides.  OUT gets every case's whole buffer, guards included, one after
//       the other.  Prints {"cases": n, "clipped": [per case]}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_quantize.hpp"

using namespace fg::quantize;

namespace {

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "quantize_host_main: %s\n", what);
    std::exit(1);
}

int64_t i64(const char *s) { return std::strtoll(s, nullptr, 10); }

std::vector<uint32_t> read_u32(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) fail("cannot open the input");
    std::vector<uint32_t> in;
    uint32_t x;
    while (std::fread(&x, 4, 1, f) == 1) in.push_back(x);
    std::fclose(f);
    return in;
}

uint32_t depth(const char *s) {
    const uint32_t bits = (uint32_t)i64(s);
    if (bits != 8u && bits != 16u && bits != 24u && bits != 32u) fail("bits");
    return bits;
}

uint32_t fmt(const char *s) {
    const uint32_t format = (uint32_t)i64(s);
    if (format >= SAMPLE_FORMATS) fail("format");
    return format;
}

int run_sample(int argc, char **argv) {
    if (argc != 6) fail("usage: sample BITS FORMAT IN OUT");
    const uint32_t bits = depth(argv[2]), format = fmt(argv[3]);
    const std::vector<uint32_t> in = read_u32(argv[4]);
    std::FILE *o = std::fopen(argv[5], "wb");
    if (!o) fail("cannot open the output");
    uint64_t clipped = 0;
    for (uint32_t e : in) {
        const Sample q = sample_of(e, format, bits);
        clipped += q.clipped;
        if (std::fwrite(&q, 8, 1, o) != 1) fail("short write");
    }
    std::fclose(o);
    std::printf("{\"count\": %zu, \"clipped\": %llu}\n", in.size(), (unsigned long long)clipped);
    return 0;
}

int run_roundtrip(int argc, char **argv) {
    if (argc != 7) fail("usage: roundtrip BITS FORMAT FIRST LAST STEP");
    const uint32_t bits = depth(argv[2]), format = fmt(argv[3]);
    const int64_t first = i64(argv[4]), last = i64(argv[5]), step = i64(argv[6]);
    if (step < 1 || first > last || first < -(1ll << (bits - 1u)) || last > (1ll << (bits - 1u)) - 1) fail("range");
    uint64_t count = 0, bad = 0;
    auto one = [&](int64_t s) {
        const Sample q = sample_of(fg::deliver::element((int32_t)s, bits, format), format, bits);
        count++;
        if (q.s != (int32_t)s || q.clipped) bad++;
    };
    for (int64_t s = first; s < last; s += step) one(s);
    one(last);
    std::printf("{\"count\": %llu, \"bad\": %llu}\n", (unsigned long long)count, (unsigned long long)bad);
    return 0;
}

int run_rows(int argc, char **argv) {
    if (argc < 5 || (argc - 5) % 5) fail("usage: rows FORMAT IN OUT (C B T PLANAR STRIDE) ...");
    constexpr size_t GUARD = 64;
    const uint32_t format = fmt(argv[2]);
    const std::vector<uint32_t> pool = read_u32(argv[3]);
    const uint32_t esz = fg::deliver::elem_size(format);
    std::FILE *o = std::fopen(argv[4], "wb");
    if (!o) fail("cannot open the output");
    std::printf("{\"clipped\": [");
    uint32_t cases = 0;
    for (int a = 5; a < argc; a += 5, cases++) {
        const uint32_t C = (uint32_t)i64(argv[a]), B = (uint32_t)i64(argv[a + 1]);
        const uint64_t T = (uint64_t)i64(argv[a + 2]), stride = (uint64_t)i64(argv[a + 4]);
        const bool planar = i64(argv[a + 3]) != 0;
        if (C < 1u || C > 8u || B < 1u || B > 4u || T < 1u || (planar && stride < T)) fail("a case's arguments");
        const uint64_t elems = planar ? (C - 1u) * stride + T : T * C;  // exactly the elements the source has
        if (elems > pool.size()) fail("the pool is too small");
        uint8_t *src = (uint8_t *)std::malloc(elems * esz);
        for (uint64_t e = 0; e < elems; e++) {
            if (esz == 4u) ((uint32_t *)src)[e] = pool[e];
            else ((uint16_t *)src)[e] = (uint16_t)pool[e];
        }
        const uint64_t n = T * C, span = pcm_words(n, B) * 4u;
        void *dp = nullptr;
        if (posix_memalign(&dp, 16, 2u * GUARD + span)) fail("no memory");
        uint8_t *base = (uint8_t *)dp;
        std::memset(base, 0xA5, 2u * GUARD + span);
        const Stream st{src, T, stride, 0};
        uint64_t clipped = 0;
        uint32_t *alt = (uint32_t *)std::malloc(span);  // the kernel's other index width: the same words
        for (uint64_t u = 0; u < units(n); u++) {
            clipped += convert_unit<uint64_t>(st, (uint32_t *)(base + GUARD), u, n, C, B, format, planar);
            convert_unit<uint32_t>(st, alt, u, n, C, B, format, planar);
        }
        if (std::memcmp(alt, base + GUARD, span) != 0) fail("the 32-bit index path differs from the 64-bit one");
        std::free(alt);
        if (std::fwrite(base, 1, 2u * GUARD + span, o) != 2u * GUARD + span) fail("short write");
        std::printf("%s%llu", cases ? ", " : "", (unsigned long long)clipped);
        std::free(src);
        std::free(dp);
    }
    std::fclose(o);
    std::printf("], \"cases\": %u}\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: quantize_host_main sample|roundtrip|rows ...");
    if (!std::strcmp(argv[1], "sample")) return run_sample(argc, argv);
    if (!std::strcmp(argv[1], "roundtrip")) return run_roundtrip(argc, argv);
    if (!std::strcmp(argv[1], "rows")) return run_rows(argc, argv);
    fail("unknown mode");
}
