// deliver_host_main.cpp -- the scalar rules of the delivery of sample windows as tensor elements
// (fg_deliver.hpp) run entirely on the host.  A stand-alone program, built by
// tests/test_deliver_host.py with -fsanitize=address,undefined.
//
//   deliver_host_main sample HEX
//       HEX: 32 bytes.  For B = 1..4 and every byte alignment 0-15 the sample at that address, by
//       load_sample and by sample_in_words (exit 1 where the two differ); each from an allocation
//       that ends with the sample's last byte (load_sample) or with the 32-bit word that holds it
//       (sample_in_words), so a read past either is a sanitizer error.
//       Prints {"samples": [[16 values] x 4]}.
//   deliver_host_main convert BITS IN OUT
//       IN: little-endian int32 samples of BITS bits.  OUT gets 8 bytes a sample: the f32 bit
//       pattern (u32), the f16 one (u16), the bf16 one (u16).  Prints {"count": n}.
//   deliver_host_main capacity (N COUNT FLAGS CAP UNIT) x M
//       Prints {"too_small": [0 | 1 ...]}.
//   deliver_host_main rows
//       For the formats i32, f32, f16 and bf16, every destination alignment within 16 bytes that the
//       element size allows and every row length 0-40: the row filled slot by slot by the kernel's
//       own fill_row_slot (head elements, whole 16-byte units, tail elements) in a guarded buffer
//       against the straightforward conversion element by element.  Prints {"cases": count}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_deliver.hpp"

using namespace fg::deliver;

namespace {

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "deliver_host_main: %s\n", what);
    std::exit(1);
}

uint64_t u64(const char *s) { return std::strtoull(s, nullptr, 10); }

int run_sample(int argc, char **argv) {
    if (argc != 3 || std::strlen(argv[2]) != 64) fail("usage: sample HEX (32 bytes)");
    uint8_t pat[32];
    for (int i = 0; i < 32; i++) {
        unsigned v;
        if (std::sscanf(argv[2] + 2 * i, "%2x", &v) != 1) fail("bad hex");
        pat[i] = (uint8_t)v;
    }
    std::printf("{\"samples\": [");
    for (uint32_t B = 1; B <= 4u; B++) {
        std::printf("%s[", B > 1 ? ", " : "");
        for (uint32_t al = 0; al < 16u; al++) {
            uint8_t *bytes = (uint8_t *)std::malloc(al + B);  // 16-byte aligned; ends with the sample's last byte
            std::memcpy(bytes, pat, al + B);
            const size_t wbytes = ((size_t)al + B + 3u) & ~(size_t)3u;  // ends with the word that holds it
            uint32_t *words = (uint32_t *)std::malloc(wbytes);
            std::memset(words, 0, wbytes);
            std::memcpy(words, pat, al + B);
            const int32_t a = load_sample(bytes + al, B), b = sample_in_words(words, al, B);
            if (a != b) fail("sample_in_words differs from load_sample");
            std::printf("%s%d", al ? ", " : "", a);
            std::free(bytes);
            std::free(words);
        }
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

int run_convert(int argc, char **argv) {
    if (argc != 5) fail("usage: convert BITS IN OUT");
    const uint32_t bits = (uint32_t)u64(argv[2]);
    if (bits != 8u && bits != 16u && bits != 24u && bits != 32u) fail("bits");
    std::FILE *f = std::fopen(argv[3], "rb");
    if (!f) fail("cannot open the input");
    std::vector<int32_t> in;
    int32_t x;
    while (std::fread(&x, 4, 1, f) == 1) in.push_back(x);
    std::fclose(f);
    std::FILE *o = std::fopen(argv[4], "wb");
    if (!o) fail("cannot open the output");
    for (int32_t v : in) {
        struct {
            uint32_t f32;
            uint16_t f16, bf16;
        } rec;
        rec.f32 = element(v, bits, SAMPLE_F32);
        rec.f16 = (uint16_t)element(v, bits, SAMPLE_F16);
        rec.bf16 = (uint16_t)element(v, bits, SAMPLE_BF16);
        if (element(v, bits, SAMPLE_I32) != (uint32_t)v) fail("the i32 element is not the sample");
        if (std::fwrite(&rec, 8, 1, o) != 1) fail("short write");
    }
    std::fclose(o);
    std::printf("{\"count\": %zu}\n", in.size());
    return 0;
}

int run_capacity(int argc, char **argv) {
    if ((argc - 2) % 5) fail("usage: capacity (N COUNT FLAGS CAP UNIT) ...");
    std::printf("{\"too_small\": [");
    for (int a = 2; a < argc; a += 5)
        std::printf("%s%d", a > 2 ? ", " : "",
                    too_small(u64(argv[a]), u64(argv[a + 1]), (uint32_t)u64(argv[a + 2]), u64(argv[a + 3]), (uint32_t)u64(argv[a + 4])) ? 1 : 0);
    std::printf("]}\n");
    return 0;
}

int run_rows() {
    constexpr uint32_t PAD = 32, MAXLEN = 40, BITS = 16, B = 2;
    uint32_t cases = 0;
    // 16-bit samples at an odd byte offset of a word buffer that ends with their last word
    constexpr uint32_t LEAD = 3;
    const size_t wbytes = ((size_t)LEAD + MAXLEN * B + 3u) & ~(size_t)3u;
    for (uint32_t format = 0; format < SAMPLE_FORMATS; format++) {
        const uint32_t esz = elem_size(format);
        for (uint32_t da = 0; da < 16u; da += esz)
            for (uint32_t len = 0; len <= MAXLEN; len++, cases++) {
                uint32_t *words = (uint32_t *)std::malloc(wbytes);
                uint8_t *raw = (uint8_t *)words;
                for (size_t i = 0; i < wbytes; i++) raw[i] = (uint8_t)(i * 89u + da * 7u + len * 13u + format + 1u);
                void *dp = nullptr;
                const size_t size = 2u * PAD + MAXLEN * 4u + 16u;
                if (posix_memalign(&dp, 16, size)) fail("no memory");
                uint8_t *base = (uint8_t *)dp, *dst = base + PAD + da;
                std::vector<uint8_t> want(size, 0xA5);
                std::memset(base, 0xA5, size);
                auto elem = [&](uint32_t e) { return element(sample_in_words(words, LEAD + e * B, B), BITS, format); };
                for (uint32_t e = 0; e < len; e++) {  // the straightforward conversion
                    const uint32_t v = element(load_sample(raw + LEAD + e * B, B), BITS, format);
                    std::memcpy(want.data() + PAD + da + (size_t)e * esz, &v, esz);  // little-endian host
                }
                const RowPlan p = row_plan((uint64_t)(uintptr_t)dst, len, esz);
                const uint32_t per_unit = 16u / esz;
                if (p.head >= per_unit || p.tail >= per_unit || p.head + per_unit * p.units + p.tail != len)
                    fail("the plan does not add up");
                if ((p.units || p.tail) && ((uintptr_t)(dst + p.head * esz) & 15u)) fail("a unit is not aligned");
                // the row as the kernel fills it: every slot, by the kernel's own function
                const uint32_t max_units = len / per_unit;
                for (uint32_t k = 0; k < max_units + 2u; k++) fill_row_slot(dst, len, esz, k, max_units, elem);
                if (std::memcmp(base, want.data(), size) != 0) fail("the row differs from the straightforward conversion");
                std::free(words);
                std::free(dp);
            }
    }
    std::printf("{\"cases\": %u}\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: deliver_host_main sample|convert|capacity|rows ...");
    if (!std::strcmp(argv[1], "sample")) return run_sample(argc, argv);
    if (!std::strcmp(argv[1], "convert")) return run_convert(argc, argv);
    if (!std::strcmp(argv[1], "capacity")) return run_capacity(argc, argv);
    if (!std::strcmp(argv[1], "rows")) return run_rows();
    fail("unknown mode");
}
