// mix_host_main.cpp -- the channel mix of the delivery of sample windows (fg_deliver.hpp: mix_valid,
// mean_element, mix_element) run entirely on the host.  A stand-alone program, built by
// tests/test_mix_host.py with -fsanitize=address,undefined.
//
//   mix_host_main valid
//       mix_valid of the one-mask mix {mask} for every format, C = 1..8 and mask 0..255.
//       Prints {"valid": [[[256 x 0 | 1] x 8] x 4]}.
//   mix_host_main mixes (C FORMAT K NULL m0 ... m7) x M
//       mix_valid of whole mixes: K as given (0 and 9 included), eight masks of which the first K
//       count, NULL = 1 passes no masks at all.  Prints {"valid": [0 | 1 ...]}.
//   mix_host_main elements BITS M IN OUT
//       IN: little-endian int32 tuples of M samples of BITS bits.  The tuple is laid down as M
//       channels of BITS / 8 bytes at an odd byte offset of a word buffer that ends with its last
//       word, and mixed with the mask of all M.  OUT gets 8 bytes a tuple: the f32 bit pattern
//       (u32), the f16 one (u16), the bf16 one (u16).  For M = 1 every format, I32 included, must
//       equal element(); mask 0 must give 0 in every format (exit 1 otherwise).  Prints {"count": n}.
//   mix_host_main rows
//       For the four formats, every destination alignment within 16 bytes that the element size
//       allows, 0-40 samples written, C in {1, 2, 3, 8}, K in {1, 2, 3}, planar and interleaved,
//       with and without padding: the tile's rows filled slot by slot by the kernel's own
//       fill_row_slot (head elements, whole 16-byte units, tail elements) in a guarded buffer, with
//       the element rule of k_window_elements<true>, against the rule element by element from
//       load_sample.  Prints {"cases": count}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_deliver.hpp"

using namespace fg::deliver;

namespace {

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "mix_host_main: %s\n", what);
    std::exit(1);
}

uint64_t u64(const char *s) { return std::strtoull(s, nullptr, 10); }

int run_valid() {
    std::printf("{\"valid\": [");
    for (uint32_t format = 0; format < SAMPLE_FORMATS; format++) {
        std::printf("%s[", format ? ", " : "");
        for (uint32_t C = 1; C <= 8u; C++) {
            std::printf("%s[", C > 1u ? ", " : "");
            for (uint32_t mask = 0; mask < 256u; mask++) {
                uint8_t *one = (uint8_t *)std::malloc(1);  // a read of a second mask is a sanitizer error
                *one = (uint8_t)mask;
                std::printf("%s%d", mask ? ", " : "", mix_valid(C, 1, one, format) ? 1 : 0);
                std::free(one);
            }
            std::printf("]");
        }
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

int run_mixes(int argc, char **argv) {
    if ((argc - 2) % 12) fail("usage: mixes (C FORMAT K NULL m0 ... m7) ...");
    std::printf("{\"valid\": [");
    for (int a = 2; a < argc; a += 12) {
        const uint32_t C = (uint32_t)u64(argv[a]), format = (uint32_t)u64(argv[a + 1]), K = (uint32_t)u64(argv[a + 2]);
        uint8_t masks[8];
        for (int k = 0; k < 8; k++) masks[k] = (uint8_t)u64(argv[a + 4 + k]);
        std::printf("%s%d", a > 2 ? ", " : "", mix_valid(C, K, u64(argv[a + 3]) ? nullptr : masks, format) ? 1 : 0);
    }
    std::printf("]}\n");
    return 0;
}

int run_elements(int argc, char **argv) {
    if (argc != 6) fail("usage: elements BITS M IN OUT");
    const uint32_t bits = (uint32_t)u64(argv[2]), M = (uint32_t)u64(argv[3]), B = bits / 8u;
    if (bits != 8u && bits != 16u && bits != 24u && bits != 32u) fail("bits");
    if (M != 1u && M != 2u && M != 4u && M != 8u) fail("M");
    std::FILE *f = std::fopen(argv[4], "rb");
    if (!f) fail("cannot open the input");
    std::vector<int32_t> in;
    int32_t x;
    while (std::fread(&x, 4, 1, f) == 1) in.push_back(x);
    std::fclose(f);
    if (in.size() % M) fail("the input is no whole number of tuples");
    std::FILE *o = std::fopen(argv[5], "wb");
    if (!o) fail("cannot open the output");
    constexpr uint32_t LEAD = 3;
    const size_t wbytes = ((size_t)LEAD + M * B + 3u) & ~(size_t)3u;
    uint32_t *words = (uint32_t *)std::malloc(wbytes);
    const uint32_t mask = (1u << M) - 1u;
    for (size_t i = 0; i < in.size(); i += M) {
        std::memset(words, 0xA5, wbytes);
        for (uint32_t c = 0; c < M; c++) std::memcpy((uint8_t *)words + LEAD + c * B, &in[i + c], B);  // little-endian host
        struct {
            uint32_t f32;
            uint16_t f16, bf16;
        } rec;
        rec.f32 = mix_element(words, LEAD, B, mask, SAMPLE_F32);
        rec.f16 = (uint16_t)mix_element(words, LEAD, B, mask, SAMPLE_F16);
        rec.bf16 = (uint16_t)mix_element(words, LEAD, B, mask, SAMPLE_BF16);
        if (M == 1u)
            for (uint32_t format = 0; format < SAMPLE_FORMATS; format++)
                if (mix_element(words, LEAD, B, mask, format) != element(in[i], bits, format)) fail("m = 1 is not element()");
        for (uint32_t format = 0; format < SAMPLE_FORMATS; format++)
            if (mix_element(words, LEAD, B, 0u, format) != 0u) fail("m = 0 is not zero");
        if (std::fwrite(&rec, 8, 1, o) != 1) fail("short write");
    }
    std::free(words);
    std::fclose(o);
    std::printf("{\"count\": %zu}\n", in.size() / M);
    return 0;
}

// the masks of the rows run: for output channel k of K over C source channels, by turns silence,
// one channel, a pair and the widest mean C allows; I32 takes no mean
uint32_t row_mask(uint32_t C, uint32_t K, uint32_t k, uint32_t format) {
    const uint32_t pick = (C + 2u * K + k) % 4u;
    const uint32_t one = 1u << ((k + K) % C);
    if (pick == 0u && K > 1u) return 0u;
    if (format == SAMPLE_I32 || C == 1u || pick == 1u) return one;
    if (pick == 2u || C < 4u) return C == 2u ? 3u : (1u | (1u << (C - 1u)));  // a pair that is not adjacent where it can be
    return C == 8u ? (k & 1u ? 0xFFu : 0xB4u) : 0xFu;
}

// the rule, element by element, from the bytes
uint32_t plain_element(const uint8_t *sample, uint32_t B, uint32_t mask, uint32_t format) {
    int64_t s = 0;
    uint32_t m = 0;
    for (uint32_t c = 0; c < 8u; c++)
        if ((mask >> c) & 1u) {
            s += load_sample(sample + c * B, B);
            m++;
        }
    if (m == 0u) return 0u;
    if (m == 1u) return element((int32_t)s, 8u * B, format);
    return mean_element(s, 8u * B, m == 2u ? 1u : (m == 4u ? 2u : 3u), format);
}

int run_rows() {
    constexpr uint32_t PAD = 32, MAXLEN = 40, LEAD = 5;
    uint32_t cases = 0, means = 0, zeros = 0;
    const uint32_t Cs[4] = {1, 2, 3, 8}, Ks[3] = {1, 2, 3};
    for (uint32_t format = 0; format < SAMPLE_FORMATS; format++) {
        const uint32_t esz = elem_size(format), per_unit = 16u / esz;
        for (uint32_t ci = 0; ci < 4u; ci++)
            for (uint32_t ki = 0; ki < 3u; ki++)
                for (uint32_t flags = 0; flags <= DELIVER_FLAGS; flags++)
                    for (uint32_t da = 0; da < 16u; da += esz)
                        for (uint32_t len = 0; len <= MAXLEN; len++, cases++) {
                            const uint32_t C = Cs[ci], K = Ks[ki], B = 1u + (C + K + format) % 4u, per = C * B;
                            const bool planar = (flags & DELIVER_PLANAR) != 0, pad = (flags & DELIVER_PAD) != 0;
                            // ns samples are written, nsrc of them decoded; a plane is `count` elements
                            const uint32_t ns = len, nsrc = pad ? (2u * len) / 3u : len, count = pad ? len : len + 5u;
                            uint32_t masks[3];
                            uint8_t m8[3];
                            for (uint32_t k = 0; k < K; k++) m8[k] = (uint8_t)(masks[k] = row_mask(C, K, k, format));
                            if (!mix_valid(C, K, m8, format)) fail("the rows run made an invalid mix");
                            for (uint32_t k = 0; k < K; k++) {
                                means += mask_count(masks[k]) > 1u;
                                zeros += masks[k] == 0u;
                            }
                            // the source: nsrc samples at byte LEAD of a word buffer that ends with their last word
                            const size_t wbytes = ((size_t)LEAD + (size_t)nsrc * per + 3u) & ~(size_t)3u;
                            uint32_t *words = (uint32_t *)std::malloc(wbytes ? wbytes : 4u);
                            uint8_t *raw = (uint8_t *)words;
                            for (size_t i = 0; i < wbytes; i++) raw[i] = (uint8_t)(i * 89u + da * 7u + len * 13u + format + C + 1u);
                            void *dp = nullptr;
                            const size_t size = 2u * PAD + 3u * (MAXLEN + 5u) * 4u + 16u;
                            if (posix_memalign(&dp, 16, size)) fail("no memory");
                            uint8_t *base = (uint8_t *)dp, *dst = base + PAD + da;
                            std::vector<uint8_t> want(size, 0xA5);
                            std::memset(base, 0xA5, size);
                            for (uint32_t t = 0; t < ns; t++)
                                for (uint32_t k = 0; k < K; k++) {
                                    const uint32_t v = t < nsrc ? plain_element(raw + LEAD + t * per, B, masks[k], format) : 0u;
                                    const size_t at = planar ? (size_t)k * count + t : (size_t)t * K + k;
                                    std::memcpy(want.data() + PAD + da + at * esz, &v, esz);
                                }
                            // the tile as the kernel fills it (t0 = 0): every slot of every row, by the kernel's own function
                            const uint32_t rows = planar ? K : 1u, row_elems = planar ? ns : ns * K;
                            for (uint32_t r = 0; r < rows; r++) {
                                uint8_t *row = dst + (planar ? (size_t)r * count : 0u) * esz;
                                const RowPlan p = row_plan((uint64_t)(uintptr_t)row, row_elems, esz);
                                if (p.head >= per_unit || p.tail >= per_unit || p.head + per_unit * p.units + p.tail != row_elems)
                                    fail("the plan does not add up");
                                auto elem = [&](uint32_t e) {
                                    const uint32_t t = planar ? e : e / K, ch = planar ? r : e - t * K;
                                    return t < nsrc ? mix_element(words, LEAD + t * per, B, masks[ch], format) : 0u;
                                };
                                const uint32_t max_units = row_elems / per_unit;
                                for (uint32_t k = 0; k < max_units + 2u; k++) fill_row_slot(row, row_elems, esz, k, max_units, elem);
                            }
                            if (std::memcmp(base, want.data(), size) != 0) fail("the rows differ from the rule element by element");
                            std::free(words);
                            std::free(dp);
                        }
    }
    if (!means || !zeros) fail("the rows run has no mean or no silent channel");
    std::printf("{\"cases\": %u}\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: mix_host_main valid|mixes|elements|rows ...");
    if (!std::strcmp(argv[1], "valid")) return run_valid();
    if (!std::strcmp(argv[1], "mixes")) return run_mixes(argc, argv);
    if (!std::strcmp(argv[1], "elements")) return run_elements(argc, argv);
    if (!std::strcmp(argv[1], "rows")) return run_rows();
    fail("unknown mode");
}
