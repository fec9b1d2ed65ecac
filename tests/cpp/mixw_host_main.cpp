// mixw_host_main.cpp -- the weighted channel mix of the delivery of sample windows (fg_deliver.hpp:
// mixw_valid, mixw_step, mixw_value, mixw_element) run entirely on the host.  A stand-alone program,
// built by tests/test_mixw_host.py with -fsanitize=address,undefined.
//
//   mixw_host_main valid IN
//       IN: records of 68 little-endian u32: C, K, FORMAT, NULL, then 64 weight bit patterns of
//       which the first K * C count (they are handed over in a buffer of exactly that size: a read
//       past it is a sanitizer error; NULL = 1 passes no weights at all).  Prints {"valid": [0 | 1 ...]}.
//   mixw_host_main elements BITS C K WEIGHTS IN OUT
//       WEIGHTS: K * C float32, row-major.  IN: little-endian int32 tuples of C samples of BITS bits.
//       The tuple is laid down as C channels of BITS / 8 bytes at an odd byte offset of a word buffer
//       that ends with its last word.  OUT gets, a tuple, K records of 8 bytes: the f32 bit pattern
//       (u32), the f16 one (u16), the bf16 one (u16) of mixw_element.  Prints {"count": n}.
//   mixw_host_main equiv
//       The equivalences, bit for bit, over every depth and C = 1..8 on seeded samples and the
//       limits: an identity matrix is element(); a row with one weight 1.0f is mix_element with
//       that channel's mask; {0.5, 0.5} on 16-bit stereo is the mask mean of both, here over every
//       pair of a set of 16-bit values that holds the limits.  Exit 1 on a difference.
//       Prints {"checked": count}.
//   mixw_host_main rows
//       For the three float formats, every destination alignment within 16 bytes that the element
//       size allows, 0-40 samples written, C in {1, 2, 3, 8}, K in {1, 2, 3}, planar and interleaved,
//       with and without padding: the tile's rows filled slot by slot by the kernel's own
//       fill_row_slot in a guarded buffer, with the element rule of k_window_elements<MIX_WEIGHTS>,
//       against the chain written out here from load_sample.  Prints {"cases": count}.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_deliver.hpp"

using namespace fg::deliver;

namespace {

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "mixw_host_main: %s\n", what);
    std::exit(1);
}

uint64_t u64(const char *s) { return std::strtoull(s, nullptr, 10); }

template <class T>
std::vector<T> read_all(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) fail("cannot open an input");
    std::vector<T> v;
    T x;
    while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

int run_valid(int argc, char **argv) {
    if (argc != 3) fail("usage: valid IN");
    const std::vector<uint32_t> in = read_all<uint32_t>(argv[2]);
    if (in.size() % 68u) fail("the input is no whole number of records");
    std::printf("{\"valid\": [");
    for (size_t a = 0; a < in.size(); a += 68u) {
        const uint32_t C = in[a], K = in[a + 1u], format = in[a + 2u];
        const size_t n = (C <= 8u && K <= 8u) ? (size_t)C * K : 0u;  // what a valid call reads
        float *w = (float *)std::malloc(n ? n * sizeof(float) : 1u);
        std::memcpy(w, &in[a + 4u], n * sizeof(float));
        std::printf("%s%d", a ? ", " : "", mixw_valid(C, K, in[a + 3u] ? nullptr : w, format) ? 1 : 0);
        std::free(w);
    }
    std::printf("]}\n");
    return 0;
}

int run_elements(int argc, char **argv) {
    if (argc != 8) fail("usage: elements BITS C K WEIGHTS IN OUT");
    const uint32_t bits = (uint32_t)u64(argv[2]), C = (uint32_t)u64(argv[3]), K = (uint32_t)u64(argv[4]), B = bits / 8u;
    if (bits != 8u && bits != 16u && bits != 24u && bits != 32u) fail("bits");
    if (C < 1u || C > 8u || K < 1u || K > 8u) fail("C or K");
    const std::vector<float> W = read_all<float>(argv[5]);
    if (W.size() != (size_t)K * C) fail("the weights are not K * C floats");
    if (!mixw_valid(C, K, W.data(), SAMPLE_F32)) fail("the weights are not valid");
    const std::vector<int32_t> in = read_all<int32_t>(argv[6]);
    if (in.size() % C) fail("the input is no whole number of tuples");
    std::FILE *o = std::fopen(argv[7], "wb");
    if (!o) fail("cannot open the output");
    constexpr uint32_t LEAD = 3;
    const size_t wbytes = ((size_t)LEAD + C * B + 3u) & ~(size_t)3u;
    uint32_t *words = (uint32_t *)std::malloc(wbytes);
    for (size_t i = 0; i < in.size(); i += C) {
        std::memset(words, 0xA5, wbytes);
        for (uint32_t c = 0; c < C; c++) std::memcpy((uint8_t *)words + LEAD + c * B, &in[i + c], B);  // little-endian host
        for (uint32_t k = 0; k < K; k++) {
            struct {
                uint32_t f32;
                uint16_t f16, bf16;
            } rec;
            const float *row = W.data() + (size_t)k * C;
            rec.f32 = mixw_element(words, LEAD, B, C, row, SAMPLE_F32);
            rec.f16 = (uint16_t)mixw_element(words, LEAD, B, C, row, SAMPLE_F16);
            rec.bf16 = (uint16_t)mixw_element(words, LEAD, B, C, row, SAMPLE_BF16);
            if (std::fwrite(&rec, 8, 1, o) != 1) fail("short write");
        }
    }
    std::free(words);
    std::fclose(o);
    std::printf("{\"count\": %zu}\n", in.size() / C);
    return 0;
}

uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int32_t sample_of(uint32_t &s, uint32_t bits, uint32_t i) {
    const int64_t lo = -((int64_t)1 << (bits - 1u)), hi = ((int64_t)1 << (bits - 1u)) - 1;
    if (i % 97u == 0u) return (int32_t)lo;
    if (i % 97u == 1u) return (int32_t)hi;
    if (i % 97u == 2u) return 0;
    const uint32_t sh = 32u - bits;
    return (int32_t)(lcg(s) << sh) >> sh;
}

int run_equiv() {
    uint64_t checked = 0;
    uint32_t seed = 12345u;
    constexpr uint32_t LEAD = 1;
    for (uint32_t bits = 8; bits <= 32u; bits += 8u)
        for (uint32_t C = 1; C <= 8u; C++) {
            const uint32_t B = bits / 8u;
            const size_t wbytes = ((size_t)LEAD + C * B + 3u) & ~(size_t)3u;
            uint32_t *words = (uint32_t *)std::malloc(wbytes);
            for (uint32_t i = 0; i < 4000u; i++) {
                int32_t x[8];
                std::memset(words, 0x5A, wbytes);
                for (uint32_t c = 0; c < C; c++) {
                    x[c] = sample_of(seed, bits, i + c);
                    std::memcpy((uint8_t *)words + LEAD + c * B, &x[c], B);
                }
                for (uint32_t k = 0; k < C; k++) {
                    float row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    row[k] = 1.0f;  // row k of the identity, and the one-weight row of channel k
                    if (!mixw_valid(C, 1u, row, SAMPLE_F32)) fail("a unit row is not valid");
                    for (uint32_t format = SAMPLE_F32; format < SAMPLE_FORMATS; format++, checked++) {
                        const uint32_t got = mixw_element(words, LEAD, B, C, row, format);
                        if (got != element(x[k], bits, format)) fail("an identity row is not element()");
                        if (got != mix_element(words, LEAD, B, 1u << k, format)) fail("a unit row is not that channel's mask");
                    }
                }
            }
            std::free(words);
        }
    // {0.5, 0.5} on 16-bit stereo against the mean mask 3
    std::vector<int32_t> vals = {-32768, -32767, -1, 0, 1, 2, 32766, 32767};
    for (uint32_t i = 0; i < 700u; i++) vals.push_back(sample_of(seed, 16u, 5u));
    const float half[2] = {0.5f, 0.5f};
    uint32_t *words = (uint32_t *)std::malloc(8);
    for (int32_t a : vals)
        for (int32_t b : vals) {
            std::memset(words, 0, 8);
            std::memcpy((uint8_t *)words + 1, &a, 2);
            std::memcpy((uint8_t *)words + 3, &b, 2);
            for (uint32_t format = SAMPLE_F32; format < SAMPLE_FORMATS; format++, checked++)
                if (mixw_element(words, 1u, 2u, 2u, half, format) != mix_element(words, 1u, 2u, 3u, format))
                    fail("{0.5, 0.5} is not the mask mean");
        }
    std::free(words);
    std::printf("{\"checked\": %llu}\n", (unsigned long long)checked);
    return 0;
}

// the weights of the rows run: for output channel k of K over C source channels, by turns silence,
// one channel, a pair with a difference and a dense row of thirds and odd factors
void row_weights(uint32_t C, uint32_t K, uint32_t k, float *w) {
    const uint32_t pick = (C + 2u * K + k) % 4u;
    for (uint32_t c = 0; c < C; c++) w[c] = 0.0f;
    if (pick == 0u && K > 1u) return;
    if (C == 1u || pick == 1u) {
        w[(k + K) % C] = pick == 1u ? 1.0f : -0.75f;
        return;
    }
    if (pick == 2u) {
        w[0] = 0.5f;
        w[C - 1u] = -0.5f;
        return;
    }
    for (uint32_t c = 0; c < C; c++) w[c] = (c & 1u ? -1.0f : 1.0f) / (float)(3u + c + k);
}

// the rule, channel by channel, from the bytes; std::fmaf is the correctly rounded operation
uint32_t plain_element(const uint8_t *sample, uint32_t B, uint32_t C, const float *w, uint32_t format) {
    float y = 0.0f;
    for (uint32_t c = 0; c < C; c++) {
        const float x = (float)load_sample(sample + c * B, B) * std::ldexp(1.0f, -(int)(8u * B - 1u));
        y = std::fmaf(w[c], x, y);
    }
    uint32_t f;
    std::memcpy(&f, &y, 4);
    if (format == SAMPLE_F32) return f;
    return format == SAMPLE_F16 ? f16_bits_wide(f) : bf16_bits(f);
}

int run_rows() {
    constexpr uint32_t PAD = 32, MAXLEN = 40, LEAD = 5;
    uint32_t cases = 0, dense = 0, zeros = 0;
    const uint32_t Cs[4] = {1, 2, 3, 8}, Ks[3] = {1, 2, 3};
    for (uint32_t format = SAMPLE_F32; format < SAMPLE_FORMATS; format++) {
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
                            float *W = (float *)std::malloc((size_t)K * C * sizeof(float));  // exactly K * C weights
                            for (uint32_t k = 0; k < K; k++) {
                                row_weights(C, K, k, W + (size_t)k * C);
                                uint32_t nz = 0;
                                for (uint32_t c = 0; c < C; c++) nz += W[(size_t)k * C + c] != 0.0f;
                                dense += nz > 2u;
                                zeros += nz == 0u;
                            }
                            if (!mixw_valid(C, K, W, format)) fail("the rows run made an invalid matrix");
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
                                    const uint32_t v =
                                        t < nsrc ? plain_element(raw + LEAD + t * per, B, C, W + (size_t)k * C, format) : 0u;
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
                                    return t < nsrc ? mixw_element(words, LEAD + t * per, B, C, W + (size_t)ch * C, format) : 0u;
                                };
                                const uint32_t max_units = row_elems / per_unit;
                                for (uint32_t k = 0; k < max_units + 2u; k++) fill_row_slot(row, row_elems, esz, k, max_units, elem);
                            }
                            if (std::memcmp(base, want.data(), size) != 0) fail("the rows differ from the rule element by element");
                            std::free(words);
                            std::free(W);
                            std::free(dp);
                        }
    }
    if (!dense || !zeros) fail("the rows run has no dense row or no silent channel");
    std::printf("{\"cases\": %u}\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: mixw_host_main valid|elements|equiv|rows ...");
    if (!std::strcmp(argv[1], "valid")) return run_valid(argc, argv);
    if (!std::strcmp(argv[1], "elements")) return run_elements(argc, argv);
    if (!std::strcmp(argv[1], "equiv")) return run_equiv();
    if (!std::strcmp(argv[1], "rows")) return run_rows();
    fail("unknown mode");
}
