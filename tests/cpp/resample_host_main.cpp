// resample_host_main.cpp -- the resampling rule of the delivery of sample windows
// (fg_resample.hpp) run entirely on the host.  A stand-alone program, built by
// tests/test_resample_host.py with -fsanitize=address,undefined.
//
//   resample_host_main table SRC DST OUT
//       The coefficient table of SRC -> DST, L * T floats row-major, to OUT.
//       Prints {"valid": 1, "L": .., "M": .., "Hw": .., "T": ..} or {"valid": 0}.
//   resample_host_main samples SRC DST START COUNT IN OUT
//       IN: the float32 samples of one channel.  Output samples [START, START + COUNT) of the sample
//       rule to OUT as float32, computed twice: straight from the samples, and the way
//       k_window_resample does it -- tile after tile of tile_plan(K = 1), the tile's source span in a
//       skewed plane of exactly the plan's size, zeros where the span leaves the stream, read only
//       inside source_range of the window.  The two must agree bit for bit (exit 1 otherwise).
//       Prints {"n": delivered, "tiles": count}.
//   resample_host_main grid
//       For every ordered pair of the rate list: validity, and for the valid ones out_total, the
//       delivered count and source_range over totals {0, 1, Hw - 1, Hw, 5000}, starts {0, the
//       middle, out_total - 1, out_total, out_total + 7} and counts {0, 1, 100, 2^64 - 1}.
//       Prints {"pairs": [[src, dst, valid, L, M, Hw, T]], "rows": [[src, dst, total, start, count,
//       out_total, n, lo, hi]]}.
//   resample_host_main narrow IN OUT
//       IN: float32 values.  OUT: 4 bytes a value, f16_bits (u16) and bf16_bits (u16).
//   resample_host_main geometry
//       tile_plan for every valid pair of the rate list and K = 1..8.
//       Prints {"plans": [[L, M, T, K, tile, span, plane, lds_bytes]]}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_deliver.hpp"
#include "../../zig-flac_amd/csrc/fg_resample.hpp"

using namespace fg::resample;

namespace {

const uint32_t kRates[13] = {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000};

[[noreturn]] void fail(const char *what) {
    std::fprintf(stderr, "resample_host_main: %s\n", what);
    std::exit(1);
}

uint64_t u64(const char *s) { return std::strtoull(s, nullptr, 10); }

std::vector<float> read_floats(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) fail("cannot open the input");
    std::vector<float> v;
    float x;
    while (std::fread(&x, 4, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

// the table in a buffer of exactly L * T floats
float *make_table(const Ratio &r) {
    float *h = (float *)std::malloc((size_t)r.L * r.T * sizeof(float));
    double *row64 = (double *)std::malloc(r.T * sizeof(double));
    for (uint32_t p = 0; p < r.L; p++) filter_row(r, p, row64, h + (size_t)p * r.T);
    std::free(row64);
    return h;
}

int run_table(int argc, char **argv) {
    if (argc != 5) fail("usage: table SRC DST OUT");
    Ratio r;
    if (!valid_ratio((uint32_t)u64(argv[2]), (uint32_t)u64(argv[3]), &r)) {
        std::printf("{\"valid\": 0}\n");
        return 0;
    }
    float *h = make_table(r);
    std::FILE *o = std::fopen(argv[4], "wb");
    if (!o || std::fwrite(h, sizeof(float), (size_t)r.L * r.T, o) != (size_t)r.L * r.T) fail("cannot write the output");
    std::fclose(o);
    std::free(h);
    std::printf("{\"valid\": 1, \"L\": %u, \"M\": %u, \"Hw\": %u, \"T\": %u}\n", r.L, r.M, r.Hw, r.T);
    return 0;
}

int run_samples(int argc, char **argv) {
    if (argc != 8) fail("usage: samples SRC DST START COUNT IN OUT");
    Ratio r;
    if (!valid_ratio((uint32_t)u64(argv[2]), (uint32_t)u64(argv[3]), &r)) fail("invalid ratio");
    const uint64_t start = u64(argv[4]), count = u64(argv[5]);
    const std::vector<float> in = read_floats(argv[6]);
    const uint64_t total = in.size();
    float *x = (float *)std::malloc(total ? total * sizeof(float) : 1u);  // exactly the stream: a read outside is an error
    if (total) std::memcpy(x, in.data(), total * sizeof(float));
    float *h = make_table(r);
    const uint64_t n = delivered(out_total(r, total), start, count);
    std::vector<float> y(n), z(n);
    // straight from the samples
    for (uint64_t t = 0; t < n; t++) {
        uint32_t p;
        const int64_t first = (int64_t)source_index(r, start + t, &p) - (int64_t)r.Hw + 1;
        y[t] = fir(h + (size_t)p * r.T, r.T, [&](uint32_t k) {
            const int64_t i = first + (int64_t)k;
            return i >= 0 && (uint64_t)i < total ? x[i] : 0.0f;
        });
    }
    // the kernel's way
    uint64_t lo, hi, tiles = 0;
    source_range(r, total, start, n, &lo, &hi);
    if (hi > total || lo > hi) fail("the source range leaves the stream");
    const TilePlan tp = tile_plan(r, 1);
    for (uint64_t t0 = 0; t0 < n; t0 += tp.tile, tiles++) {
        const uint32_t nfir = (uint32_t)(n - t0 < tp.tile ? n - t0 : tp.tile);
        const uint64_t first = source_index(r, start + t0, nullptr), last = source_index(r, start + t0 + nfir - 1u, nullptr);
        const uint32_t len = (uint32_t)(last - first) + r.T;
        if (len > tp.span) fail("a tile's span passes the plan's");
        float *plane = (float *)std::malloc(tp.plane * sizeof(float));
        const int64_t s0 = (int64_t)first - (int64_t)r.Hw + 1;
        for (uint32_t j = 0; j < len; j++) {
            const int64_t i = s0 + (int64_t)j;
            plane[skew(j)] = (i >= (int64_t)lo && i < (int64_t)hi) ? x[i] : 0.0f;
        }
        for (uint32_t t = 0; t < nfir; t++) {
            uint32_t p;
            const uint32_t base = (uint32_t)(source_index(r, start + t0 + t, &p) - first);
            z[t0 + t] = fir(h + (size_t)p * r.T, r.T, [&](uint32_t k) { return plane[skew(base + k)]; });
        }
        std::free(plane);
    }
    if (n && std::memcmp(y.data(), z.data(), n * sizeof(float)) != 0) fail("the tiles differ from the rule sample by sample");
    std::FILE *o = std::fopen(argv[7], "wb");
    if (!o || (n && std::fwrite(y.data(), sizeof(float), n, o) != n)) fail("cannot write the output");
    std::fclose(o);
    std::free(h);
    std::free(x);
    std::printf("{\"n\": %llu, \"tiles\": %llu}\n", (unsigned long long)n, (unsigned long long)tiles);
    return 0;
}

int run_grid() {
    std::printf("{\"pairs\": [");
    bool firstp = true;
    for (uint32_t src : kRates)
        for (uint32_t dst : kRates) {
            Ratio r = {0, 0, 0, 0};
            const bool ok = valid_ratio(src, dst, &r);
            std::printf("%s[%u, %u, %d, %u, %u, %u, %u]", firstp ? "" : ", ", src, dst, ok ? 1 : 0, r.L, r.M, r.Hw, r.T);
            firstp = false;
        }
    std::printf("], \"rows\": [");
    bool firstr = true;
    for (uint32_t src : kRates)
        for (uint32_t dst : kRates) {
            Ratio r;
            if (!valid_ratio(src, dst, &r)) continue;
            const uint64_t totals[5] = {0, 1, r.Hw - 1u, r.Hw, 5000};
            for (uint64_t total : totals) {
                const uint64_t ot = out_total(r, total);
                const uint64_t starts[5] = {0, ot / 2u, ot ? ot - 1u : 0u, ot, ot + 7u};
                const uint64_t counts[4] = {0, 1, 100, ~0ull};
                for (uint64_t start : starts)
                    for (uint64_t count : counts) {
                        const uint64_t n = delivered(ot, start, count);
                        uint64_t lo, hi;
                        source_range(r, total, start, n, &lo, &hi);
                        std::printf("%s[%u, %u, %llu, %llu, %llu, %llu, %llu, %llu, %llu]", firstr ? "" : ", ", src, dst,
                                    (unsigned long long)total, (unsigned long long)start, (unsigned long long)count,
                                    (unsigned long long)ot, (unsigned long long)n, (unsigned long long)lo, (unsigned long long)hi);
                        firstr = false;
                    }
            }
        }
    std::printf("]}\n");
    return 0;
}

int run_narrow(int argc, char **argv) {
    if (argc != 4) fail("usage: narrow IN OUT");
    const std::vector<float> in = read_floats(argv[2]);
    std::FILE *o = std::fopen(argv[3], "wb");
    if (!o) fail("cannot open the output");
    for (float v : in) {
        uint32_t f;
        std::memcpy(&f, &v, 4);
        const uint16_t rec[2] = {fg::deliver::f16_bits(f), fg::deliver::bf16_bits(f)};
        if (std::fwrite(rec, 4, 1, o) != 1) fail("short write");
    }
    std::fclose(o);
    std::printf("{\"count\": %zu}\n", in.size());
    return 0;
}

int run_geometry() {
    std::printf("{\"plans\": [");
    bool first = true;
    for (uint32_t src : kRates)
        for (uint32_t dst : kRates) {
            Ratio r;
            if (!valid_ratio(src, dst, &r)) continue;
            for (uint32_t K = 1; K <= 8u; K++) {
                const TilePlan t = tile_plan(r, K);
                std::printf("%s[%u, %u, %u, %u, %u, %u, %u, %u]", first ? "" : ", ", r.L, r.M, r.T, K, t.tile, t.span, t.plane,
                            t.lds_bytes);
                first = false;
            }
        }
    std::printf("]}\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) fail("usage: resample_host_main table|samples|grid|narrow|geometry ...");
    if (!std::strcmp(argv[1], "table")) return run_table(argc, argv);
    if (!std::strcmp(argv[1], "samples")) return run_samples(argc, argv);
    if (!std::strcmp(argv[1], "grid")) return run_grid();
    if (!std::strcmp(argv[1], "narrow")) return run_narrow(argc, argv);
    if (!std::strcmp(argv[1], "geometry")) return run_geometry();
    fail("unknown mode");
}
