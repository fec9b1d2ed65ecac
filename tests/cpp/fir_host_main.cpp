// fir_host_main.cpp -- the filter rule of zig-flac_amd/csrc/fg_fir.hpp on the host, built by
// tests/test_fir_host.py with -fsanitize=address,undefined.  Stand-alone: it includes the header the
// kernel includes and nothing of the library.  One JSON object on stdout.
//
//   rule T d start count x.bin h.bin y.bin    the rule over x (float32) by fir::element: y[t] for t < n,
//                                             +0.0f for the rest of the count
//   tile T d start count x.bin h.bin y.bin    the same window the way k_window_fir computes it: the
//                                             stage-1 span and the taps in heap blocks of exactly the
//                                             words the kernel may read, the LDS planes in blocks of
//                                             exactly fir_geometry's words, every tile, chunk, row and
//                                             column through the kernel's own index functions, one
//                                             fmaf a step in ascending u; counts the elements that
//                                             differ from the rule's, bit for bit
//   geometry                                  fir_geometry and the LDS layout over every T
//   valid offset taps delay rows reserved K taps_len     fir::filter_valid
//   span start count T d                      fir::span and fir::span_valid
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_fir.hpp"

using namespace fg;

static std::vector<float> read_f32(const char *path) {
    std::vector<float> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) std::exit(3);
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / 4u);
    if (n && std::fread(v.data(), 4, v.size(), f) != v.size()) std::exit(3);
    std::fclose(f);
    return v;
}

static void write_bytes(const char *path, const void *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f || (n && std::fwrite(p, 1, n, f) != n)) std::exit(3);
    std::fclose(f);
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static uint64_t delivered(uint64_t total, uint64_t start, uint64_t count) {
    if (start >= total) return 0;
    return start + count > total ? total - start : count;
}

struct Window {
    uint32_t T, d;
    uint64_t start, count;
    std::vector<float> x, h, y;
};

static bool read_window(int argc, char **argv, Window &w) {
    if (argc != 9) return false;
    w.T = (uint32_t)std::atoi(argv[2]);
    w.d = (uint32_t)std::atoi(argv[3]);
    w.start = std::strtoull(argv[4], nullptr, 10);
    w.count = std::strtoull(argv[5], nullptr, 10);
    w.x = read_f32(argv[6]);
    w.h = read_f32(argv[7]);
    const fir::Filter f{0u, w.T, w.d, 1u, 0u};
    if (!fir::filter_valid(f, 1u, w.h.size()) || w.h.size() != w.T || !fir::span_valid(w.count, w.T)) return false;
    w.y.assign(w.count, 0.0f);
    return true;
}

static float rule_element(const Window &w, uint64_t t) {
    return fir::element(w.h.data(), w.T, w.d, w.start, t,
                        [&](int64_t i) { return i >= 0 && (uint64_t)i < w.x.size() ? w.x[(size_t)i] : 0.0f; });
}

static int do_rule(int argc, char **argv) {
    Window w;
    if (!read_window(argc, argv, w)) return 2;
    const uint64_t n = delivered(w.x.size(), w.start, w.count);
    for (uint64_t t = 0; t < n; t++) w.y[t] = rule_element(w, t);
    write_bytes(argv[8], w.y.data(), w.y.size() * 4u);
    std::printf("{\"n\": %llu}\n", (unsigned long long)n);
    return 0;
}

static int do_tile(int argc, char **argv) {
    Window w;
    if (!read_window(argc, argv, w)) return 2;
    const uint64_t total = w.x.size(), n = delivered(total, w.start, w.count);
    const fir::Span sp = fir::span(w.start, w.count, w.T, w.d);
    // stage 1: the span's stored samples, zero past the stream's end, in a block of exactly s_count floats
    float *xp = new float[sp.count ? sp.count : 1u];
    for (uint64_t m = 0; m < sp.count; m++) xp[m] = sp.first + m < total ? w.x[(size_t)(sp.first + m)] : 0.0f;
    float *row = new float[w.T];
    std::memcpy(row, w.h.data(), w.T * 4u);
    const FirGeometry g = fir_geometry(w.T);
    float *s_x = new float[g.plane], *s_h = new float[g.tap_words];
    const uint32_t n_steps = fir::steps(w.T), rows = g.tile / 16u;
    uint64_t differ = 0, steps_run = 0;
    std::vector<float> acc((size_t)g.tile);
    for (uint64_t t0 = 0; t0 < n; t0 += g.tile) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        uint32_t chunks = 0;
        for (uint32_t u0 = 0; u0 < n_steps; u0 += g.chunk, chunks++) {
            const int64_t lo = fir::stage_lo(t0, w.T, u0, g.chunk);
            for (uint32_t q = 0; q < g.span; q++) s_x[fir::lds_pos(q)] = fir::span_at(xp, sp.count, sp.clip, lo + q);
            for (uint32_t p = 0; p < g.tap_words; p++) s_h[p] = fir::tap_at(row, w.T, fir::stage_tap(u0, p));
            const uint32_t nu = n_steps - u0 < g.chunk ? n_steps - u0 : g.chunk;
            if (nu % 4u) return 4;
            for (uint32_t r = 0; r < rows; r++)
                for (uint32_t j = 0; j < 16u; j++)
                    for (uint32_t uu = 0; uu < nu; uu++) {
                        const float av = s_x[fir::lds_pos(fir::a_slot(r, uu, g.chunk))], bv = s_h[fir::b_slot(uu, j)];
                        acc[16u * r + j] = fmaf(av, bv, acc[16u * r + j]);
                    }
            steps_run += nu;
        }
        if (chunks != g.n_chunks) return 4;
        for (uint32_t e = 0; e < g.tile && t0 + e < n; e++) {
            const float v = fir::plus_zero(acc[e]);
            w.y[t0 + e] = v;
            if (!same_bits(v, rule_element(w, t0 + e))) differ++;
        }
    }
    delete[] xp;
    delete[] row;
    delete[] s_x;
    delete[] s_h;
    write_bytes(argv[8], w.y.data(), w.y.size() * 4u);
    std::printf("{\"n\": %llu, \"differ\": %llu, \"clip\": %u, \"s_count\": %llu, \"chunk\": %u, \"n_chunks\": %u, \"steps\": %llu}\n",
                (unsigned long long)n, (unsigned long long)differ, sp.clip, (unsigned long long)sp.count, g.chunk, g.n_chunks,
                (unsigned long long)steps_run);
    return 0;
}

static int do_geometry() {
    uint64_t bad = 0, conflicts = 0;
    uint32_t max_lds = 0, max_chunk = 0;
    const FirGeometry big = fir_geometry(fir::kMaxTaps);
    for (uint32_t T = 1; T <= fir::kMaxTaps; T++) {
        const FirGeometry g = fir_geometry(T);
        const uint32_t st = fir::steps(T);
        bool ok = g.waves == 4u && g.accs >= 2u && g.tile == g.waves * g.accs * 256u && g.chunk % 16u == 0u && g.chunk >= 16u &&
                  g.chunk <= kFirChunk && st >= T + fir::kPad && st % 4u == 0u && st < T + fir::kPad + 4u;
        ok = ok && (uint64_t)g.n_chunks * g.chunk >= st && (uint64_t)(g.n_chunks - 1u) * g.chunk < st;
        ok = ok && g.span == g.tile - 16u + g.chunk && g.plane == fir::lds_pos(g.span - 1u) + 1u && g.tap_words == g.chunk + fir::kPad;
        ok = ok && g.lds_bytes == (g.plane + g.tap_words) * 4u && g.lds_bytes <= kFirLdsBytes && g.lds_bytes <= big.lds_bytes;
        // the largest slots the kernel forms
        ok = ok && fir::a_slot(g.tile / 16u - 1u, 0u, g.chunk) == g.span - 1u && fir::b_slot(g.chunk - 1u, 15u) == g.tap_words - 1u;
        if (!ok) bad++;
        if (g.lds_bytes > max_lds) max_lds = g.lds_bytes;
        if (g.chunk > max_chunk) max_chunk = g.chunk;
    }
    // lds_pos is strictly increasing, and the 64 lanes of an A read (16 rows x 4 steps) touch 64 banks
    for (uint32_t q = 1; q < big.span; q++)
        if (fir::lds_pos(q) <= fir::lds_pos(q - 1u)) bad++;
    for (uint32_t chunk = 16u; chunk <= kFirChunk; chunk += 16u)
        for (uint32_t base = 0; base < big.tile / 16u; base += 16u)
            for (uint32_t uu0 = 0; uu0 < chunk; uu0 += 4u) {
                uint64_t seen = 0;
                for (uint32_t l = 0; l < 64u; l++) seen |= 1ull << (fir::lds_pos(fir::a_slot(base + (l & 15u), uu0 + (l >> 4), chunk)) & 63u);
                if (seen != ~0ull) conflicts++;
            }
    std::printf("{\"bad\": %llu, \"conflicts\": %llu, \"max_lds\": %u, \"max_chunk\": %u, \"tile\": %u, \"edge\": %u}\n",
                (unsigned long long)bad, (unsigned long long)conflicts, max_lds, max_chunk, big.tile, kFirChunk - fir::kPad);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "rule") return do_rule(argc, argv);
    if (mode == "tile") return do_tile(argc, argv);
    if (mode == "geometry") return do_geometry();
    if (mode == "valid" && argc == 9) {
        const fir::Filter f{std::strtoull(argv[2], nullptr, 10), (uint32_t)std::strtoul(argv[3], nullptr, 10),
                            (uint32_t)std::strtoul(argv[4], nullptr, 10), (uint32_t)std::strtoul(argv[5], nullptr, 10),
                            (uint32_t)std::strtoul(argv[6], nullptr, 10)};
        std::printf("{\"valid\": %d}\n", fir::filter_valid(f, (uint32_t)std::atoi(argv[7]), std::strtoull(argv[8], nullptr, 10)) ? 1 : 0);
        return 0;
    }
    if (mode == "span" && argc == 6) {
        const uint64_t start = std::strtoull(argv[2], nullptr, 10), count = std::strtoull(argv[3], nullptr, 10);
        const uint32_t T = (uint32_t)std::atoi(argv[4]), d = (uint32_t)std::atoi(argv[5]);
        const fir::Span s = fir::span(start, count, T, d);
        std::printf("{\"first\": %llu, \"count\": %llu, \"clip\": %u, \"valid\": %d}\n", (unsigned long long)s.first,
                    (unsigned long long)s.count, s.clip, fir::span_valid(count, T) ? 1 : 0);
        return 0;
    }
    return 2;
}
