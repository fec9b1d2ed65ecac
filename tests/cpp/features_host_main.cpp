// features_host_main.cpp -- the feature rule of zig-flac_amd/csrc/fg_features.hpp on the host, built
// by tests/test_features_host.py with -fsanitize=address,undefined.  Stand-alone: it includes the
// header the kernel includes and nothing of the library.  One JSON object on stdout.
//
//   table N out.bin                              the [2][B][N] table by feat::table_entry
//   frames N H R start frames x.bin F.bin|- y.bin  the rule over x (float32): y [rows][frames]; inside, every
//                                                power against a plain double DFT under the bound of
//                                                tests/features_ref.py, and every filter row dense against
//                                                zero-skipping, bit for bit
//   narrow v.bin out.bin                         feat::element of every value as (f16, bf16) pairs
//   geometry                                     feat_geometry over the whole parameter domain
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_features.hpp"

using namespace fg;

static std::vector<float> read_f32(const char *path) {
    std::vector<float> v;
    if (std::string(path) == "-") return v;
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

static std::vector<float> table_of(uint32_t N) {
    const uint32_t B = N / 2u + 1u;
    std::vector<float> t((size_t)2u * B * N);
    for (uint32_t p = 0; p < 2u; p++)
        for (uint32_t b = 0; b < B; b++)
            for (uint32_t n = 0; n < N; n++) t[((size_t)p * B + b) * N + n] = feat::table_entry(N, p, b, n);
    return t;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static int do_frames(int argc, char **argv) {
    if (argc != 10) return 2;
    const feat::Params p{(uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4])};
    const uint64_t start = std::strtoull(argv[5], nullptr, 10), frames = std::strtoull(argv[6], nullptr, 10);
    if (!feat::valid(p)) return 2;
    const std::vector<float> x = read_f32(argv[7]), F = read_f32(argv[8]);
    const uint32_t N = p.n_fft, B = feat::bins(p), R = feat::rows(p);
    if (F.size() != (size_t)p.n_rows * B) return 2;
    const std::vector<float> table = table_of(N);
    std::vector<float> y((size_t)R * frames), xf(N), P(B);
    const double u = std::ldexp(1.0, -24), gN = N * u / (1.0 - N * u);
    uint64_t over_bound = 0, skip_differs = 0, zero_frames = 0;
    double worst = 0.0;
    for (uint64_t t = 0; t < frames; t++) {
        const int64_t first = (int64_t)(start + t * p.hop) - (int64_t)(N / 2u);
        bool any = false;
        for (uint32_t i = 0; i < N; i++) {
            const int64_t at = first + (int64_t)i;
            const bool in = at >= 0 && (uint64_t)at < x.size();
            xf[i] = in ? x[(size_t)at] : 0.0f;  // the zero extension at both ends
            any = any || in;
        }
        if (!any) zero_frames++;
        for (uint32_t b = 0; b < B; b++) {
            P[b] = feat::bin_power(table.data(), N, b, [&](uint32_t i) { return xf[i]; });
            // a plain double DFT with the window, and the bound of features_ref.py without its rfft term
            double re = 0.0, im = 0.0, sre = 0.0, sim = 0.0;
            for (uint32_t n = 0; n < N; n++) {
                const double a = feat::kTwoPi * (double)(((uint64_t)b * n) % N) / (double)N, w = feat::hann(N, n);
                re += w * std::cos(a) * xf[n];
                im += -w * std::sin(a) * xf[n];
                sre += std::fabs(w * std::cos(a) * xf[n]);
                sim += std::fabs(w * std::sin(a) * xf[n]);
            }
            // (the double sums above are themselves within N 2^-52 of their sums of magnitudes)
            const double lead = u + gN * (1.0 + u) + N * std::ldexp(1.0, -52), small = N * std::ldexp(1.0, -150);
            const double ere = lead * sre + small, eim = lead * sim + small;
            const double are = std::fabs(re) + ere, aim = std::fabs(im) + eim;
            const double eP = 2.0 * std::fabs(re) * ere + ere * ere + 2.0 * std::fabs(im) * eim + eim * eim + u * are * are +
                              u * ((1.0 + u) * are * are + aim * aim) + std::ldexp(1.0, -149);
            const double err = std::fabs((double)P[b] - (re * re + im * im));
            if (err > eP) over_bound++;
            if (eP > 0.0 && err / eP > worst) worst = err / eP;
            if (!any && !same_bits(P[b], 0.0f)) over_bound++;  // wholly outside: +0.0f
        }
        for (uint32_t r = 0; r < R; r++) {
            float v = P[r < B ? r : 0u];
            if (p.n_rows) {
                v = feat::filter_row_dense(F.data() + (size_t)r * B, P.data(), B);
                if (!same_bits(v, feat::filter_row_skip(F.data() + (size_t)r * B, P.data(), B))) skip_differs++;
            }
            y[(size_t)r * frames + t] = v;
        }
    }
    write_bytes(argv[9], y.data(), y.size() * 4u);
    std::printf("{\"rows\": %u, \"frames\": %llu, \"n\": %llu, \"over_bound\": %llu, \"skip_differs\": %llu, \"zero_frames\": %llu, "
                "\"worst\": %.6f}\n",
                R, (unsigned long long)frames, (unsigned long long)feat::delivered(p, x.size(), start, frames),
                (unsigned long long)over_bound, (unsigned long long)skip_differs, (unsigned long long)zero_frames, worst);
    return 0;
}

static int do_geometry() {
    // every even n_fft, every hop, with and without a filter bank (the plan depends on n_rows only through that)
    uint64_t checked = 0, bad = 0;
    uint32_t min_frames = 99, max_lds = 0, hist[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t N = feat::kMinFft; N <= feat::kMaxFft; N += 2u)
        for (uint32_t H = 1; H <= N; H++)
            for (uint32_t R = 0; R <= 256u; R += 128u) {
                const FeatGeometry g = feat_geometry(N, H, R);
                const uint32_t bp = (N / 2u + 1u + 15u) & ~15u;
                bool ok = g.lds_bytes <= 65536u && g.frames >= 1u && g.frames <= 32u && (g.frames & (g.frames - 1u)) == 0u && g.waves == 4u;
                ok = ok && g.span == (g.frames - 1u) * H + N && g.plane == resample::skew(g.span - 1u) + 1u && g.bins_pad == bp;
                ok = ok && g.p_stride == (R ? (g.frames == 32u ? 48u : g.frames) : 0u) && g.p_stride * (R ? 1u : 0u) >= (R ? g.frames : 0u);
                ok = ok && g.lds_bytes == (g.plane + bp * g.p_stride) * 4u;
                if (g.frames < 32u) {  // the largest such tile: twice the frames do not fit
                    const uint32_t f2 = g.frames * 2u, plane2 = resample::skew((f2 - 1u) * H + N - 1u) + 1u;
                    ok = ok && (plane2 + bp * (R ? (f2 == 32u ? 48u : f2) : 0u)) * 4u > 65536u;
                }
                if (!ok) bad++;
                checked++;
                if (g.frames < min_frames) min_frames = g.frames;
                if (g.lds_bytes > max_lds) max_lds = g.lds_bytes;
                for (uint32_t k = 0; k < 6u; k++)
                    if (g.frames == (1u << k)) hist[k]++;
            }
    const FeatGeometry a = feat_geometry(400, 160, 80), b = feat_geometry(2048, 2048, 0), c = feat_geometry(2048, 512, 128);
    std::printf("{\"checked\": %llu, \"bad\": %llu, \"min_frames\": %u, \"max_lds\": %u, \"hist\": [%u, %u, %u, %u, %u, %u], "
                "\"g400\": [%u, %u], \"g2048_2048\": [%u, %u], \"g2048_512_128\": [%u, %u]}\n",
                (unsigned long long)checked, (unsigned long long)bad, min_frames, max_lds, hist[0], hist[1], hist[2], hist[3], hist[4],
                hist[5], a.frames, a.lds_bytes, b.frames, b.lds_bytes, c.frames, c.lds_bytes);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "table" && argc == 4) {
        const uint32_t N = (uint32_t)std::atoi(argv[2]);
        if (!feat::valid(feat::Params{N, 1u, 0u})) return 2;
        const std::vector<float> t = table_of(N);
        write_bytes(argv[3], t.data(), t.size() * 4u);
        std::printf("{\"B\": %u, \"n\": %zu}\n", N / 2u + 1u, t.size());
        return 0;
    }
    if (mode == "frames") return do_frames(argc, argv);
    if (mode == "narrow" && argc == 4) {
        const std::vector<float> v = read_f32(argv[2]);
        std::vector<uint16_t> out(v.size() * 2u);
        for (size_t i = 0; i < v.size(); i++) {
            out[2u * i] = (uint16_t)feat::element(v[i], deliver::SAMPLE_F16);
            out[2u * i + 1u] = (uint16_t)feat::element(v[i], deliver::SAMPLE_BF16);
            uint32_t bits;
            std::memcpy(&bits, &v[i], 4);
            if (feat::element(v[i], deliver::SAMPLE_F32) != bits) return 4;
        }
        write_bytes(argv[3], out.data(), out.size() * 2u);
        std::printf("{\"count\": %zu}\n", v.size());
        return 0;
    }
    if (mode == "geometry") return do_geometry();
    return 2;
}
