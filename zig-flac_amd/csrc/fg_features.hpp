// fg_features.hpp -- the scalar rules of delivering sample windows as short-time power spectra,
// bare or folded onto the rows of a caller's filter bank, shared by the device kernel (k_features,
// fg_features.hip), the host layer (fg_dec_host.cpp, fg_dec_api.cpp) and the stand-alone host
// program of the tests (tests/cpp/features_host_main.cpp).  Compiles under hipcc and plain g++.
//
// With N = n_fft (even, 16 .. 2048), H = hop (1 .. N), B = N / 2 + 1 bins and R = n_rows (0 .. 256;
// 0: no filter bank, the rows are the B bins), the signal x is one output channel of the delivery
// as F32 ELEMENTS (fg_deliver.hpp; resampled by fg_resample.hpp where the rates differ), +0.0f
// outside [0, total).  Frame t of a window that starts at sample `start` is centred at
// q = start + t * H and reads xf[n] = x[q - N / 2 + n], n < N.  The table, in double, rounded once:
//   w[n] = 0.5 - 0.5 cos(2 pi n / N)                          (the periodic Hann window)
//   c[b][n] = (float)( w[n] * cos(2 pi ((b * n) mod N) / N))
//   s[b][n] = (float)(-w[n] * sin(2 pi ((b * n) mod N) / N))   (b * n reduced in integers)
// re_b and im_b are ONE chain of fused multiply-adds each, from +0.0f, in ascending n:
// re_b = fmaf(c[b][n], xf[n], re_b); P_b = fmaf(im_b, im_b, re_b * re_b), the product rounded to
// float first.  Row r of a filter bank F[R][B] is one more chain from +0.0f in ascending b:
// m_r = fmaf(F[r][b], P_b, m_r).  P is finite (|x| <= 4, so P < 2^28 * N^2), so a zero entry of F
// leaves the chain where it was, bit for bit: filter_row_skip may pass over it, and nothing else
// here may reassociate, split or shorten a chain.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fg_crc.hpp"       // FG_HD
#include "fg_deliver.hpp"   // the element formats and their narrowing
#include "fg_resample.hpp"  // skew, kLdsBytes

namespace fg {
namespace feat {

constexpr uint32_t kMinFft = 16, kMaxFft = 2048, kMaxRows = 256;
constexpr double kTwoPi = 6.28318530717958647692;

struct Params {  // = flacgpu_features
    uint32_t n_fft, hop, n_rows;
};

FG_HD bool valid(const Params &p) {
    return p.n_fft >= kMinFft && p.n_fft <= kMaxFft && (p.n_fft & 1u) == 0u && p.hop >= 1u && p.hop <= p.n_fft && p.n_rows <= kMaxRows;
}
FG_HD uint32_t bins(const Params &p) { return p.n_fft / 2u + 1u; }
FG_HD uint32_t rows(const Params &p) { return p.n_rows ? p.n_rows : bins(p); }

// the samples a window of `frames` frames reads: [start - N / 2, start - N / 2 + span)
FG_HD uint64_t span(const Params &p, uint64_t frames) { return frames ? (frames - 1u) * p.hop + p.n_fft : 0u; }

// the frames whose centre lies inside a stream of `total` samples
FG_HD uint64_t delivered(const Params &p, uint64_t total, uint64_t start, uint64_t frames) {
    if (start >= total) return 0;
    const uint64_t most = (total - start + p.hop - 1u) / p.hop;
    return frames < most ? frames : most;
}

// ---- the table (double, built on the host) -------------------------------------------------------
FG_HD double hann(uint32_t N, uint32_t n) { return 0.5 - 0.5 * cos(kTwoPi * (double)n / (double)N); }
// plane 0: c[b][n], plane 1: s[b][n]
FG_HD float table_entry(uint32_t N, uint32_t plane, uint32_t b, uint32_t n) {
    const double a = kTwoPi * (double)(((uint64_t)b * n) % N) / (double)N, w = hann(N, n);
    return plane == 0u ? (float)(w * cos(a)) : (float)(-w * sin(a));
}

// ---- a frame ------------------------------------------------------------------------------------------
// one chain: sum over n of row[n] * x(n), x(n) the frame's sample n
template <class X>
FG_HD float chain(const float *row, uint32_t N, X x) {
    float y = 0.0f;
    for (uint32_t n = 0; n < N; n++) y = fmaf(row[n], x(n), y);
    return y;
}

FG_HD float power(float re, float im) {
    const float rr = re * re;  // rounded to float before it enters the fused multiply-add
    return fmaf(im, im, rr);
}

// bin b of a frame; table: [2][B][N]
template <class X>
FG_HD float bin_power(const float *table, uint32_t N, uint32_t b, X x) {
    const uint32_t B = N / 2u + 1u;
    const float re = chain(table + (uint64_t)b * N, N, x), im = chain(table + ((uint64_t)B + b) * N, N, x);
    return power(re, im);
}

// a row of the filter bank over the B powers of a frame: every entry, in order
FG_HD float filter_row_dense(const float *f, const float *P, uint32_t B) {
    float m = 0.0f;
    for (uint32_t b = 0; b < B; b++) m = fmaf(f[b], P[b], m);
    return m;
}
// the same chain without its zero entries: fmaf(0, P, m) = m for a finite P (m is never -0.0f: it
// starts at +0.0f, and a sum that is exactly zero rounds to +0.0f), so the result is the same bit
// for bit
FG_HD float filter_row_skip(const float *f, const float *P, uint32_t B) {
    float m = 0.0f;
    for (uint32_t b = 0; b < B; b++)
        if (f[b] != 0.0f) m = fmaf(f[b], P[b], m);
    return m;
}

// ---- narrowing --------------------------------------------------------------------------------------
// A row's element in `format` (deliver::SAMPLE_F32, _F16, _BF16): 32 bits, or 16 in the low half.
// deliver::f16_bits is stated below 65520; linear power passes it (a full-scale tone at n_fft 2048
// has P = 2^18), and from 65520 on -- the tie between the largest f16 and 2^16, which goes to even --
// nearest-even gives infinity.  bf16 keeps the range of f32.  v is finite and not negative.
FG_HD uint32_t element(float v, uint32_t format) {
    union {
        float f;
        uint32_t u;
    } b;
    b.f = v;
    if (format == deliver::SAMPLE_F32) return b.u;
    if (format == deliver::SAMPLE_BF16) return deliver::bf16_bits(b.u);
    return (b.u & 0x7FFFFFFFu) >= 0x477FF000u ? ((b.u >> 16) & 0x8000u) | 0x7C00u : deliver::f16_bits(b.u);
}

}  // namespace feat

// ---- the tile of k_features --------------------------------------------------------------------------
// A workgroup of 4 waves takes `frames` consecutive frames of one window and channel.  Their span
// -- (frames - 1) * H + N samples -- lies in LDS as one plane skewed as the resampler's
// (resample::skew: lanes a hop apart do not meet on the few banks a hop of 32 k words would give).
// With a filter bank the tile's powers follow it as [Bp][p_stride] (Bp: B rounded up to 16;
// p_stride 48 for 32 frames, so that the 16 x 4 lanes of an operand read touch every bank twice).
// The tile is the largest of 32, 16, 8, 4, 2, 1 frames that fits kLdsBytes: 32 and 16 fill the 16
// rows of v_mfma_f32_16x16x4_f32 (two accumulator tiles or one), the smaller ones -- only where
// n_fft and the hop are large -- leave rows of it idle.  One frame always fits: 2112 + 1040 words.
struct FeatGeometry {
    uint32_t frames;     // of a tile
    uint32_t waves;      // of the workgroup
    uint32_t span;       // samples of the tile's plane
    uint32_t plane;      // words of the skewed plane
    uint32_t bins_pad;   // B rounded up to 16
    uint32_t p_stride;   // words between two bins' powers (0: no filter bank, no powers in LDS)
    uint32_t lds_bytes;
};

FG_HD FeatGeometry feat_geometry(uint32_t n_fft, uint32_t hop, uint32_t n_rows) {
    FeatGeometry g;
    g.waves = 4u;
    g.bins_pad = (n_fft / 2u + 1u + 15u) & ~15u;
    for (uint32_t tf = 32u;; tf >>= 1) {
        g.frames = tf;
        g.span = (tf - 1u) * hop + n_fft;
        g.plane = resample::skew(g.span - 1u) + 1u;
        g.p_stride = n_rows ? (tf == 32u ? 48u : tf) : 0u;
        g.lds_bytes = (g.plane + g.bins_pad * g.p_stride) * 4u;
        if (g.lds_bytes <= resample::kLdsBytes || tf == 1u) return g;
    }
}

// what the host hands k_features for one window
struct FeatWindow {
    uint64_t x_off;    // floats: channel k's samples from x_off + k * count of the stage-1 scratch
    uint64_t count;    // samples stage 1 delivered a channel: the span less `clip`
    uint64_t start;    // as the caller states it
    uint64_t out_off;  // elements
    uint32_t clip;     // samples of the span before the stream's start: zeros, not in the scratch
    uint32_t frames;
    uint32_t stream;
    uint32_t too_small;
};
static_assert(sizeof(FeatWindow) == 48, "FeatWindow layout");

}  // namespace fg
