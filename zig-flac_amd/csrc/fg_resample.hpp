// fg_resample.hpp -- the scalar rules of delivering decoded sample windows at another sample rate,
// shared by the device kernel (k_window_resample in its two instantiations, fg_resample.hip), the
// host layer (fg_dec_host.cpp, fg_dec_api.cpp) and the stand-alone host program of the tests
// (tests/cpp/resample_host_main.cpp).  Compiles under hipcc and plain g++.
//
// A source of rate Rs is delivered at rate Rd by a polyphase windowed-sinc FIR: with g = gcd(Rs, Rd),
// L = Rd / g and M = Rs / g, output sample n sits at source position n * M / L = i0 + p / L
// (i0 = n * M div L, p = n * M mod L) and is the sum of T = 2 * Hw source samples around i0 weighted
// by row p of a table of L rows.  The source samples are the F32 ELEMENTS of fg_deliver.hpp (one
// channel, or the exact mean of a mask), zero outside [0, total).  The sum is ONE chain of fused
// multiply-adds in tap order from +0.0f, which is what makes the host and the device agree bit for
// bit: nothing here may reassociate it, split it or skip a zero tap.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fg_crc.hpp"  // FG_HD

namespace fg {
namespace resample {

constexpr uint32_t kZero = 24;       // zero crossings of the sinc on either side, at the filter's own cutoff
constexpr double kBeta = 9.0;        // of the Kaiser window
constexpr double kRolloff = 0.95;    // cutoff, as a part of the lower Nyquist
constexpr uint32_t kMaxFactor = 1024;  // L and M
constexpr uint32_t kMaxDecim = 12;     // M <= kMaxDecim * L
constexpr uint32_t kMaxTaps = 2u * kZero * kMaxDecim;  // 576

struct Ratio {
    uint32_t L, M;   // up by L, down by M
    uint32_t Hw, T;  // half width in source samples, taps = 2 * Hw
};

FG_HD uint32_t gcd32(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// The ratio of src_rate -> dst_rate, where it is one this filter serves: the rates differ, L and M
// are at most 1024 and the decimation at most 12.  Equal rates are no resampling.
FG_HD bool valid_ratio(uint32_t src_rate, uint32_t dst_rate, Ratio *out) {
    if (src_rate == 0u || dst_rate == 0u || src_rate == dst_rate) return false;
    const uint32_t g = gcd32(src_rate, dst_rate);
    const uint32_t L = dst_rate / g, M = src_rate / g;
    if (L > kMaxFactor || M > kMaxFactor || (uint64_t)M > (uint64_t)kMaxDecim * L) return false;
    if (out) {
        out->L = L;
        out->M = M;
        out->Hw = L >= M ? kZero : (kZero * M + L - 1u) / L;
        out->T = 2u * out->Hw;
    }
    return true;
}

// ---- the filter (double, built on the host) --------------------------------------------------------
// I0 by its power series, summed until a term no longer changes the sum
FG_HD double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (uint32_t m = 1; m < 1000u; m++) {
        term *= q / ((double)m * (double)m);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

FG_HD double sinc_pi(double t) {
    if (t == 0.0) return 1.0;
    const double y = 3.14159265358979323846 * t;
    return sin(y) / y;
}

// tap k of phase p before the row is normalised
FG_HD double raw_tap(const Ratio &r, uint32_t p, uint32_t k) {
    const double rho = r.L >= r.M ? 1.0 : (double)r.L / (double)r.M, c = kRolloff * rho;
    const double d = ((double)k - (double)r.Hw + 1.0) - (double)p / (double)r.L;
    const double u = d / (double)r.Hw;
    double a = 1.0 - u * u;
    if (a < 0.0) a = 0.0;
    return c * sinc_pi(c * d) * bessel_i0(kBeta * sqrt(a)) / bessel_i0(kBeta);
}

// Row p of the table: row[0 .. T), every tap divided by the row's sum (DC gain 1), then narrowed.
// row64 (T doubles) is the caller's work space.
FG_HD void filter_row(const Ratio &r, uint32_t p, double *row64, float *row) {
    double sum = 0.0;
    for (uint32_t k = 0; k < r.T; k++) {
        row64[k] = raw_tap(r, p, k);
        sum += row64[k];
    }
    for (uint32_t k = 0; k < r.T; k++) row[k] = (float)(row64[k] / sum);
}

// ---- positions -----------------------------------------------------------------------------------
// Output sample n (<= 2^40, with M <= 1024: no product passes 2^51) at i0 + p / L.
FG_HD uint64_t source_index(const Ratio &r, uint64_t n, uint32_t *p) {
    const uint64_t a = n * r.M;
    if (p) *p = (uint32_t)(a % r.L);
    return a / r.L;
}

// the output samples of a stream of `total` source samples
FG_HD uint64_t out_total(const Ratio &r, uint64_t total) { return (total * r.L + r.M - 1u) / r.M; }

// how many of the output samples [start, start + count) a stream of out_n delivers: the range is
// clipped, a sum that passes 64 bits is clipped and not wrapped
FG_HD uint64_t delivered(uint64_t out_n, uint64_t start, uint64_t count) {
    if (start >= out_n) return 0;
    const uint64_t end = (start + count < start || start + count > out_n) ? out_n : start + count;
    return end - start;
}

// The source samples [lo, hi) that output samples [start, start + n), all below out_total, need;
// nothing (0, 0) for n = 0.
FG_HD void source_range(const Ratio &r, uint64_t total, uint64_t start, uint64_t n, uint64_t *lo, uint64_t *hi) {
    *lo = *hi = 0;
    if (n == 0) return;
    const uint64_t first = source_index(r, start, nullptr), last = source_index(r, start + n - 1u, nullptr);
    *lo = first + 1u > r.Hw ? first + 1u - r.Hw : 0u;
    *hi = last + r.Hw + 1u < total ? last + r.Hw + 1u : total;
}

// ---- the sample ----------------------------------------------------------------------------------
// y = sum over k of row[k] * x(k), x(k) the float at source index i0 - Hw + 1 + k (the caller's
// functor gives +0.0f outside the stream): one accumulator, one fused multiply-add a tap, in order.
template <class X>
FG_HD float fir(const float *row, uint32_t T, X x) {
    float y = 0.0f;
    for (uint32_t k = 0; k < T; k++) y = fmaf(row[k], x(k), y);
    return y;
}

// ---- the tile of k_window_resample -----------------------------------------------------------------
// A workgroup takes `tile` consecutive output samples of one window.  Their source span -- at most
// (tile - 1) * M div L + 1 + T samples -- lies in LDS as K planes of F32 elements, one an output
// channel.  A plane is SKEWED: element i at word i + i / 32, one word of padding after every 32,
// so that lanes which read at an even stride of s words (a thread owns consecutive output samples,
// so s is a multiple of M) do not all meet on s / gcd(s, 32) of the 32 banks of a 4-byte read:
// strides of 2 to 32 words that are powers of two then touch 32 banks in a 32-lane half.
constexpr uint32_t kLdsBytes = 65536;
constexpr uint32_t kMaxTile = 1024;

FG_HD uint32_t skew(uint32_t i) { return i + (i >> 5); }

FG_HD uint32_t tile_span(const Ratio &r, uint32_t tile) { return (uint32_t)(((uint64_t)(tile - 1u) * r.M) / r.L) + 1u + r.T; }

struct TilePlan {
    uint32_t tile;       // output samples of a tile
    uint32_t span;       // source samples of its planes
    uint32_t plane;      // words of one skewed plane
    uint32_t lds_bytes;  // K planes
};

// The largest tile of at most kMaxTile output samples whose K planes fit kLdsBytes.  One output
// sample always fits: its span is 1 + T <= 577 samples.
FG_HD TilePlan tile_plan(const Ratio &r, uint32_t K) {
    uint32_t lo = 1u, hi = kMaxTile;  // lo fits
    const uint32_t words = kLdsBytes / 4u / K;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (skew(tile_span(r, mid) - 1u) + 1u <= words) lo = mid;
        else hi = mid - 1u;
    }
    TilePlan t;
    t.tile = lo;
    t.span = tile_span(r, lo);
    t.plane = skew(t.span - 1u) + 1u;
    t.lds_bytes = t.plane * 4u * K;
    return t;
}

}  // namespace resample
}  // namespace fg
