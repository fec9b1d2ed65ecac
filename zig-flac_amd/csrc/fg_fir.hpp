// fg_fir.hpp -- the scalar rules of delivering sample windows convolved with a per-window FIR filter,
// shared by the device kernel (k_window_fir, fg_fir.hip), the host layer (fg_dec_host.cpp,
// fg_dec_api.cpp) and the stand-alone host program of the tests (tests/cpp/fir_host_main.cpp).
// Compiles under hipcc and plain g++.
//
// The signal x is one output channel of the delivery as F32 ELEMENTS at the delivered rate
// (fg_deliver.hpp; resampled by fg_resample.hpp where the rates differ), +0.0f outside [0, total).
// A filter has T taps h[0 .. T), 1 <= T <= kMaxTaps, all finite, and a delay d, 0 <= d < T.  Element
// t of a window that starts at sample `start` is ONE chain of fused multiply-adds from +0.0f in
// ascending k:  y = fmaf(h[k], x[start + t + d - k], y),  k = 0 .. T - 1;  a y that is zero is
// delivered as +0.0f.  Nothing may reassociate, split, shorten or skip a step of a chain.  The only
// extra steps allowed are those of a tap index outside [0, T): a zero tap times a finite sample,
// which leaves every accumulator as it was -- but for -0.0f, which such a step after the chain's last
// may turn into +0.0f.  An accumulator is -0.0f only where a negative product or sum has underflowed
// to zero (|h x| below 2^-150: a subnormal tap, or an accumulator of a few 2^-149); the rule's last
// clause makes the delivered bits the same there too.  {1.0f} with d = 0 is the identity.
//
// The decomposition of k_window_fir: with c = 15 the product D = A . B over u ascending, where
// A[i][u] = x[tb + 16 i + c - u] and B[u][j] = h[u + j - c] (zero outside [0, T)), is
// D[i][j] = y[tb + 16 i + j]: a Toeplitz operand, T + 15 steps, 15 of them a zero tap in every
// column.  The window's stage-1 span holds x[start + d - (T - 1) + m] at span index m (its first
// `clip` entries, before the stream's start, are not stored), so A[i][u] is span index
// tb + 16 i + T + 14 - u.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fg_crc.hpp"      // FG_HD
#include "fg_deliver.hpp"  // the element formats and their narrowing

namespace fg {
namespace fir {

constexpr uint32_t kMaxTaps = 4096;
constexpr uint32_t kPad = 15;            // c: zero taps on either side of a column's T
constexpr uint64_t kMaxSpan = 1ull << 31;  // count + T - 1 stays below it

struct Filter {  // = flacgpu_fir
    uint64_t offset;  // floats into the taps; row r at offset + r * taps
    uint32_t taps, delay, rows, reserved;
};
static_assert(sizeof(Filter) == 24, "Filter layout");

// a filter of a call that delivers K channels from `taps_len` floats of taps
FG_HD bool filter_valid(const Filter &f, uint32_t K, uint64_t taps_len) {
    if (f.taps < 1u || f.taps > kMaxTaps || f.delay >= f.taps || f.reserved != 0u) return false;
    if (f.rows != 1u && f.rows != K) return false;
    const uint64_t need = (uint64_t)f.rows * f.taps;  // <= 8 * 4096
    return f.offset <= taps_len && need <= taps_len - f.offset;
}

// a window of `count` samples through a filter of T taps: its span stays below 2^31
FG_HD bool span_valid(uint64_t count, uint32_t T) { return count < kMaxSpan && count + T - 1u < kMaxSpan; }

// The stage-1 span of a window: the samples [start + d - (T - 1), start + count + d), of which the
// first `clip` lie before the stream's start.  first: where stage 1 starts; count: what it delivers.
struct Span {
    uint64_t first, count;
    uint32_t clip;
};
FG_HD Span span(uint64_t start, uint64_t count, uint32_t T, uint32_t d) {
    Span s;
    const uint32_t back = T - 1u - d;  // samples before `start` the first element reads
    s.clip = count && start < back ? (uint32_t)(back - start) : 0u;
    s.first = count && start >= back ? start - back : 0u;
    s.count = count ? count + T - 1u - s.clip : 0u;
    return s;
}

// the rule's last clause
FG_HD float plus_zero(float y) { return y == 0.0f ? 0.0f : y; }

// one element by the rule: x(i) the signal at sample i (int64: below 0 and past the end +0.0f)
template <class X>
FG_HD float element(const float *h, uint32_t T, uint32_t d, uint64_t start, uint64_t t, X x) {
    float y = 0.0f;
    const int64_t at = (int64_t)(start + t) + (int64_t)d;
    for (uint32_t k = 0; k < T; k++) y = fmaf(h[k], x(at - (int64_t)k), y);
    return plus_zero(y);
}

// ---- the operands of k_window_fir ------------------------------------------------------------------
// tap k of a row, zero outside [0, T): nothing outside the row is read
FG_HD float tap_at(const float *row, uint32_t T, int64_t k) { return k >= 0 && k < (int64_t)T ? row[k] : 0.0f; }
// span index m of a window's channel: xp its s_count stored samples, the `clip` before them and
// everything from clip + s_count on zero: nothing outside the s_count samples is read
FG_HD float span_at(const float *xp, uint64_t s_count, uint32_t clip, int64_t m) {
    return m >= (int64_t)clip && (uint64_t)(m - (int64_t)clip) < s_count ? xp[m - (int64_t)clip] : 0.0f;
}
// the u steps of a filter: T + 15, rounded up to the 4 of an instruction
FG_HD uint32_t steps(uint32_t T) { return (T + kPad + 3u) & ~3u; }

// A tile stages, for the chunk of steps [u0, u0 + chunk), the span indices lo .. lo + span - 1 as
// LDS slots q = 0 .. span - 1 and the taps u0 - 15 .. u0 + chunk - 1 as slots p = 0 .. chunk + 14.
FG_HD int64_t stage_lo(uint64_t t0, uint32_t T, uint32_t u0, uint32_t chunk) {
    return (int64_t)t0 + (int64_t)T + 14 - (int64_t)u0 - (int64_t)(chunk - 1u);
}
FG_HD int64_t stage_tap(uint32_t u0, uint32_t p) { return (int64_t)u0 + (int64_t)p - (int64_t)kPad; }
// A[row][u0 + uu] of the tile (row: 16 outputs) is slot a_slot, B[u0 + uu][j] is slot b_slot
FG_HD uint32_t a_slot(uint32_t row, uint32_t uu, uint32_t chunk) { return 16u * row + (chunk - 1u - uu); }
FG_HD uint32_t b_slot(uint32_t uu, uint32_t j) { return uu + j; }
// Where slot q lies in LDS: 4 words of skew every 16, so the 16 rows of an A read (16 slots apart)
// fall on banks 20 i mod 64 = 4 (5 i mod 16), all distinct, and the aligned group of 4 steps of the
// lanes' k fills the 4 banks between them: the 64 lanes of a read touch 64 banks.
FG_HD uint32_t lds_pos(uint32_t q) { return q + 4u * (q >> 4); }

}  // namespace fir

// ---- the tile of k_window_fir -------------------------------------------------------------------------
// A workgroup of 4 waves takes `tile` consecutive outputs of one window and channel; a wave holds
// `accs` accumulators of 16 x 16 outputs, independent of each other.  The taps run in chunks of
// `chunk` steps (a multiple of 16, at most kFirChunk), so the LDS does not grow with T: per chunk the
// tile's sample span (tile - 16 + chunk slots, skewed by fir::lds_pos) and chunk + 15 taps.
struct FirGeometry {
    uint32_t waves, accs;
    uint32_t tile;       // outputs of a workgroup's tile
    uint32_t chunk;      // u steps staged at a time
    uint32_t n_chunks;
    uint32_t span;       // sample slots staged a chunk
    uint32_t plane;      // words of the skewed sample plane
    uint32_t tap_words;  // chunk + 15
    uint32_t lds_bytes;
};
constexpr uint32_t kFirChunk = 256, kFirAccs = 2, kFirLdsBytes = 16384;

FG_HD FirGeometry fir_geometry(uint32_t taps) {
    FirGeometry g;
    g.waves = 4u;
    g.accs = kFirAccs;
    g.tile = g.waves * g.accs * 256u;
    const uint32_t st = fir::steps(taps), all = (st + 15u) & ~15u;
    g.chunk = all < kFirChunk ? all : kFirChunk;
    g.n_chunks = (st + g.chunk - 1u) / g.chunk;
    g.span = g.tile - 16u + g.chunk;
    g.plane = fir::lds_pos(g.span - 1u) + 1u;
    g.tap_words = g.chunk + fir::kPad;
    g.lds_bytes = (g.plane + g.tap_words) * 4u;
    return g;
}

// what the host hands k_window_fir for one window
struct FirWindow {
    uint64_t x_off;    // floats: channel k's stored span from x_off + k * s_count of the stage-1 scratch
    uint64_t s_count;  // samples stage 1 delivered a channel: the span less `clip`
    uint64_t start;    // as the caller states it
    uint64_t out_off;  // elements
    uint64_t cap;      // elements
    uint64_t tap_off;  // floats: the filter's row r at tap_off + r * taps
    uint32_t count;    // as the caller states it (below 2^31)
    uint32_t clip;     // samples of the span before the stream's start: zeros, not in the scratch
    uint32_t stream;
    uint32_t taps, rows, pad;
};
static_assert(sizeof(FirWindow) == 72, "FirWindow layout");

}  // namespace fg
