// fg_deliver.hpp -- the scalar rules of delivering decoded sample windows as tensor elements,
// shared by the device kernel (k_window_elements in its three instantiations, fg_window.hip), the
// host layer (fg_dec_host.cpp) and the stand-alone host programs of the tests
// (tests/cpp/deliver_host_main.cpp, tests/cpp/mix_host_main.cpp, tests/cpp/mixw_host_main.cpp),
// which run the kernel's own row code (fill_row_slot).  Compiles under hipcc and plain g++.
//
// A SOURCE SAMPLE is the B = bits / 8 bytes at a byte address of any alignment: signed two's
// complement, little-endian, sign-extended to i32 -- what every decode call here writes to PCM,
// 8-bit included.  An ELEMENT is that sample in one of four formats (SAMPLE_*).  A window of
// `count` stated samples, n of them delivered after clipping, of C channels goes to a region of
// elements: sample t, channel c at t * C + c (interleaved) or c * count + t (DELIVER_PLANAR);
// with DELIVER_PAD the elements of t in [n, count) are written as zero.  A ROW is a run of
// consecutive destination elements (one plane, or the whole interleaved region); its ROW PLAN cuts
// it into the elements before the first 16-byte boundary, whole 16-byte units and the elements
// after them: the element-granular counterpart of window::copy_plan.  With a CHANNEL MIX the
// region has K output channels in place of C, each made of a set of source channels or, with
// WEIGHTS, of a weighted sum of all of them (below).
#pragma once
#include <stdint.h>

#include "fg_crc.hpp"  // FG_HD

namespace fg {
namespace deliver {

enum : uint32_t { SAMPLE_I32 = 0, SAMPLE_F32 = 1, SAMPLE_F16 = 2, SAMPLE_BF16 = 3, SAMPLE_FORMATS = 4 };  // = FLACGPU_SAMPLE_*
enum : uint32_t { DELIVER_PLANAR = 1, DELIVER_PAD = 2, DELIVER_FLAGS = 3 };                               // = FLACGPU_DELIVER_*
constexpr uint32_t SAMPLE_BYTES = 0xFFFFFFFFu;  // not an element format: the byte copy of flacgpu_decode_windows_device

constexpr uint32_t kMixMaxChannels = 8;  // output channels of a mix, and source channels of a mask

// The three modes of a delivery's `mix`: the source channels as they are, output channels made of
// channel masks, output channels made of a weight matrix.
enum : uint32_t { MIX_NONE = 0, MIX_MASKS = 1, MIX_WEIGHTS = 2 };

// How a window call delivers: `format` SAMPLE_BYTES copies the PCM bytes (k_window_copy, flags 0);
// any other format converts (k_window_elements<MIX_NONE>) or, with `mix` set, converts and mixes:
// out_channels output channels, output channel k made of the source channels whose bits masks[k]
// has (k_window_elements<MIX_MASKS>), or the weighted sum of all source channels by row k of
// `weights`, out_channels x channels floats, row-major, in DEVICE memory
// (k_window_elements<MIX_WEIGHTS>).  Without `mix` out_channels = channels and masks[k] = 1 << k.
struct Delivery {
    uint32_t format, flags, channels, sample_bytes;
    uint32_t mix, out_channels;
    uint8_t masks[kMixMaxChannels];
    const float *weights;
};

FG_HD Delivery identity_delivery(uint32_t format, uint32_t flags, uint32_t channels, uint32_t sample_bytes) {
    Delivery dv = {format, flags, channels, sample_bytes, MIX_NONE, channels, {0, 0, 0, 0, 0, 0, 0, 0}, nullptr};
    for (uint32_t k = 0; k < channels && k < kMixMaxChannels; k++) dv.masks[k] = (uint8_t)(1u << k);
    return dv;
}

FG_HD uint32_t elem_size(uint32_t format) { return format <= SAMPLE_F32 ? 4u : 2u; }

// the B bytes at p, any alignment, as a sign-extended little-endian integer
FG_HD int32_t load_sample(const uint8_t *p, uint32_t B) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < B; i++) v |= (uint32_t)p[i] << (8u * i);
    const uint32_t sh = 32u - 8u * B;
    return (int32_t)(v << sh) >> sh;
}

// The same sample out of little-endian 32-bit words: the B bytes at byte offset `off` of `words`.
// Only the words that hold one of those bytes are read.
FG_HD int32_t sample_in_words(const uint32_t *words, uint32_t off, uint32_t B) {
    const uint32_t i = off >> 2, r = off & 3u;
    uint64_t v = words[i];
    if (r + B > 4u) v |= (uint64_t)words[i + 1u] << 32;
    const uint32_t sh = 32u - 8u * B;
    return (int32_t)((uint32_t)(v >> (8u * r)) << sh) >> sh;
}

// (float)x * 2^-(bits-1) as its bit pattern.  The conversion rounds to nearest-even (inexact only
// for 32-bit samples with |x| >= 2^24); the scale is a power of two and a normal f32, so the
// product is exact.  The value lies in [-1, 1].
FG_HD uint32_t f32_bits(int32_t x, uint32_t bits) {
    union {
        float f;
        uint32_t u;
    } s, v;
    s.u = (127u - (bits - 1u)) << 23;
    v.f = (float)x * s.f;
    return v.u;
}

// f32 -> bf16, round to nearest-even, by integer arithmetic on the bit pattern (no NaN can occur)
FG_HD uint16_t bf16_bits(uint32_t f) { return (uint16_t)((f + 0x7FFFu + ((f >> 16) & 1u)) >> 16); }

// f32 -> f16, round to nearest-even, subnormal results kept, by integer arithmetic on the bit
// pattern; for |value| < 65520, where the result is finite (no overflow, no NaN): a sample is at
// most 1 in magnitude, a resampled one (fg_resample.hpp) below 4.
FG_HD uint16_t f16_bits(uint32_t f) {
    const uint32_t sign = (f >> 16) & 0x8000u, a = f & 0x7FFFFFFFu, e = a >> 23;
    if (e >= 113u) {  // >= 2^-14, a normal f16: a rounding that carries goes into the exponent field, as it should
        uint32_t r = a - (112u << 23);
        r += 0xFFFu + ((r >> 13) & 1u);
        return (uint16_t)(sign | (r >> 13));
    }
    if (e < 102u) return (uint16_t)sign;  // < 2^-25: rounds to zero
    // a subnormal f16, in units of 2^-24: m * 2^(e - 150) = m >> (126 - e)
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u, s = 126u - e;  // 14 <= s <= 24
    uint32_t q = m >> s;
    const uint32_t rem = m & ((1u << s) - 1u), half = 1u << (s - 1u);
    if (rem > half || (rem == half && (q & 1u))) q++;
    return (uint16_t)(sign | q);  // q = 0x400 is the smallest normal
}

// the element of sample x (of `bits` bits) in `format`: 32 bits, or 16 in the low half
FG_HD uint32_t element(int32_t x, uint32_t bits, uint32_t format) {
    if (format == SAMPLE_I32) return (uint32_t)x;
    const uint32_t f = f32_bits(x, bits);
    if (format == SAMPLE_F32) return f;
    return format == SAMPLE_F16 ? f16_bits(f) : bf16_bits(f);
}

// ---- the channel mix ----------------------------------------------------------------------------
// Output channel k of a mix is made of the m source channels in its mask (bit c: source channel c):
// m = 0 is silence (bit pattern 0), m = 1 that channel's element, m = 2, 4 or 8 the exact mean.
FG_HD uint32_t mask_count(uint32_t mask) {
    uint32_t m = 0;
    for (; mask; mask &= mask - 1u) m++;
    return m;
}

// A mix of K output channels over a source of C: K is 1 to 8, no mask has a bit at or above C,
// every mask holds 0, 1, 2, 4 or 8 channels, and SAMPLE_I32 -- which has no value for a mean -- at
// most one.
FG_HD bool mix_valid(uint32_t C, uint32_t K, const uint8_t *masks, uint32_t format) {
    if (!masks || C < 1u || C > kMixMaxChannels || K < 1u || K > kMixMaxChannels || format >= SAMPLE_FORMATS) return false;
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t m = mask_count(masks[k]);
        if ((uint32_t)masks[k] >> C) return false;
        if (m != 0u && m != 1u && m != 2u && m != 4u && m != 8u) return false;
        if (format == SAMPLE_I32 && m > 1u) return false;
    }
    return true;
}

// The mean of m = 2^log2m samples of `bits` bits whose exact sum is s (|s| <= 8 * 2^31), in a
// float `format`: (float)s * 2^-(bits - 1 + log2m).  s goes through double, which holds it exactly,
// so the one rounding -- to nearest-even, inexact only for |s| >= 2^24 -- is that of the double ->
// float conversion, the same instruction class on the host and the device; the scale is a normal
// power of two (>= 2^-34) and the product exact, in [-1, 1].
FG_HD uint32_t mean_element(int64_t s, uint32_t bits, uint32_t log2m, uint32_t format) {
    union {
        float f;
        uint32_t u;
    } sc, v;
    sc.u = (127u - (bits - 1u + log2m)) << 23;
    v.f = (float)(double)s * sc.f;
    if (format == SAMPLE_F32) return v.u;
    return format == SAMPLE_F16 ? f16_bits(v.u) : bf16_bits(v.u);
}

// Output channel `mask` of one sample whose C source channels are the B-byte samples from byte
// offset `off` of `words` on (sample_in_words): only the channels in the mask are read.
FG_HD uint32_t mix_element(const uint32_t *words, uint32_t off, uint32_t B, uint32_t mask, uint32_t format) {
    const uint32_t m = mask_count(mask);
    if (m == 0u) return 0u;
    int64_t s = 0;
    int32_t one = 0;
    for (uint32_t c = 0; mask >> c; c++)
        if ((mask >> c) & 1u) {
            one = sample_in_words(words, off + c * B, B);
            s += one;
        }
    if (m == 1u) return element(one, 8u * B, format);
    return mean_element(s, 8u * B, m == 2u ? 1u : (m == 4u ? 2u : 3u), format);
}

// ---- the weighted channel mix --------------------------------------------------------------------
// With weights, output channel k of a sample of C source channels is a chain over row k of a
// row-major K x C float matrix W.  With x_c the F32 element of source channel c (f32_bits),
//     y = +0.0f;  for c = 0 .. C-1 in this order:  y = fmaf(W[k][c], x_c, y)
// one accumulator and one correctly rounded fused multiply-add a source channel: the construction
// of resample::fir and of the feature chains.  SAMPLE_F32 is y, F16 and BF16 are y narrowed
// (f16_bits_wide, bf16_bits); SAMPLE_I32 is not offered.
//
// A weight is 0 (either sign) or has 2^-32 <= |w| <= 2^32, and these bounds are derived: |x_c| is 0
// or lies in [2^-31, 1] and is a multiple of 2^-31; a weight that is not 0 is a multiple of 2^-55
// (24 significant bits from 2^-32 up).  Every product is therefore 0 or a normal number, a multiple
// of 2^-86, of magnitude 2^-63 to 2^32; every partial sum is a multiple of 2^-86 of magnitude at
// most 8 * 2^32 = 2^35.  So no fused multiply-add underflows or overflows, none of its results is
// subnormal, and the only zero it gives is the exact cancellation, which to nearest-even is +0.0f:
// the accumulator starts at +0.0f and is never -0.0f.  With y never -0.0f, fmaf(w, x, y) = y bit
// for bit where w or x is zero (y + (+-0) = y), so passing over zero weights, and over channels
// whose x_c is 0, changes no bit: mixw_step skips a zero weight, and such a channel is not read.
FG_HD bool mixw_weight_valid(float w) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = w;
    const uint32_t a = v.u & 0x7FFFFFFFu;  // NaN and infinity lie above the upper bound, subnormals below the lower
    return a == 0u || (a >= ((127u - 32u) << 23) && a <= ((127u + 32u) << 23));
}

// A weight matrix of K rows over a source of C channels: C and K are 1 to 8, the format is a float
// one, every weight is valid.
FG_HD bool mixw_valid(uint32_t C, uint32_t K, const float *W, uint32_t format) {
    if (!W || C < 1u || C > kMixMaxChannels || K < 1u || K > kMixMaxChannels) return false;
    if (format != SAMPLE_F32 && format != SAMPLE_F16 && format != SAMPLE_BF16) return false;
    for (uint32_t i = 0; i < K * C; i++)
        if (!mixw_weight_valid(W[i])) return false;
    return true;
}

// One link of the chain: source sample s of `bits` bits under weight w onto the accumulator y.  The
// multiply-add is the explicit builtin; nothing else here can be contracted (the scale of f32_bits
// is an exact product and an operand of the multiplication, not of the sum).
FG_HD float mixw_step(float y, float w, int32_t s, uint32_t bits) {
    if (w == 0.0f) return y;
    union {
        float f;
        uint32_t u;
    } x;
    x.u = f32_bits(s, bits);
    return __builtin_fmaf(w, x.f, y);
}

// The chain over one row w[0 .. C) for the sample whose C source channels are the B-byte samples
// from byte offset `off` of `words` on (sample_in_words); a channel under a zero weight is not read.
FG_HD float mixw_value(const uint32_t *words, uint32_t off, uint32_t B, uint32_t C, const float *w) {
    float y = 0.0f;
    for (uint32_t c = 0; c < C; c++) {
        const float wc = w[c];
        if (wc != 0.0f) y = mixw_step(y, wc, sample_in_words(words, off + c * B, B), 8u * B);
    }
    return y;
}

// f16_bits for a value that can pass 65520 -- a weighted sample reaches 2^35, a resampled one four
// times that --: from 65520 on, the tie between the largest f16 and 2^16, nearest-even is infinity.
FG_HD uint16_t f16_bits_wide(uint32_t f) {
    return (f & 0x7FFFFFFFu) >= 0x477FF000u ? (uint16_t)(((f >> 16) & 0x8000u) | 0x7C00u) : f16_bits(f);
}

// y in a float `format`: 32 bits, or 16 in the low half
FG_HD uint32_t mixw_narrow(float y, uint32_t format) {
    union {
        float f;
        uint32_t u;
    } v;
    v.f = y;
    if (format == SAMPLE_F32) return v.u;
    return format == SAMPLE_F16 ? f16_bits_wide(v.u) : bf16_bits(v.u);
}

FG_HD uint32_t mixw_element(const uint32_t *words, uint32_t off, uint32_t B, uint32_t C, const float *w, uint32_t format) {
    return mixw_narrow(mixw_value(words, off, B, C, w), format);
}

// The capacity rule.  A window that delivers n of its `count` stated samples needs count * unit of
// its capacity under PLANAR or PAD (the layout is the stated one), else n * unit; unit = channels
// for a capacity in elements, channels * bytes per sample for one in bytes.  No product is formed,
// so count = 2^64 - 1 is too small and does not wrap; count = 0 needs nothing.
FG_HD bool too_small(uint64_t n, uint64_t count, uint32_t flags, uint64_t cap, uint32_t unit) {
    return ((flags & (DELIVER_PLANAR | DELIVER_PAD)) ? count : n) > cap / unit;
}

// The samples a clean window writes: all `count` under PAD, else the n delivered.
FG_HD uint64_t written_samples(uint64_t n, uint64_t count, uint32_t flags) { return (flags & DELIVER_PAD) ? count : n; }

// A row of n elements of esz (2 or 4) bytes at dst_addr (a multiple of esz): `head` elements up to
// the first 16-byte boundary (all of them where the row ends before it), `units` whole 16-byte
// units, `tail` elements after the last.
struct RowPlan {
    uint32_t head, tail;
    uint64_t units;
};
FG_HD RowPlan row_plan(uint64_t dst_addr, uint64_t n, uint32_t esz) {
    RowPlan p;
    const uint64_t to_boundary = ((16u - (dst_addr & 15u)) & 15u) / esz, per_unit = 16u / esz;
    p.head = (uint32_t)(to_boundary < n ? to_boundary : n);
    p.units = (n - p.head) / per_unit;
    p.tail = (uint32_t)((n - p.head) % per_unit);
    return p;
}

// ---- a row's slots ---------------------------------------------------------------------------------
// A row of row_elems elements is written as max_units + 2 independent SLOTS, max_units =
// row_elems / (16 / esz) -- no plan has more units --: slot k < max_units is whole unit k (nothing
// where the plan has fewer), slot max_units the head elements, the last slot the tail ones.
// elem(e) is row element e: 32 bits, or 16 in the low half.  k_window_elements gives a thread a
// slot; the host programs of the tests run the same function slot after slot.
struct alignas(16) Unit {
    uint32_t q[4];
};

FG_HD void store_element(uint8_t *row, uint64_t e, uint32_t esz, uint32_t v) {
    if (esz == 4u) ((uint32_t *)row)[e] = v;
    else ((uint16_t *)row)[e] = (uint16_t)v;
}

template <class Elem>
FG_HD void fill_row_slot(uint8_t *row, uint32_t row_elems, uint32_t esz, uint32_t k, uint32_t max_units, Elem elem) {
    const RowPlan p = row_plan((uint64_t)(uintptr_t)row, row_elems, esz);
    const uint32_t per_unit = 16u / esz;
    if (k < max_units) {
        if (k >= p.units) return;
        const uint32_t e0 = p.head + k * per_unit;
        Unit u;
        if (esz == 4u) {
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) u.q[j] = elem(e0 + j);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) u.q[j] = elem(e0 + 2u * j) | (elem(e0 + 2u * j + 1u) << 16);
        }
        *(Unit *)(row + (uint64_t)e0 * esz) = u;  // 16-byte aligned by the plan: one store
    } else if (k == max_units) {
        for (uint32_t e = 0; e < p.head; e++) store_element(row, e, esz, elem(e));
    } else {
        const uint32_t e1 = p.head + (uint32_t)p.units * per_unit;
        for (uint32_t e = e1; e < e1 + p.tail; e++) store_element(row, e, esz, elem(e));
    }
}

// ---- the tile of k_window_elements --------------------------------------------------------------
// A workgroup takes kTileBytes / per consecutive samples of one window (per = channels * bytes per
// sample <= 32, so at least 128): their source bytes go to LDS as the aligned 8-byte words that
// hold them, at most kTileWords.
constexpr uint32_t kTileBytes = 4096;
constexpr uint32_t kTileWords = (kTileBytes + 7u + 7u) / 8u;
FG_HD uint32_t tile_samples(uint32_t per) { return kTileBytes / per; }

}  // namespace deliver
}  // namespace fg
