// fg_quantize.hpp -- the scalar rules of turning tensor elements into the PCM the encoder reads:
// the inverse of fg_deliver.hpp.  Shared by the device kernel (k_elements_pcm, fg_quantize.hip), the
// host layer (flacgpu_pcm_from_elements_host, fg_api.cpp) and the stand-alone host program of the
// tests (tests/cpp/quantize_host_main.cpp), which run the kernel's own PCM writer (write_unit).
// Compiles under hipcc and plain g++.
//
// An ELEMENT is one of the four formats of a delivery (SAMPLE_*): 32 bits, or 16 in the low half.
// Its SAMPLE of `bits` bits (8, 16, 24, 32) is, for a float format, the element widened to f32
// (exact), times 2^(bits-1) (a power of two: exact, or an overflow to +-inf), rounded to an integer
// to nearest-even, clamped to [-2^(bits-1), 2^(bits-1) - 1]; NaN is 0.  For SAMPLE_I32 it is the
// value, clamped to the same range.  An element whose value the clamp changed, or a NaN, is CLIPPED:
// 1.0 is, since a delivery only produces [-1, 1).  Every step is exact but the one rounding, so
// sample_of(deliver::element(s, bits, F), F, bits) == s wherever element() itself is exact: F32 up
// to 24 bits, F16 and BF16 at 8, I32 at every depth.
//
// The PCM of a stream of T samples of C channels is T * C interleaved samples of B = bits / 8 bytes,
// signed little-endian (what deliver::load_sample reads back, and the encoder's unpack, 8-bit
// included), from a 4-byte-aligned byte offset: the layout flacgpu_plan_create takes.  It is written
// in UNITS of 4 consecutive interleaved samples: 4 B bytes, B whole 32-bit words, so no depth needs a
// byte store or a read-modify-write.  The stream's last word is written whole, its pad bytes zero;
// nothing past the stream's length rounded up to 4 is touched.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fg_crc.hpp"  // FG_HD
#include "fg_deliver.hpp"

namespace fg {
namespace quantize {

using deliver::SAMPLE_BF16;
using deliver::SAMPLE_F16;
using deliver::SAMPLE_F32;
using deliver::SAMPLE_FORMATS;
using deliver::SAMPLE_I32;

constexpr uint32_t kMaxStreams = 65535;  // of one launch: the stream is blockIdx.y
constexpr uint32_t kUnitSamples = 4;

// One stream of a launch (device table): `src` its elements at any element alignment, T samples a
// channel; planar sources hold channel c's sample t at c * plane_stride + t (plane_stride >= T),
// interleaved ones at t * C + c.  The PCM starts pcm_off bytes into the call's buffer.
struct Stream {
    const void *src;
    uint64_t samples, plane_stride, pcm_off;
};

struct Sample {
    int32_t s;
    uint32_t clipped;  // 0 or 1
};

// f16 -> f32 as bit patterns: exact (subnormals through an exact int -> float conversion and a
// power-of-two scale; infinities and NaNs keep their class)
FG_HD uint32_t f16_to_f32_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 31u) return sign | 0x7F800000u | (m << 13);
    if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
    union {
        float f;
        uint32_t u;
    } v, sc;
    sc.u = (127u - 24u) << 23;  // 2^-24, the unit of an f16 subnormal
    v.f = (float)m * sc.f;
    return sign | v.u;
}

// the element as f32 (float formats only)
FG_HD float widen(uint32_t element, uint32_t format) {
    union {
        float f;
        uint32_t u;
    } v;
    v.u = format == SAMPLE_F32 ? element : (format == SAMPLE_F16 ? f16_to_f32_bits(element & 0xFFFFu) : (element & 0xFFFFu) << 16);
    return v.f;
}

// The rule.  The upper limit 2^(bits-1) - 1 is no f32 at 32 bits, so the clamp compares the rounded
// value r with the two powers of two before the conversion: r is an integer, r >= 2^(bits-1) is
// r > limit, and no float -> int conversion sees a value outside [-2^(bits-1), 2^(bits-1) - 1].
FG_HD Sample sample_of(uint32_t element, uint32_t format, uint32_t bits) {
    const int32_t lo = (int32_t)(0xFFFFFFFFu << (bits - 1u)), hi = (int32_t)~(0xFFFFFFFFu << (bits - 1u));
    if (format == SAMPLE_I32) {
        const int32_t x = (int32_t)element;
        if (x < lo) return {lo, 1u};
        if (x > hi) return {hi, 1u};
        return {x, 0u};
    }
    const float x = widen(element, format);
    if (x != x) return {0, 1u};
    union {
        float f;
        uint32_t u;
    } top;
    top.u = (127u + (bits - 1u)) << 23;  // 2^(bits-1)
    const float r = rintf(x * top.f);    // to nearest-even: the default mode on the host, v_rndne_f32 on the device
    if (r >= top.f) return {hi, 1u};
    if (r < -top.f) return {lo, 1u};
    return {(int32_t)r, 0u};  // -0.0 converts to 0
}

FG_HD uint64_t pcm_bytes(uint64_t n_interleaved, uint32_t B) { return n_interleaved * B; }
FG_HD uint64_t pcm_words(uint64_t n_interleaved, uint32_t B) { return (n_interleaved * B + 3u) >> 2; }
FG_HD uint64_t units(uint64_t n_interleaved) { return (n_interleaved + kUnitSamples - 1u) / kUnitSamples; }

// The PCM writer: unit u of a stream of n interleaved samples whose PCM starts at `words`.
// sample(j, i) is interleaved sample i = 4 u + j, j < 4, called for i < n only, in ascending order.
// The unit's B words, or as many of them as lie below pcm_words(n, B), are stored whole.
template <class SampleAt>
FG_HD void write_unit(uint32_t *words, uint64_t u, uint64_t n, uint32_t B, SampleAt sample) {
    const uint64_t i0 = u * kUnitSamples;
    const uint32_t mask = 0xFFFFFFFFu >> (32u - 8u * B);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < kUnitSamples; j++) {
        if (i0 + j >= n) break;
        const uint32_t v = (uint32_t)sample(j, i0 + j) & mask, bit = 8u * B * j, k = bit >> 5, sh = bit & 31u;
        w[k] |= v << sh;
        if (sh + 8u * B > 32u) w[k + 1u] |= v >> (32u - sh);
    }
    const uint64_t w0 = u * B, total = pcm_words(n, B);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
        if (k < B && w0 + k < total) words[w0 + k] = w[k];
}

// The source index of interleaved sample i = t * C + c.
FG_HD uint64_t source_index(uint64_t t, uint32_t c, uint32_t C, uint64_t plane_stride, bool planar) {
    return planar ? (uint64_t)c * plane_stride + t : t * C + c;
}

// The element at index e of a source in `format`: 32 bits, or 16 in the low half.
FG_HD uint32_t load_element(const void *src, uint64_t e, uint32_t format) {
    return deliver::elem_size(format) == 4u ? ((const uint32_t *)src)[e] : (uint32_t)((const uint16_t *)src)[e];
}

// Unit u of stream st: its samples from the source by the rule; returns the clipped elements.
// Idx is the integer the sample index is divided in: uint32_t where n < 2^32, else uint64_t.
template <class Idx>
FG_HD uint32_t convert_unit(const Stream &st, uint32_t *words, uint64_t u, uint64_t n, uint32_t C, uint32_t B, uint32_t format,
                            bool planar) {
    const Idx i0 = (Idx)(u * kUnitSamples);
    Idx t = i0 / (Idx)C;
    uint32_t c = (uint32_t)(i0 - t * (Idx)C), clipped = 0;
    write_unit(words, u, n, B, [&](uint32_t, uint64_t) {
        const Sample q = sample_of(load_element(st.src, source_index(t, c, C, st.plane_stride, planar), format), format, 8u * B);
        clipped += q.clipped;
        if (++c == C) {
            c = 0;
            t++;
        }
        return q.s;
    });
    return clipped;
}

}  // namespace quantize
}  // namespace fg
