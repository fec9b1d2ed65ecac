// fg_crc.hpp -- the table-free CRC-16 fold shared by the encode kernels (fg_device.hpp) and the
// decode kernels (fg_dec.hip), and by the host build of the decode core (fg_dec.hpp, plain g++).
#pragma once
#include <stdint.h>

// FG_HD: host+device under hipcc, plain inline under a host compiler
#ifndef FG_HD
#if defined(__HIPCC__)
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD inline
#endif
#endif

namespace fg {

// CRC-16/UMTS (crc16.zig: poly 0x8005, init 0) without tables.  P = z^16 + z^15 + z^2 + 1 = (z + 1)(z^15 + z + 1), so a residue
// mod P is the pair (residue mod Q = z^15 + z + 1, residue mod z + 1 = the parity of the
// message bits), recombined by CRT: r = A ^ (parity(A) != p ? Q : 0) (Q has three terms, so
// adding it flips the parity and keeps A mod Q).  Mod Q, z^15 = z + 1 folds 14 bits per
// shift/XOR step, so the per-lane CRC chain is VALU only -- no table gathers, whose random
// indices cost 2-3 LDS bank-conflict cycles each.  Frame words are big-endian (first byte in bits
// 31..24), so a word is the next 32 coefficients of the message polynomial.
FG_HD uint32_t q_fold(uint32_t t) {  // t < 2^32 -> same residue, < 2^18
    const uint32_t h = t >> 15;
    return (t & 0x7FFFu) ^ h ^ (h << 1);
}
// s * z^32 + W mod Q (z^32 = z^4 + z^2 mod Q); s < 2^18 in and out, not fully reduced
FG_HD uint32_t q_word(uint32_t s, uint32_t W) { return q_fold(W ^ (s << 4) ^ (s << 2)); }
// a * e mod Q, a and e < 2^15 (fully reduced): 15 terms accumulated in one register (once per
// frame per lane: few live registers matter more than the chain), one fold
FG_HD uint32_t q_mul(uint32_t a, uint32_t e) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 15; i++) r ^= (e << i) & (uint32_t)(-(int32_t)((a >> i) & 1u));
    return q_fold(r);
}
// (residue mod Q in bits 0..14, message parity in bit 16) -> CRC-16 register value
FG_HD uint32_t crc_from_q(uint32_t qp) {
    const uint32_t A = qp & 0x7FFFu;
    return A ^ (((__builtin_popcount(A) ^ (qp >> 16)) & 1u) ? 0x8003u : 0u);
}
// one lane's share of a frame CRC: words [va, va + n) of img (negative indices read as zero: the
// front padding of an init-0 CRC), times e = z^(16 + 32 * words after them) mod Q; parity in bit 16.
FG_HD uint32_t crc_lane_q(const uint32_t *img, int32_t va, uint32_t n, uint32_t e) {
    uint32_t s = 0, px = 0;
    // the padding words before the image leave an init-0 chain at 0: start past them instead of
    // testing every index (the test put each load under its own exec mask)
    for (uint32_t i = va < 0 ? (uint32_t)(-va) : 0u; i < n; i++) {
        const uint32_t w = img[va + (int32_t)i];
        s = q_word(s, w);
        px ^= w;
    }
    return q_mul(q_fold(s), e) | ((__builtin_popcount(px) & 1u) << 16);
}
// crc16.zig's byte step without a table: T[t] = t * z^16 mod P = (t << 1) ^ (t << 2) ^ (parity(t) ? Q : 0)
FG_HD uint32_t crc_byte_v(uint32_t crc, uint32_t b) {
    const uint32_t t = ((crc >> 8) ^ b) & 255u;
    return ((crc << 8) ^ (t << 1) ^ (t << 2) ^ ((__builtin_popcount(t) & 1u) ? 0x8003u : 0u)) & 0xFFFFu;
}
// a * b mod P for a, b < 2^16 without tables: the carry-less product mod Q plus its parity
FG_HD uint32_t crc_mulmod_v(uint32_t a, uint32_t b) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = (b << i) & (uint32_t)(-(int32_t)((a >> i) & 1u));
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; i++) t[i] ^= t[i + w];
    return crc_from_q(q_fold(q_fold(t[0])) | ((__builtin_popcount(t[0]) & 1u) << 16));
}

}  // namespace fg
