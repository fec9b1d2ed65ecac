// fg_levels.hpp -- the scalar rules of measuring the levels of decoded sample windows, shared by
// the device kernels (k_window_levels, k_levels_fold: fg_levels.hip), the host layer
// (fg_dec_host.cpp), the host statement (flacgpu_levels_host, fg_dec_api.cpp) and the stand-alone
// host program of the tests (tests/cpp/levels_host_main.cpp).  Compiles under hipcc and plain g++.
//
// A window of n samples of C channels is cut by a HOP h into ceil(n / h) BLOCKS: block j holds the
// window's samples [j * h, min((j + 1) * h, n)).  Of every block and channel three numbers are
// delivered: the PEAK max |x| (u32: |-2^31| fits), the SUM of x (i64, exact) and the ENERGY, the sum
// of x^2 as an exact unsigned 128-bit integer rounded ONCE to the nearest double, ties to even
// (u128_to_f64).  Every accumulator is an integer, so partial results (Acc) combine exactly in any
// order and the delivered bits depend on nothing but the samples.
#pragma once
#include <stdint.h>

#include "fg_deliver.hpp"

namespace fg {
namespace levels {

// The double nearest to lo + 2^64 hi, ties to even.  Below 2^64 that is the conversion of lo.  Above,
// the value is shifted right by s = its bit length - 64 with every bit shifted out ORed into bit 0:
// the 64-bit result has its top bit set, so the conversion rounds at bit 11, and the sticky bit 0
// lies below the rounding position and only says whether the rest is zero -- the rounding of the
// shifted value is that of the whole.  The scale 2^s (s <= 64) is exact.
FG_HD double u128_to_f64(uint64_t lo, uint64_t hi) {
    if (hi == 0) return (double)lo;
    const uint32_t s = 64u - (uint32_t)__builtin_clzll(hi);  // 1..64
    uint64_t v, lost;
    if (s == 64u) {
        v = hi;
        lost = lo;
    } else {
        v = (hi << (64u - s)) | (lo >> s);
        lost = lo << (64u - s);
    }
    v |= lost != 0 ? 1ull : 0ull;
    union {
        double d;
        uint64_t u;
    } scale;
    scale.u = (uint64_t)(1023u + s) << 52;
    return (double)v * scale.d;
}

// The exact partial result of some samples of one channel.
struct Acc {
    uint64_t e_lo, e_hi;  // the sum of squares, 128 bits
    int64_t sum;
    uint32_t peak, pad;
};
static_assert(sizeof(Acc) == 32, "Acc layout");

FG_HD Acc acc_zero() {
    Acc a = {0, 0, 0, 0, 0};
    return a;
}

FG_HD uint32_t magnitude(int32_t x) { return x < 0 ? 0u - (uint32_t)x : (uint32_t)x; }

FG_HD void acc_add(Acc &a, int32_t x) {
    const uint32_t m = magnitude(x);
    const uint64_t sq = (uint64_t)m * m;  // <= 2^62
    a.e_lo += sq;
    a.e_hi += a.e_lo < sq ? 1u : 0u;
    a.sum += x;
    a.peak = m > a.peak ? m : a.peak;
}

FG_HD void acc_merge(Acc &a, const Acc &b) {
    const uint64_t lo = a.e_lo + b.e_lo;
    a.e_hi += b.e_hi + (lo < b.e_lo ? 1u : 0u);
    a.e_lo = lo;
    a.sum += b.sum;
    a.peak = b.peak > a.peak ? b.peak : a.peak;
}

FG_HD double acc_energy(const Acc &a) { return u128_to_f64(a.e_lo, a.e_hi); }

// ---- the blocks ------------------------------------------------------------------------------------
FG_HD uint64_t n_blocks(uint64_t n, uint32_t hop) { return n / hop + (n % hop ? 1u : 0u); }
FG_HD uint64_t block_len(uint64_t n, uint32_t hop, uint64_t j) {
    const uint64_t left = n - j * hop;
    return left < hop ? left : hop;
}
constexpr uint32_t kMaxHop = 0x7FFFFFFFu;
// The capacity rule: a window of n samples needs C * ceil(n / hop) records.  n <= 2^40 where it is asked.
FG_HD bool too_small(uint64_t n, uint32_t hop, uint32_t C, uint64_t cap) { return n_blocks(n, hop) > cap / C; }

// ---- the tiles of k_window_levels -------------------------------------------------------------------
// A workgroup takes a TILE of at most T = deliver::tile_samples(per) consecutive samples of a window,
// staged in LDS as the aligned 8-byte words that hold them (tile_words), and a tile never crosses a
// block boundary it does not hold whole:
//   LV_LANES  hop < 64:       a tile is T / hop whole blocks, a thread takes a (block, channel)
//   LV_WAVES  64 <= hop < T:  a tile is T / hop whole blocks, a wave takes a block, lanes stride it
//   LV_PARTS  hop >= T:       a block is cut into P = ceil(hop / T) parts of T samples; a tile is one
//                             part, all threads stride it.  With P > 1 every (block, part) leaves one
//                             Acc a channel, which k_levels_fold sums.
enum : uint32_t { LV_LANES = 0, LV_WAVES = 1, LV_PARTS = 2 };
constexpr uint32_t kWave = 64;

struct Plan {
    uint32_t hop, T, mode, group;  // group: blocks of a tile (1 with LV_PARTS)
    uint64_t parts;                // P
};

FG_HD Plan plan(uint32_t hop, uint32_t per) {
    Plan p;
    p.hop = hop;
    p.T = deliver::tile_samples(per);
    if (hop >= p.T) {
        p.mode = LV_PARTS;
        p.group = 1;
        p.parts = ((uint64_t)hop + p.T - 1u) / p.T;
    } else {
        p.mode = hop < kWave ? LV_LANES : LV_WAVES;
        p.group = p.T / hop;
        p.parts = 1;
    }
    return p;
}

FG_HD uint64_t parts_of(uint64_t len, uint32_t T) { return (len + T - 1u) / T; }

// the tiles of a window of n samples
FG_HD uint64_t n_tiles(uint64_t n, const Plan &p) {
    const uint64_t nb = n_blocks(n, p.hop);
    if (nb == 0) return 0;
    if (p.mode == LV_PARTS) return (nb - 1u) * p.parts + parts_of(block_len(n, p.hop, nb - 1u), p.T);
    return (nb + p.group - 1u) / p.group;
}

struct Tile {
    uint64_t t0, block0;  // its first sample in the window; its first block
    uint32_t ns, part;    // its samples; LV_PARTS: which part of block0
};

FG_HD Tile tile_at(uint64_t n, const Plan &p, uint64_t tile) {
    Tile t;
    if (p.mode == LV_PARTS) {
        t.block0 = tile / p.parts;
        t.part = (uint32_t)(tile - t.block0 * p.parts);
        t.t0 = t.block0 * p.hop + (uint64_t)t.part * p.T;
        const uint64_t end = t.block0 * p.hop + block_len(n, p.hop, t.block0);
        t.ns = (uint32_t)(end - t.t0 < p.T ? end - t.t0 : p.T);
    } else {
        t.block0 = tile * p.group;
        t.part = 0;
        t.t0 = t.block0 * p.hop;
        const uint64_t most = (uint64_t)p.group * p.hop;
        t.ns = (uint32_t)(n - t.t0 < most ? n - t.t0 : most);
    }
    return t;
}

// the Acc records a window of n samples of C channels leaves for k_levels_fold: none where P = 1
FG_HD uint64_t partial_records(uint64_t n, const Plan &p, uint32_t C) {
    return p.parts > 1u ? n_blocks(n, p.hop) * p.parts * C : 0u;
}

// The aligned 8-byte words that hold the ns * per source bytes at address a (ns > 0): from address
// a0 on, n_words of them (<= deliver::kTileWords), the first source byte at byte `lead` of the first.
// No word past the one that holds the last source byte is among them.
FG_HD void tile_words(uint64_t a, uint32_t ns, uint32_t per, uint64_t &a0, uint32_t &lead, uint32_t &n_words) {
    a0 = a & ~(uint64_t)7;
    lead = (uint32_t)(a - a0);
    n_words = (lead + ns * per + 7u) / 8u;
}

// Channel c of the tile's samples t = first, first + stride, ... < end, out of the staged words.
FG_HD Acc tile_acc(const uint32_t *words, uint32_t lead, uint32_t per, uint32_t B, uint32_t c, uint32_t first, uint32_t end,
                   uint32_t stride) {
    Acc a = acc_zero();
    for (uint32_t t = first; t < end; t += stride) acc_add(a, deliver::sample_in_words(words, lead + t * per + c * B, B));
    return a;
}

}  // namespace levels
}  // namespace fg
