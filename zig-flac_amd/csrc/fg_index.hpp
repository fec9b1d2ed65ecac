// fg_index.hpp -- the scalar pieces of the frame index, shared by the device kernels
// (fg_index.hip), the host index (fg_dec_api.cpp: header_at) and the stand-alone host program of
// the tests (tests/cpp/index_host_main.cpp).  Compiles under hipcc and plain g++.
//
// The host index (fg_dec_api.cpp index_frames) walks from offset 0 and ends a frame at the first
// position e >= start + header + 3 where the CRC-16 over the frame is good and a clean header (or
// the end of the data) follows.  FLAC's CRC-16 has init 0 and no final XOR, so it is linear: with
// P(x) the CRC register after bytes [0, x), CRC[s, e) = P(e) ^ P(s) z^(8(e-s)) mod the
// polynomial, and a good frame [s, e) (CRC over body and stored CRC = 0) is P(e) = P(s) z^(8(e-s)).
// The walk starts at P(0) = 0, so every position it reaches has P = 0: the frame starts are among
// the CANDIDATES, the positions with P = 0 and a clean header, and the only serial rule left is the
// minimum distance start + header + 3, which matters between candidates closer than kNear bytes.
//
// P at every position, in parallel: z is invertible (the polynomial has constant term 1; the order
// of z is 32767), so Q(x) = P(x) z^(-8x) is a plain XOR prefix sum, Q(b) = Q(a) ^ CRC[a, b) z^(-8b),
// of per-chunk terms that depend on the chunk's bytes and its end position alone.
#pragma once
#include <stdint.h>

#include "fg_dec.hpp"

namespace fg {
namespace idx {

enum : uint32_t { IDX_OK = 0, IDX_INVALID = 1, IDX_TOO_SMALL = 2 };  // = FLACGPU_INDEX_*

constexpr uint32_t kZOrder = 32767;  // z^15 + z + 1 is primitive, the other factor is z + 1
constexpr uint32_t kMaxHdr = 16;     // sync/codes 4, coded number 7, block size 2, sample rate 2, CRC-8 1
constexpr uint32_t kMinBody = 3;     // a frame's end is at least header + one subframe byte + CRC-16 past its start
constexpr uint32_t kNear = kMaxHdr + kMinBody - 1;  // a candidate this close before another may jump over it

// z^e mod P, e < 2^15: square and multiply, the multiply by z being one shift
FG_HD uint32_t zpow(uint32_t e) {
    uint32_t r = 1;
    for (int i = 14; i >= 0; i--) {
        r = crc_mulmod_v(r, r);
        if ((e >> i) & 1u) {
            r <<= 1;
            if (r & 0x10000u) r ^= 0x18005u;
        }
    }
    return r;
}
FG_HD uint32_t z8(uint64_t x) { return zpow((uint32_t)((8u * x) % kZOrder)); }  // z^(8x), x < 2^60
FG_HD uint32_t zinv8(uint64_t x) {                                              // z^(-8x)
    const uint32_t m = (uint32_t)((8u * x) % kZOrder);
    return zpow(m ? kZOrder - m : 0u);
}

// the XOR-prefix term of a chunk that ends at position b, from the plain CRC-16 of its bytes
FG_HD uint32_t chunk_term(uint32_t crc, uint64_t b) { return crc ? crc_mulmod_v(crc, zinv8(b)) : 0u; }
// P(a) from Q(a)
FG_HD uint32_t running_crc(uint32_t q, uint64_t a) { return q ? crc_mulmod_v(q, z8(a)) : 0u; }

// Chunk j of size C of the data laid `lead` bytes into a grid of chunks (the device aligns its
// chunks to the address, not to the data's first byte): positions [*a, *b) of [0, len), maybe empty.
FG_HD void chunk_bounds(uint64_t j, uint32_t C, uint32_t lead, uint64_t len, uint64_t *a, uint64_t *b) {
    const uint64_t lo = j * C, hi = lo + C, end = (uint64_t)lead + len;
    *a = (lo > lead ? lo : lead) - lead;
    *b = (hi < end ? hi : end) - lead;
    if (*b < *a) *b = *a;
}

// a frame header with a good CRC-8 starts at p (RFC 9639 9.1); its length in *hdr_bytes.  len: the
// bytes from p to the end of the data; the reader is clamped to them (and to 32).
FG_HD bool header_at(const uint8_t *p, uint64_t len, uint32_t stream_bits, uint32_t stream_rate, uint32_t *hdr_bytes) {
    if (len < 6 || p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return false;
    dec::BitReader b = dec::br_make(p, (uint32_t)(len > 32 ? 32 : len));
    dec::FrameHdr h;
    const uint32_t st = dec::parse_header(b, stream_bits, stream_rate, 0, 0, 65535u, h);
    *hdr_bytes = h.hdr_bytes;
    return st == dec::ST_OK;
}

// The candidate test at position x, whose byte is `byte` and whose successor is `next` (0 past the
// end): the running CRC before the byte is 0, a sync code, and a clean header.
FG_HD bool sync_at_zero(uint32_t P, uint32_t byte, uint32_t next) {
    return P == 0 && byte == 0xFFu && (next & 0xFEu) == 0xF8u;
}
FG_HD bool is_candidate(uint32_t P, uint32_t byte, uint32_t next, const uint8_t *data, uint64_t len, uint64_t x,
                        uint32_t stream_bits, uint32_t stream_rate) {
    if (!sync_at_zero(P, byte, next)) return false;
    uint32_t hdr = 0;
    return header_at(data + x, len - x, stream_bits, stream_rate, &hdr);
}

// ---- the minimum-distance rule --------------------------------------------------------------
// win(v): a word whose bit k says "a candidate sits at v + k" (k < 32; v may be negative; no
// candidates outside the data).  hdr_of(v): the header length of the candidate at v.
//
// A candidate with no other candidate in the kNear bytes before it is a HEAD.  The walk cannot
// pass a head: from a start s <= c - kNear - 1 the earliest end s + hdr + 3 is <= c, so the first
// candidate at or after it is c or comes before c.  Every head is therefore a frame start (given
// that offset 0 is one), and the frame starts between two heads are found by walking from the
// first: from a start, the next is the first candidate at or after start + hdr + 3; if that one
// is not a head it lies less than kNear past that bound (the candidate that makes it a non-head
// is before the bound).
template <class Win>
FG_HD bool is_head(int64_t v, Win &&win) {
    return (win(v - (int64_t)kNear) & ((1u << kNear) - 1u)) == 0;
}
// If v is a head: mark(v), and mark every frame start after it up to the next head.
template <class Win, class Hdr, class Mark>
FG_HD void resolve_from(int64_t v, Win &&win, Hdr &&hdr_of, Mark &&mark) {
    if (!is_head(v, win)) return;
    mark(v);
    for (int64_t cur = v;;) {
        const int64_t t = cur + (int64_t)hdr_of(cur) + (int64_t)kMinBody;
        const uint32_t w = win(t) & ((1u << kNear) - 1u);
        if (!w) return;
        const int64_t nxt = t + (int64_t)__builtin_ctz(w);
        if (is_head(nxt, win)) return;
        mark(nxt);
        cur = nxt;
    }
}

// The verdict, once the frame starts are counted: offset 0 must be a candidate, the running CRC at
// the end of the data must be 0 (the end is then the last frame's end), and the last frame must
// have its minimum length.  n_starts > cap: too small, with the true count.
FG_HD uint32_t verdict(bool cand0, uint32_t q_end, uint64_t last_start, uint32_t last_hdr, uint64_t len, uint64_t n_starts,
                       uint64_t cap) {
    if (!cand0 || q_end != 0 || n_starts == 0 || len - last_start < (uint64_t)last_hdr + kMinBody) return IDX_INVALID;
    return n_starts > cap ? IDX_TOO_SMALL : IDX_OK;
}

// ---- what the host hands the kernels (fg_index.hip) -----------------------------------------
constexpr uint32_t kIdxChunk = 64;   // bytes per lane: one 64-bit candidate mask per chunk
constexpr uint32_t kIdxGroup = 256;  // chunks (lanes) per workgroup

struct IndexResult {  // = flacgpu_index_result
    uint64_t n_frames;
    uint32_t status, reserved;
};
static_assert(sizeof(IndexResult) == 16, "IndexResult layout");

struct IdxArgs {
    const uint8_t *data;
    uint64_t len;            // 0 < len < 2^32
    uint32_t lead;           // address of data % 16: the chunk grid starts that many bytes before it
    uint32_t bits, rate;     // what the "from STREAMINFO" header codes stand for
    uint32_t n_groups;
    uint64_t n_chunks;       // chunks of the grid that hold data
    uint16_t *terms;         // [n_chunks]
    uint32_t *grp;           // [n_groups] XOR of the group's terms, then the exclusive scan of those
    uint64_t *cmask, *smask; // [n_chunks] candidates / frame starts, bit k = grid byte 64 j + k
    uint32_t *gcnt;          // [n_groups] frame starts of the group, then their exclusive scan
    uint32_t *ctl;           // [0] Q at the end of the data, [1] number of frame starts
    uint32_t *spos;          // [spos_cap] frame start by rank
    uint64_t spos_cap;       // min(cap, len / 8 + 1)
    uint64_t *offs;          // the caller's arrays
    uint32_t *bytes;
    uint64_t cap;
    IndexResult *res;
    uint64_t base_off;       // added to every offset written to offs[] (many streams: the stream's offset in the buffer)
};

// ---- many streams in one call ---------------------------------------------------------------
// Every stream is indexed on its own: its IdxArgs is one entry of a table in device memory, the
// kernels pick theirs from blockIdx.y (the two scans: one workgroup per stream), and every grid's
// x extent is sized from the longest stream; workgroups past a stream's groups exit at once.
constexpr uint32_t kIdxMaxStreams = 65535;  // gridDim.y

// what a stream's length, address and table capacity fix: the chunk grid and the rank array
FG_HD void stream_geometry(IdxArgs &g, uint64_t addr, uint64_t len, uint64_t cap) {
    g.len = len;
    g.lead = (uint32_t)(addr & 15u);
    g.n_chunks = len ? (g.lead + len + kIdxChunk - 1u) / kIdxChunk : 0u;
    g.n_groups = (uint32_t)((g.n_chunks + kIdxGroup - 1u) / kIdxGroup);
    const uint64_t most = len / 8u + 1u;  // a frame is at least 9 bytes
    g.spos_cap = len ? (cap < most ? cap : most) : 0u;
    g.cap = cap;
}

// the elements of each scratch array that the streams so far take, and the longest stream's grids
struct IdxTotals {
    uint64_t chunks = 0, groups = 0, spos = 0, streams = 0;
    uint32_t max_groups = 0;
    uint64_t max_spos = 0;
};
// the scratch arrays of all streams, each one allocation-aligned array over all of them
struct IdxPool {
    uint64_t *cmask, *smask;
    uint32_t *grp, *gcnt, *ctl, *spos;
    uint16_t *terms;
};
FG_HD void totals_add(IdxTotals &t, const IdxArgs &g) {
    t.chunks += g.n_chunks;
    t.groups += g.n_groups;
    t.spos += g.spos_cap;
    t.streams += 1u;
    if (g.n_groups > t.max_groups) t.max_groups = g.n_groups;
    if (g.spos_cap > t.max_spos) t.max_spos = g.spos_cap;
}
// stream g's carve of the pool: the elements after those of the streams counted in t; then counts g
FG_HD void carve_stream(IdxArgs &g, const IdxPool &p, IdxTotals &t) {
    g.cmask = p.cmask + t.chunks;
    g.smask = p.smask + t.chunks;
    g.terms = p.terms + t.chunks;
    g.grp = p.grp + t.groups;
    g.gcnt = p.gcnt + t.groups;
    g.spos = p.spos + t.spos;
    g.ctl = p.ctl + 4u * t.streams;
    totals_add(t, g);
}

}  // namespace idx
}  // namespace fg
