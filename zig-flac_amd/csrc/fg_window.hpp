// fg_window.hpp -- the scalar rules of the sample-window decode, shared by the device kernels
// (fg_window.hip), the host layer (fg_dec_host.cpp) and the stand-alone host program of the tests
// (tests/cpp/window_host_main.cpp).  Compiles under hipcc and plain g++.
//
// A stream's POSITIONS are the exclusive sum of its frames' block sizes, each read from the
// frame's header alone (never the coded frame or sample number: the rule of every other PCM
// offset in this decoder).  A WINDOW is a sample range [start, start + count) of one stream; its
// COVER is the run of frames that hold those samples.  The covering frames are decoded whole into
// scratch, and the window's bytes are then copied out of them: the COPY PLAN cuts the destination
// into the bytes before its first 16-byte boundary, whole 16-byte units and the bytes after them.
#pragma once
#include <stdint.h>

#include "fg_dec.hpp"

namespace fg {
namespace window {

enum : uint32_t { WIN_OK = 0, WIN_BAD_INDEX = 1, WIN_BAD_FRAME = 2, WIN_TOO_SMALL = 3 };  // = FLACGPU_WINDOW_*

struct WindowResult {  // = flacgpu_window_result
    uint64_t n_samples, first_frame;
    uint32_t n_frames, status, first_bad_frame, first_bad_status;
};
static_assert(sizeof(WindowResult) == 32, "WindowResult layout");

constexpr uint32_t kHdrRead = 16;  // = idx::kMaxHdr: the longest frame header

// The block size of the frame whose header starts at p, `avail` bytes before the end of its
// frame: parse_header as idx::header_at calls it (any channel count and depth, blocks up to
// 65535), over at most kHdrRead bytes.  0: no header parses there.
FG_HD uint32_t block_at(const uint8_t *p, uint64_t avail, uint32_t stream_bits, uint32_t stream_rate) {
    dec::BitReader b = dec::br_make(p, (uint32_t)(avail > kHdrRead ? kHdrRead : avail));
    dec::FrameHdr h;
    return dec::parse_header(b, stream_bits, stream_rate, 0, 0, 65535u, h) == dec::ST_OK ? h.block_size : 0u;
}

// how many of the ascending pos[0 .. n) are <= v
FG_HD uint64_t count_le(const uint64_t *pos, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (pos[mid] <= v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

struct Cover {
    uint64_t first_frame;  // first covering frame, counted in its stream
    uint64_t span;         // samples of the covering frames
    uint64_t skip;         // samples of the first covering frame before the window
    uint64_t n_samples;    // samples the window delivers
    uint32_t n_frames;     // covering frames
    uint32_t status;       // WIN_*
};
static_assert(sizeof(Cover) == 40, "Cover layout");

// The cover of [start, start + count) over a stream of n frames at positions pos[0 .. n) with
// `total` samples.  The range is clipped to the total (a sum that passes 64 bits is clipped, not
// wrapped); a window that starts at or past the end or has no samples covers nothing.
FG_HD Cover cover(const uint64_t *pos, uint64_t n, uint64_t total, uint64_t start, uint64_t count) {
    Cover c;
    c.first_frame = c.span = c.skip = c.n_samples = 0;
    c.n_frames = 0;
    c.status = WIN_OK;
    if (n == 0 || start >= total || count == 0) return c;
    const uint64_t end = (start + count < start || start + count > total) ? total : start + count;
    const uint64_t first = count_le(pos, n, start) - 1u;  // pos[0] = 0 <= start
    const uint64_t last = count_le(pos, n, end - 1u) - 1u;
    if (first >= n || last < first) return c;  // a table that does not start at 0: no stream's positions
    c.first_frame = first;
    c.n_frames = (uint32_t)(last - first + 1u);
    c.span = (last + 1u < n ? pos[last + 1u] : total) - pos[first];
    c.skip = start - pos[first];
    c.n_samples = end - start;
    return c;
}

// The copy of nb bytes to a destination whose address is dst_addr: `head` bytes up to the first
// 16-byte boundary (all of them where the copy ends before it), `units` whole 16-byte units,
// `tail` bytes after the last.
struct CopyPlan {
    uint32_t head, tail;
    uint64_t units;
};
FG_HD CopyPlan copy_plan(uint64_t dst_addr, uint64_t nb) {
    CopyPlan p;
    const uint64_t to_boundary = (16u - (dst_addr & 15u)) & 15u;
    p.head = (uint32_t)(to_boundary < nb ? to_boundary : nb);
    p.units = (nb - p.head) >> 4;
    p.tail = (uint32_t)((nb - p.head) & 15u);
    return p;
}

// The 16 source bytes at src (any alignment) as two little-endian words, by aligned 8-byte loads:
// the words read are those that hold a byte of [src, src + 16), so nothing is read past the
// 8-byte word that holds the source's last byte.
FG_HD void load_unit(const uint8_t *src, uint64_t &q0, uint64_t &q1) {
    const uintptr_t a = (uintptr_t)src, a0 = a & ~(uintptr_t)7;
    const uint32_t sh = (uint32_t)(a - a0) * 8u;
    const uint64_t *w = (const uint64_t *)a0;
    const uint64_t w0 = w[0], w1 = w[1];
    if (sh == 0) {
        q0 = w0;
        q1 = w1;
        return;
    }
    const uint64_t w2 = w[2];
    q0 = (w0 >> sh) | (w1 << (64u - sh));
    q1 = (w1 >> sh) | (w2 << (64u - sh));
}

// ---- what the host hands the kernels (fg_window.hip) ----------------------------------------
struct PosStream {  // one stream of a positions call
    uint64_t table_first, table_cap;
    uint32_t bits, rate;
};
static_assert(sizeof(PosStream) == 24, "PosStream layout");

struct WindowArg {  // one window of a call, as the caller states it
    uint64_t start, count, cap;  // cap: bytes of its destination
    uint64_t table_first;        // of its stream
    uint32_t stream, pad;
};
static_assert(sizeof(WindowArg) == 40, "WindowArg layout");

}  // namespace window
}  // namespace fg
