// fg_dec.hpp -- the scalar core of the FLAC frame decoder, shared by the device kernels
// (fg_dec.hip), the host side of the C ABI (flacgpu_flac_index) and the stand-alone host
// program of the tests (tests/cpp/decode_host_main.cpp).  Compiles under hipcc and plain g++.
//
// Written from RFC 9639 (section 9.1 frame header, 9.1.5 coded number, 9.1.8 CRC-8, 9.2 subframes,
// 9.2.2 wasted bits, 9.2.3-9.2.6 the four subframe types, 9.2.7 the coded residual, 9.3 frame
// footer) and from the format as the verifier decoder (oracle/flac_decode.c) reads it: the checks
// are made in that decoder's order, and a read past the frame's end behaves as its br_t does.
//
// Two stages.  The WALK (walk_subframe) goes through a subframe once, sequentially, doing no
// arithmetic on the residual values: it checks every rule of the layout and leaves a DecSub
// descriptor that says where each segment's residuals start: a frame is cut into kSegs = 64
// segments of seg_len(block size) = 64, 128 or 256 samples.  The SEGMENT DECODE (decode_segment)
// then turns one segment's codes into residuals, independently of every other segment -- on the
// device, one lane per segment.
#pragma once
#include <stdint.h>

#include "fg_crc.hpp"

namespace fg {
namespace dec {

// per-frame status: 1..7 are minus the verifier decoder's FD_* codes (include/flacgpu.h)
enum : uint32_t {
    ST_OK = 0, ST_SYNC = 1, ST_HEADER = 2, ST_CRC8 = 3, ST_SUBFRAME = 4, ST_CRC16 = 5, ST_TRUNCATED = 6,
    ST_RANGE = 7, ST_MISMATCH = 8
};

constexpr uint32_t kMaxFrameBytes = 1u << 28;  // bit positions stay below 2^31; longer "frames" are cut here
constexpr uint32_t kSegs = 64;                 // segments of a frame, whatever its block size
constexpr uint32_t kMaxBlock = 16384;          // RFC 9639's streamable subset; 64-bit planes (32-bit samples): 8192

// Samples of one segment of a frame of bs samples: 64 up to 4096 samples (the only length there
// was when no frame was larger, so those frames' descriptors are what they always were), 128 up to
// 8192, 256 up to 16384 = kMaxBlock.  A function of the frame alone, not of the context.
FG_HD uint32_t seg_shift(uint32_t bs) { return bs <= 4096u ? 6u : (bs <= 8192u ? 7u : 8u); }
FG_HD uint32_t seg_len(uint32_t bs) { return 1u << seg_shift(bs); }

// ---- bounded bit reader over one frame's bytes [p, p + nbits / 8) ----------------------------
// A read past the end returns zeros for the missing bits, leaves pos at the end and sets the
// sticky err flag (br_t of the verifier decoder, read bit by bit).
struct BitReader {
    const uint8_t *p;
    uint32_t nbits;
    uint32_t pos;
    uint32_t err;
};

FG_HD BitReader br_make(const uint8_t *p, uint32_t len_bytes, uint32_t pos = 0) {
    BitReader r;
    r.p = p;
    r.nbits = (len_bytes > kMaxFrameBytes ? kMaxFrameBytes : len_bytes) * 8u;
    r.pos = pos;
    r.err = 0;
    return r;
}

// bytes b .. b+7 as a big-endian word, zeros past the frame's end: the only memory access
FG_HD uint64_t br_window(const BitReader &r, uint32_t b) {
    const uint32_t len = r.nbits >> 3;
    uint64_t w = 0;
    if (b + 8u <= len) {
        __builtin_memcpy(&w, r.p + b, 8);
        return __builtin_bswap64(w);
    }
    for (uint32_t k = 0; k < 8u; k++) w = (w << 8) | (b + k < len ? (uint64_t)r.p[b + k] : 0ull);
    return w;
}
FG_HD uint32_t br_peek32(const BitReader &r) { return (uint32_t)((br_window(r, r.pos >> 3) << (r.pos & 7u)) >> 32); }

FG_HD void br_skip(BitReader &r, uint32_t n) {
    const uint32_t rem = r.nbits - r.pos;
    if (n > rem) {
        r.pos = r.nbits;
        r.err = 1;
    } else {
        r.pos += n;
    }
}
FG_HD uint32_t br_u(BitReader &r, uint32_t n) {  // n <= 32
    if (n == 0) return 0;
    const uint32_t v = br_peek32(r) >> (32u - n);
    br_skip(r, n);
    return v;
}
FG_HD uint64_t br_u64(BitReader &r, uint32_t n) {  // n <= 64
    if (n <= 32u) return br_u(r, n);
    const uint64_t hi = br_u(r, n - 32u);
    return (hi << 32) | br_u(r, 32u);
}
FG_HD int64_t br_s(BitReader &r, uint32_t n) {  // n <= 64, two's complement
    if (n == 0) return 0;
    uint64_t v = br_u64(r, n);
    if (n < 64u && ((v >> (n - 1u)) & 1u)) v |= ~0ull << n;
    return (int64_t)v;
}
// zeros before the next one bit; the run ends at the frame's end (err)
FG_HD uint64_t br_unary(BitReader &r) {
    uint64_t z = 0;
    for (;;) {
        const uint32_t rem = r.nbits - r.pos;
        if (rem == 0) {
            r.err = 1;
            return z;
        }
        const uint32_t w = br_peek32(r);
        const uint32_t lead = w ? (uint32_t)__builtin_clz(w) : 32u;
        if (lead >= rem) {  // only zeros up to the end
            z += rem;
            r.pos = r.nbits;
            r.err = 1;
            return z;
        }
        if (lead == 32u) {
            z += 32u;
            r.pos += 32u;
            continue;
        }
        r.pos += lead + 1u;
        return z + lead;
    }
}

// ---- CRCs -------------------------------------------------------------------------------------
FG_HD uint32_t crc8_bytes(const uint8_t *p, uint32_t n) {  // RFC 9639 9.1.8: poly x^8 + x^2 + x + 1, init 0
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    }
    return c;
}
FG_HD uint32_t crc16_bytes(const uint8_t *p, uint32_t n, uint32_t crc = 0) {  // RFC 9639 9.3, by the table-free byte step
    for (uint32_t i = 0; i < n; i++) crc = crc_byte_v(crc, p[i]);
    return crc;
}

// ---- frame header (RFC 9639 9.1) ----------------------------------------------------------------
struct FrameHdr {
    uint64_t number;  // coded frame / sample number (9.1.5)
    uint32_t block_size, sample_rate, channel_assign, bits, nch;
    uint32_t hdr_bytes;  // header bytes including the CRC-8
};

// Parses the header at the reader's position 0.  stream_bits / stream_rate stand in for the
// "from STREAMINFO" codes; channels / bits are what the context decodes; max_block its block size.
FG_HD uint32_t parse_header(BitReader &b, uint32_t stream_bits, uint32_t stream_rate, uint32_t channels, uint32_t bits,
                            uint32_t max_block, FrameHdr &h) {
    h.number = 0;
    h.block_size = h.sample_rate = h.channel_assign = h.bits = h.nch = h.hdr_bytes = 0;
    if (br_u(b, 15) != 0x7FFCu) return ST_SYNC;  // 9.1.1: sync code and the reserved bit after it
    br_u(b, 1);                                  // blocking strategy
    const uint32_t bsc = br_u(b, 4), src = br_u(b, 4), chc = br_u(b, 4), bitc = br_u(b, 3);
    if (br_u(b, 1) != 0) return ST_HEADER;  // 9.1.4: reserved bit
    // 9.1.5: the coded number, UTF-8-like, up to 7 bytes (36 bits)
    const uint32_t first = br_u(b, 8);
    uint64_t num;
    int extra;
    if (!(first & 0x80u)) { num = first; extra = 0; }
    else if ((first & 0xE0u) == 0xC0u) { num = first & 0x1Fu; extra = 1; }
    else if ((first & 0xF0u) == 0xE0u) { num = first & 0x0Fu; extra = 2; }
    else if ((first & 0xF8u) == 0xF0u) { num = first & 0x07u; extra = 3; }
    else if ((first & 0xFCu) == 0xF8u) { num = first & 0x03u; extra = 4; }
    else if ((first & 0xFEu) == 0xFCu) { num = first & 0x01u; extra = 5; }
    else if (first == 0xFEu) { num = 0; extra = 6; }
    else return ST_HEADER;
    for (int i = 0; i < extra; i++) {
        const uint32_t c = br_u(b, 8);
        if ((c & 0xC0u) != 0x80u) return ST_HEADER;
        num = (num << 6) | (c & 0x3Fu);
    }
    // 9.1.2: block size code
    uint32_t bs;
    if (bsc == 0) return ST_HEADER;
    else if (bsc == 1) bs = 192;
    else if (bsc <= 5) bs = 576u << (bsc - 2u);
    else if (bsc == 6) bs = br_u(b, 8) + 1u;
    else if (bsc == 7) bs = br_u(b, 16) + 1u;
    else bs = 256u << (bsc - 8u);
    // 9.1.2: sample rate code
    uint32_t rate;
    switch (src) {
    case 0: rate = stream_rate; break;
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = br_u(b, 8) * 1000u; break;
    case 13: rate = br_u(b, 16); break;
    case 14: rate = br_u(b, 16) * 10u; break;
    default: return ST_HEADER;
    }
    // 9.1.4: bit depth code
    uint32_t fbits;
    switch (bitc) {
    case 0: fbits = stream_bits; break;
    case 1: fbits = 8; break;
    case 2: fbits = 12; break;
    case 4: fbits = 16; break;
    case 5: fbits = 20; break;
    case 6: fbits = 24; break;
    case 7: fbits = 32; break;
    default: fbits = 0;
    }
    if (fbits == 0) return ST_HEADER;
    // 9.1.3: channels; a frame that is not of the context's channel count or bit depth is refused here
    const uint32_t nch = chc <= 7u ? chc + 1u : (chc <= 10u ? 2u : 0u);
    // (channels == 0: any, for the host-side frame index)
    if (nch == 0 || (channels != 0 && (nch != channels || fbits != bits))) return ST_HEADER;
    const uint32_t hdr = b.pos >> 3;
    const uint32_t crc8 = br_u(b, 8);
    if (b.err) return ST_TRUNCATED;
    if (crc8 != crc8_bytes(b.p, hdr)) return ST_CRC8;
    h.number = num;
    h.block_size = bs;
    h.sample_rate = rate;
    h.channel_assign = chc;
    h.bits = fbits;
    h.nch = nch;
    h.hdr_bytes = hdr + 1u;
    if (bs > max_block) return ST_RANGE;
    return ST_OK;
}

// bit depth of subframe c of a frame (9.1.3: the side channel has one bit more)
FG_HD uint32_t sub_bps(uint32_t chc, uint32_t c, uint32_t bits) {
    return ((chc == 8u && c == 1u) || (chc == 9u && c == 0u) || (chc == 10u && c == 1u)) ? bits + 1u : bits;
}

// ---- subframe descriptor --------------------------------------------------------------------
// seg_par[s]: bits 0..4 the Rice parameter (or the escape width), bit 5 escape, bit 6 "seg_pos
// points at a partition's parameter field" (the segment starts a partition)
constexpr uint32_t PAR_ESC = 0x20u, PAR_FIELD = 0x40u;
enum : uint32_t { SUB_CONSTANT = 0, SUB_VERBATIM = 1, SUB_FIXED = 2, SUB_LPC = 3 };

struct DecSub {
    uint32_t warm_pos;   // bit position of the warm-up samples (CONSTANT: the value, VERBATIM: sample 0)
    uint32_t coef_pos;   // LPC: bit position of the first coefficient
    uint32_t end_pos;    // bit position after the subframe's last bit
    uint32_t seg_pos[kSegs];  // where segment s's first residual (sample max(seg_len s, order)) starts
    uint8_t seg_par[kSegs];
    uint8_t type, order, waste, sbps;  // sbps: bits of a sample of this subframe after the waste shift
    uint8_t method, porder, prec, shift;
};
static_assert(sizeof(DecSub) == 340, "DecSub layout");

// 9.2.7: the coded residual, walked without decoding a value; SH = seg_shift(bs).  This loop bounds
// the whole decode (one lane per frame), and a segment length held in a register instead of the
// constant 64 measured 3 to 5 % slower on frames of 4096 samples: hence one copy per length.
template <uint32_t SH>
FG_HD uint32_t walk_residual_at(BitReader &b, uint32_t bs, uint32_t order, DecSub &d) {
    const uint32_t method = br_u(b, 2);
    if (method > 1u) return ST_SUBFRAME;
    const uint32_t pbits = method ? 5u : 4u, esc = method ? 31u : 15u;
    const uint32_t porder = br_u(b, 4);
    const uint32_t nparts = 1u << porder;
    if ((bs >> porder) < order || (bs % nparts) != 0) return ST_SUBFRAME;
    d.method = (uint8_t)method;
    d.porder = (uint8_t)porder;
    constexpr uint32_t L = 1u << SH;
    uint32_t i = order, seg = 0;
    for (uint32_t pt = 0; pt < nparts; pt++) {
        const uint32_t cnt = (bs >> porder) - (pt == 0 ? order : 0u);
        const uint32_t field = b.pos;
        const uint32_t k = br_u(b, pbits);
        uint32_t w = 0;
        if (k == esc) w = br_u(b, 5);
        for (uint32_t j = 0; j < cnt; j++, i++) {
            while (seg < kSegs && L * seg <= i) {
                d.seg_pos[seg] = j == 0 ? field : b.pos;
                d.seg_par[seg] = (uint8_t)((k == esc ? (PAR_ESC | w) : k) | (j == 0 ? PAR_FIELD : 0u));
                seg++;
            }
            if (k == esc) {
                br_skip(b, w);
            } else {
                br_unary(b);
                br_skip(b, k);
            }
        }
        if (b.err) return ST_TRUNCATED;
    }
    for (; seg < kSegs; seg++) {
        d.seg_pos[seg] = b.pos;
        d.seg_par[seg] = 0;
    }
    return ST_OK;
}

// MAXSH: the largest segment shift the caller's frames can have.  A caller whose frames have at
// most 4096 samples (parse_header's max_block) says 6 and compiles the instructions such frames
// always ran, and nothing else; 8 takes every frame up to kMaxBlock.
template <uint32_t MAXSH>
FG_HD uint32_t walk_residual_upto(BitReader &b, uint32_t bs, uint32_t order, DecSub &d) {
    if (MAXSH == 6u || bs <= 4096u) return walk_residual_at<6>(b, bs, order, d);
    if (MAXSH == 7u || bs <= 8192u) return walk_residual_at<7>(b, bs, order, d);
    return walk_residual_at<8>(b, bs, order, d);
}
FG_HD uint32_t walk_residual(BitReader &b, uint32_t bs, uint32_t order, DecSub &d) {
    return walk_residual_upto<8>(b, bs, order, d);
}

// 9.2: one subframe of bps bits per sample; fills d.  The rules and their order are
// decode_subframe's of the verifier decoder.
template <uint32_t MAXSH>
FG_HD uint32_t walk_subframe_upto(BitReader &b, uint32_t bs, uint32_t bps, DecSub &d) {
    d.warm_pos = d.coef_pos = d.end_pos = 0;
    d.type = d.order = d.waste = d.sbps = d.method = d.porder = d.prec = d.shift = 0;
    if (br_u(b, 1) != 0) return ST_SUBFRAME;  // 9.2.1: padding bit
    const uint32_t t = br_u(b, 6);
    uint64_t waste = 0;
    if (br_u(b, 1)) waste = br_unary(b) + 1u;  // 9.2.2
    if (waste > bps) return ST_SUBFRAME;
    const uint32_t sbps = bps - (uint32_t)waste;
    d.waste = (uint8_t)waste;
    d.sbps = (uint8_t)sbps;
    for (uint32_t s = 0; s < kSegs; s++) {
        d.seg_pos[s] = 0;
        d.seg_par[s] = 0;
    }
    if (t == 0) {  // 9.2.3 CONSTANT
        d.type = SUB_CONSTANT;
        d.warm_pos = b.pos;
        br_skip(b, sbps);
    } else if (t == 1) {  // 9.2.4 VERBATIM
        d.type = SUB_VERBATIM;
        d.warm_pos = b.pos;
        br_skip(b, bs * sbps);
    } else if (t >= 8 && t <= 12) {  // 9.2.5 FIXED
        const uint32_t order = t - 8u;
        d.type = SUB_FIXED;
        d.order = (uint8_t)order;
        if (order > bs) return ST_SUBFRAME;
        d.warm_pos = b.pos;
        br_skip(b, order * sbps);
        const uint32_t rc = walk_residual_upto<MAXSH>(b, bs, order, d);
        if (rc) return rc;
    } else if (t >= 32) {  // 9.2.6 LPC
        const uint32_t order = (t & 31u) + 1u;
        d.type = SUB_LPC;
        d.order = (uint8_t)order;
        if (order > bs) return ST_SUBFRAME;
        d.warm_pos = b.pos;
        br_skip(b, order * sbps);
        const uint32_t prec = br_u(b, 4) + 1u;
        if (prec == 16u) return ST_SUBFRAME;
        const int32_t shift = (int32_t)br_s(b, 5);
        if (shift < 0) return ST_SUBFRAME;
        d.prec = (uint8_t)prec;
        d.shift = (uint8_t)shift;
        d.coef_pos = b.pos;
        br_skip(b, order * prec);
        const uint32_t rc = walk_residual_upto<MAXSH>(b, bs, order, d);
        if (rc) return rc;
    } else {
        return ST_SUBFRAME;  // reserved types
    }
    d.end_pos = b.pos;
    return b.err ? ST_TRUNCATED : ST_OK;
}
FG_HD uint32_t walk_subframe(BitReader &b, uint32_t bs, uint32_t bps, DecSub &d) {
    return walk_subframe_upto<8>(b, bs, bps, d);
}

// The whole provisional check of one frame: header, every subframe's walk, the padding and the
// presence of the CRC-16 (its value is checked by the caller over body_bytes).  subs: h.nch entries.
// MAXSH = 6 needs max_block <= 4096: a larger frame is RANGE before any subframe is walked.
template <uint32_t MAXSH>
FG_HD uint32_t parse_frame_upto(const uint8_t *p, uint32_t len, uint32_t stream_rate, uint32_t channels, uint32_t bits,
                                uint32_t max_block, FrameHdr &h, DecSub *subs, uint32_t &body_bytes) {
    BitReader b = br_make(p, len);
    body_bytes = 0;
    uint32_t st = parse_header(b, bits, stream_rate, channels, bits, max_block, h);
    if (st) return st;
    for (uint32_t c = 0; c < h.nch; c++) {
        st = walk_subframe_upto<MAXSH>(b, h.block_size, sub_bps(h.channel_assign, c, h.bits), subs[c]);
        if (st) return st;
    }
    while (b.pos & 7u)  // 9.3: zero padding to a byte boundary
        if (br_u(b, 1) != 0) return ST_SUBFRAME;
    const uint32_t body = b.pos >> 3;
    br_u(b, 16);
    if (b.err) return ST_TRUNCATED;
    body_bytes = body;
    return ST_OK;
}
FG_HD uint32_t parse_frame(const uint8_t *p, uint32_t len, uint32_t stream_rate, uint32_t channels, uint32_t bits,
                           uint32_t max_block, FrameHdr &h, DecSub *subs, uint32_t &body_bytes) {
    return parse_frame_upto<8>(p, len, stream_rate, channels, bits, max_block, h, subs, body_bytes);
}

// ---- segment decode -------------------------------------------------------------------------
// Residuals of samples max(L s, order) .. min(L s + L, bs) - 1, L = seg_len(bs), of a FIXED / LPC subframe, each
// handed to put(i, value); crosses partition boundaries (a partition may be shorter than a
// segment).  Returns the bit position after the segment's last code.
template <typename Put>
FG_HD uint32_t decode_segment(const uint8_t *p, uint32_t len, const DecSub &d, uint32_t bs, uint32_t s, uint32_t &err,
                              Put &&put) {
    BitReader b = br_make(p, len, d.seg_pos[s]);
    const uint32_t L = seg_len(bs);
    uint32_t i = L * s < d.order ? d.order : L * s;
    const uint32_t end = L * s + L < bs ? L * s + L : bs;
    const uint32_t psize = bs >> d.porder;
    const uint32_t pbits = d.method ? 5u : 4u, escv = d.method ? 31u : 15u;
    uint32_t par = d.seg_par[s];
    bool field = (par & PAR_FIELD) != 0;
    for (bool first = true; i < end; i++, first = false) {
        if (first ? field : (i % psize) == 0) {
            const uint32_t k = br_u(b, pbits);
            par = k == escv ? (PAR_ESC | br_u(b, 5)) : k;
        }
        const uint32_t k = par & 31u;
        int64_t v;
        if (par & PAR_ESC) {
            v = br_s(b, k);
        } else {
            const uint64_t q = br_unary(b);
            const uint64_t u = (q << k) | br_u(b, k);
            v = (u & 1u) ? -(int64_t)(u >> 1) - 1 : (int64_t)(u >> 1);
        }
        put(i, v);
    }
    err |= b.err;
    return b.pos;
}

// ---- interleaved little-endian PCM, the bytes the verifier decoder writes ------------------
FG_HD bool sample_in_range(int64_t v, uint32_t bits) { return v >= -(1ll << (bits - 1u)) && v < (1ll << (bits - 1u)); }

// ---- what the host hands the two kernels (fg_dec.hip) ------------------------------------------
struct Result {  // = flacgpu_decode_result
    uint32_t status, block_size;
    uint64_t number;
    uint32_t sample_rate, first_bad;
    uint8_t channel_assign, bits, pad[6];
};
static_assert(sizeof(Result) == 32, "Result layout");

struct Args {
    const uint8_t *frames;
    const uint64_t *frame_off;   // [f] byte offset of frame f in frames
    const uint32_t *frame_bytes; // [f]
    uint32_t n_frames;
    uint32_t channels, bits, bps, rate, block;  // the context's stream; bps = bytes per sample
    DecSub *subs;                // [f * channels + c] (k_dec_parse -> k_dec_recon)
    uint32_t *blocks;            // [f] parsed block size, 0 if the header did not parse (input of the scan)
    uint32_t *body;              // [f] bytes before the CRC-16
    const uint64_t *pcm_off;     // [f] byte offset of the frame's PCM, or NULL:
    const uint64_t *samp_off;    //     [f] sample offset from the scan of blocks
    uint8_t *out;                // interleaved PCM (NULL: none), capacity cap bytes
    uint64_t cap;
    const uint8_t *expect;       // PCM to compare with (NULL: none), same offsets
    const uint64_t *exp_number;  // verify: [f] the frame number and
    const uint32_t *exp_n;       //         [f] the sample count the frame must have (NULL: any)
    Result *results;
    uint32_t *bad;               // frames with a non-zero status
    uint32_t *ticket;            // frame queue of k_dec_recon (zeroed by k_dec_parse)
};

}  // namespace dec
}  // namespace fg
