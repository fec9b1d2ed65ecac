// decode_host_main.cpp -- the decode core of libflacgpu.so (zig-flac_amd/csrc/fg_dec.hpp) run
// entirely on the host: header parse, subframe walk, segment decode, continuity check, and a
// plain scalar restore in place of the device's wave-level one.  A stand-alone program, built by
// tests/test_decode_host.py with -fsanitize=address,undefined: every byte the shared code reads
// or writes for good and for corrupted frames is checked here before a GPU sees such input.
//
//   decode_host_main FRAMES CHANNELS BITS RATE BLOCK OUT_PCM [SIZES]
//
// FRAMES: concatenated frames.  SIZES (text, one length per line): each frame is decoded alone
// within its own length; without it the frames are taken one after another, each as long as it
// parses.  Prints {"status": [...], "consumed": [...], "block": [...], "number": [...]} and writes
// the PCM of the frames with status 0 to OUT_PCM.  Each frame is copied into an allocation of
// exactly its length first, so a read past the frame is a heap overflow the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_dec.hpp"

using namespace fg::dec;

namespace {

struct Frame {
    uint32_t status = 0, consumed = 0, block = 0;
    uint64_t number = 0;
};

// one frame within [p, p + len): status as the device computes it, samples to planes
Frame decode_frame(const uint8_t *p, uint32_t len, uint32_t channels, uint32_t bits, uint32_t rate, uint32_t block,
                   bool exact_len, std::vector<std::vector<int64_t>> &planes) {
    Frame f;
    FrameHdr h;
    std::vector<DecSub> subs(8);
    uint32_t body = 0;
    f.status = parse_frame(p, len, rate, channels, bits, block, h, subs.data(), body);
    f.block = h.block_size;
    f.number = h.number;
    if (f.status) return f;
    f.consumed = body + 2;
    const uint32_t bs = h.block_size;
    uint32_t err = 0;
    for (uint32_t c = 0; c < h.nch; c++) {
        const DecSub &d = subs[c];
        std::vector<int64_t> &x = planes[c];
        x.assign(bs, 0);
        BitReader b = br_make(p, len, d.warm_pos);
        if (d.type == SUB_CONSTANT) {
            const int64_t v = br_s(b, d.sbps);
            for (uint32_t i = 0; i < bs; i++) x[i] = v;
        } else if (d.type == SUB_VERBATIM) {
            for (uint32_t i = 0; i < bs; i++) x[i] = br_s(b, d.sbps);
        } else {
            for (uint32_t i = 0; i < d.order; i++) x[i] = br_s(b, d.sbps);
            int64_t coef[32] = {0};
            if (d.type == SUB_LPC) {
                BitReader cb = br_make(p, len, d.coef_pos);
                for (uint32_t j = 0; j < d.order; j++) coef[j] = br_s(cb, d.prec);
                err |= cb.err;
            }
            // every segment on its own, then the continuity check
            for (uint32_t s = 0; s < kSegs; s++) {
                const uint32_t end = decode_segment(p, len, d, bs, s, err, [&](uint32_t i, int64_t v) { x.at(i) = v; });
                const uint32_t next = s + 1 < kSegs ? d.seg_pos[s + 1] : d.end_pos;
                if (end != next) f.status = ST_SUBFRAME;
            }
            for (uint32_t i = d.order; i < bs; i++) {
                if (d.type == SUB_FIXED) {
                    uint64_t pr = 0;  // unsigned: wraps as the device's integers do on hostile values
                    const uint64_t a = i >= 1 ? (uint64_t)x[i - 1] : 0, bq = i >= 2 ? (uint64_t)x[i - 2] : 0,
                                   cq = i >= 3 ? (uint64_t)x[i - 3] : 0, dq = i >= 4 ? (uint64_t)x[i - 4] : 0;
                    switch (d.order) {
                    case 1: pr = a; break;
                    case 2: pr = 2 * a - bq; break;
                    case 3: pr = 3 * a - 3 * bq + cq; break;
                    case 4: pr = 4 * a - 6 * bq + 4 * cq - dq; break;
                    default: pr = 0;
                    }
                    x[i] = (int64_t)((uint64_t)x[i] + pr);
                } else {
                    uint64_t acc = 0;
                    for (uint32_t j = 0; j < d.order; j++) acc += (uint64_t)coef[j] * (uint64_t)x[i - 1 - j];
                    x[i] = (int64_t)((uint64_t)x[i] + (uint64_t)((int64_t)acc >> d.shift));
                }
            }
        }
        err |= b.err;
        if (d.waste)
            for (uint32_t i = 0; i < bs; i++) x[i] = (int64_t)((uint64_t)x[i] << d.waste);
    }
    if (f.status) return f;
    if (err) {
        f.status = ST_TRUNCATED;
        return f;
    }
    const uint32_t chc = h.channel_assign;
    for (uint32_t i = 0; i < bs && h.nch == 2; i++) {
        const uint64_t a = (uint64_t)planes[0][i], s = (uint64_t)planes[1][i];
        if (chc == 8) planes[1][i] = (int64_t)(a - s);
        else if (chc == 9) planes[0][i] = (int64_t)(a + s);
        else if (chc == 10) {
            const uint64_t mid = a * 2 + (s & 1);
            planes[0][i] = (int64_t)(mid + s) >> 1;
            planes[1][i] = (int64_t)(mid - s) >> 1;
        }
    }
    const uint32_t crc = ((uint32_t)p[body] << 8) | p[body + 1];
    if (crc != crc16_bytes(p, body)) {
        f.status = ST_CRC16;
        return f;
    }
    if (exact_len && f.consumed != len) {  // bytes after the CRC-16 are no frame
        f.status = ST_SYNC;
        return f;
    }
    for (uint32_t c = 0; c < h.nch; c++)
        for (uint32_t i = 0; i < bs; i++)
            if (!sample_in_range(planes[c][i], bits)) f.status = ST_RANGE;
    return f;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 7) {
        fprintf(stderr, "usage: %s FRAMES CHANNELS BITS RATE BLOCK OUT_PCM [SIZES]\n", argv[0]);
        return 2;
    }
    const uint32_t channels = (uint32_t)atoi(argv[2]), bits = (uint32_t)atoi(argv[3]), rate = (uint32_t)atoi(argv[4]),
                   block = (uint32_t)atoi(argv[5]);
    if (channels < 1 || channels > 8 || (bits != 8 && bits != 16 && bits != 24 && bits != 32) || block < 1 ||
        block > kMaxBlock)
        return 2;
    std::vector<uint8_t> buf;
    {
        FILE *fp = fopen(argv[1], "rb");
        if (!fp) return 2;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, fp)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(fp);
    }
    std::vector<uint32_t> sizes;
    const bool have_sizes = argc > 7;
    if (have_sizes) {
        FILE *fp = fopen(argv[7], "r");
        if (!fp) return 2;
        unsigned long v;
        while (fscanf(fp, "%lu", &v) == 1) sizes.push_back((uint32_t)v);
        fclose(fp);
    }
    FILE *out = fopen(argv[6], "wb");
    if (!out) return 2;
    std::vector<std::vector<int64_t>> planes(8);
    std::vector<Frame> res;
    const uint32_t bps = bits / 8;
    size_t pos = 0;
    for (size_t k = 0; have_sizes ? k < sizes.size() : pos < buf.size(); k++) {
        const size_t len = have_sizes ? sizes[k] : buf.size() - pos;
        if (pos + len > buf.size()) return 2;
        // the frame alone in an allocation of exactly its size
        uint8_t *fr = (uint8_t *)malloc(len ? len : 1);
        memcpy(fr, buf.data() + pos, len);
        const Frame f = decode_frame(fr, (uint32_t)len, channels, bits, rate, block, have_sizes, planes);
        free(fr);
        res.push_back(f);
        if (f.status == 0) {
            std::vector<uint8_t> pcm((size_t)f.block * channels * bps);
            for (uint32_t i = 0; i < f.block; i++)
                for (uint32_t c = 0; c < channels; c++)
                    for (uint32_t b = 0; b < bps; b++)
                        pcm[((size_t)i * channels + c) * bps + b] = (uint8_t)((uint64_t)planes[c][i] >> (8 * b));
            fwrite(pcm.data(), 1, pcm.size(), out);
        }
        if (!have_sizes && f.status) break;
        pos += have_sizes ? len : f.consumed;
    }
    fclose(out);
    std::string js = "{";
    const char *names[4] = {"status", "consumed", "block", "number"};
    for (int q = 0; q < 4; q++) {
        js += std::string(q ? ", \"" : "\"") + names[q] + "\": [";
        for (size_t i = 0; i < res.size(); i++) {
            const unsigned long long v = q == 0 ? res[i].status : q == 1 ? res[i].consumed : q == 2 ? res[i].block : res[i].number;
            js += (i ? ", " : "") + std::to_string(v);
        }
        js += "]";
    }
    js += "}";
    puts(js.c_str());
    return 0;
}
