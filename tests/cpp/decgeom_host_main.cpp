// decgeom_host_main.cpp -- the decoder's geometry (zig-flac_amd/csrc/fg_geom.hpp: dec_geometry,
// fg_dec.hpp: seg_len) and the subframe descriptors its walk leaves, on the host.  A stand-alone
// program, built by tests/test_bigblock_host.py with -fsanitize=address,undefined.
//
//   decgeom_host_main geom CHANNELS,BITS,BLOCK ...
//       one JSON row per argument: {"ok": 1, "elem": bytes of a plane element, "plane_words", "W",
//       "lds", "passes"} or {"ok": 0}
//   decgeom_host_main seglen BLOCK ...
//       the segment length of a frame of BLOCK samples, one per argument
//   decgeom_host_main decsub FRAMES SIZES CHANNELS BITS RATE OUT
//       parse_frame over each frame of FRAMES (SIZES: text, one length per line), each alone in an
//       allocation of exactly its length; the DecSub bytes of its subframes, in order, go to OUT.
//       Prints {"status": [...], "nsub": [...]}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// host only: fg_layout.hpp's functions are plain inline functions here
#define __host__
#define __device__
#include "../../zig-flac_amd/csrc/fg_geom.hpp"
#include "../../zig-flac_amd/csrc/fg_dec.hpp"

using namespace fg::dec;

static int decsub(int argc, char **argv) {
    if (argc != 8) return 2;
    const uint32_t channels = (uint32_t)atoi(argv[4]), bits = (uint32_t)atoi(argv[5]), rate = (uint32_t)atoi(argv[6]);
    std::vector<uint8_t> buf;
    {
        FILE *fp = fopen(argv[2], "rb");
        if (!fp) return 2;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, fp)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(fp);
    }
    std::vector<uint32_t> sizes;
    {
        FILE *fp = fopen(argv[3], "r");
        if (!fp) return 2;
        unsigned long v;
        while (fscanf(fp, "%lu", &v) == 1) sizes.push_back((uint32_t)v);
        fclose(fp);
    }
    FILE *out = fopen(argv[7], "wb");
    if (!out) return 2;
    std::vector<uint32_t> status, nsub;
    size_t pos = 0;
    for (uint32_t len : sizes) {
        if (pos + len > buf.size()) return 2;
        uint8_t *fr = (uint8_t *)malloc(len ? len : 1);
        memcpy(fr, buf.data() + pos, len);
        DecSub subs[8];
        memset(subs, 0, sizeof subs);
        FrameHdr h;
        uint32_t body = 0;
        const uint32_t st = parse_frame(fr, len, rate, channels, bits, kMaxBlock, h, subs, body);
        free(fr);
        status.push_back(st);
        nsub.push_back(st ? 0u : h.nch);
        if (!st) fwrite(subs, sizeof(DecSub), h.nch, out);
        pos += len;
    }
    fclose(out);
    printf("{\"status\": [");
    for (size_t i = 0; i < status.size(); i++) printf("%s%u", i ? ", " : "", status[i]);
    printf("], \"nsub\": [");
    for (size_t i = 0; i < nsub.size(); i++) printf("%s%u", i ? ", " : "", nsub[i]);
    printf("]}\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "decsub")) return decsub(argc, argv);
    if (!strcmp(argv[1], "seglen")) {
        printf("[");
        for (int i = 2; i < argc; i++) printf("%s%u", i > 2 ? ", " : "", seg_len((uint32_t)atoi(argv[i])));
        printf("]\n");
        return 0;
    }
    if (!strcmp(argv[1], "geom")) {
        printf("[");
        for (int i = 2; i < argc; i++) {
            unsigned c = 0, b = 0, blk = 0;
            if (sscanf(argv[i], "%u,%u,%u", &c, &b, &blk) != 3) return 2;
            const fg::DecGeom g = fg::dec_geometry(c, b, blk);
            if (!g.ok) printf("%s{\"ok\": 0}", i > 2 ? ", " : "");
            else
                printf("%s{\"ok\": 1, \"elem\": %u, \"plane_words\": %u, \"W\": %u, \"lds\": %u, \"passes\": %u}",
                       i > 2 ? ", " : "", g.elem, g.plane_words, g.W, g.lds, g.passes);
        }
        printf("]\n");
        return 0;
    }
    return 2;
}
