// levels_host_main.cpp -- the scalar rules of the level measurement (zig-flac_amd/csrc/fg_levels.hpp)
// on the host, for tests/test_levels_host.py, which builds this file with -fsanitize=address,undefined.
// Plain C++, no HIP.  Modes (JSON on stdout unless a file is named):
//   f64 IN OUT            IN: pairs of u64 (lo, hi); OUT: u128_to_f64 of each as the double's u64 bits
//   acc KIND N SPLIT      N samples -- KIND 0: all -2^31; 1: -2^31 and 2^31 - 1 alternating -- dealt
//                         round-robin to SPLIT partial Acc (acc_add), merged last to first (acc_merge)
//   geom N HOP PER        the plan of (HOP, PER) and every tile of a window of N samples
//   tile IN OUT B C N HOP LEAD
//                         IN: N * C samples as i32.  The window's PCM of B-byte samples is measured tile
//                         by tile the way k_window_levels does it: every tile's bytes lie alone in a
//                         heap block of exactly the aligned 8-byte words tile_words names, its first
//                         byte `lead` bytes in (LEAD for the first tile, then as the addresses fall),
//                         so a word read past the one that holds the tile's last byte is a sanitizer
//                         error; the words are copied to a second exact block and reduced out of it by
//                         the plan's mode with the kernel's strides (1; 64 lanes; 256 threads), parts
//                         merged per block.  OUT: per (block, channel) u32 peak, i64 sum, u64 energy bits
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string_view>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_levels.hpp"

using namespace fg;

static void fail(const char *why) {
    std::fprintf(stderr, "levels_host_main: %s\n", why);
    std::exit(2);
}

static std::vector<uint8_t> read_file(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) fail("cannot open the input");
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

static void write_file(const char *path, const void *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f || (n && std::fwrite(p, 1, n, f) != n)) fail("cannot write the output");
    std::fclose(f);
}

static uint64_t bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

static void *words_alloc(size_t n_words) {
    void *p = nullptr;
    if (posix_memalign(&p, 8, n_words * 8u)) fail("no memory");
    std::memset(p, 0xA5, n_words * 8u);
    return p;
}

struct Rec {
    uint32_t peak, pad;
    int64_t sum;
    uint64_t energy;
};

int main(int argc, char **argv) {
    if (argc < 2) fail("no mode");
    const std::string_view mode = argv[1];
    if (mode == "f64" && argc == 4) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        const size_t n = in.size() / 16u;
        std::vector<uint64_t> out(n);
        for (size_t i = 0; i < n; i++) {
            uint64_t lo, hi;
            std::memcpy(&lo, &in[16u * i], 8);
            std::memcpy(&hi, &in[16u * i + 8u], 8);
            out[i] = bits_of(levels::u128_to_f64(lo, hi));
        }
        write_file(argv[3], out.data(), n * 8u);
        std::printf("{\"count\": %zu}\n", n);
        return 0;
    }
    if (mode == "acc" && argc == 5) {
        const uint32_t kind = (uint32_t)std::atoi(argv[2]), split = (uint32_t)std::atoi(argv[4]);
        const uint64_t n = std::strtoull(argv[3], nullptr, 10);
        if (split == 0) fail("no partial");
        std::vector<levels::Acc> part(split, levels::acc_zero());
        for (uint64_t t = 0; t < n; t++) levels::acc_add(part[t % split], (kind == 1 && (t & 1u)) ? INT32_MAX : INT32_MIN);
        levels::Acc a = levels::acc_zero();
        for (uint32_t k = split; k-- > 0;) levels::acc_merge(a, part[k]);
        std::printf("{\"peak\": %u, \"sum\": %lld, \"e_lo\": \"%llu\", \"e_hi\": \"%llu\", \"energy\": \"%llu\"}\n", a.peak,
                    (long long)a.sum, (unsigned long long)a.e_lo, (unsigned long long)a.e_hi,
                    (unsigned long long)bits_of(levels::acc_energy(a)));
        return 0;
    }
    if (mode == "geom" && argc == 5) {
        const uint64_t n = std::strtoull(argv[2], nullptr, 10);
        const uint32_t hop = (uint32_t)std::strtoul(argv[3], nullptr, 10), per = (uint32_t)std::atoi(argv[4]);
        const levels::Plan pl = levels::plan(hop, per);
        const uint64_t tiles = levels::n_tiles(n, pl);
        std::printf("{\"blocks\": %llu, \"T\": %u, \"mode\": %u, \"group\": %u, \"parts\": %llu, \"partials\": %llu, \"last\": %llu, "
                    "\"too_small_at\": [%d, %d], \"tiles\": [",
                    (unsigned long long)levels::n_blocks(n, hop), pl.T, pl.mode, pl.group, (unsigned long long)pl.parts,
                    (unsigned long long)levels::partial_records(n, pl, 3u),
                    (unsigned long long)(levels::n_blocks(n, hop) ? levels::block_len(n, hop, levels::n_blocks(n, hop) - 1u) : 0u),
                    (int)levels::too_small(n, hop, 3u, 3u * levels::n_blocks(n, hop)),
                    (int)(levels::n_blocks(n, hop) ? levels::too_small(n, hop, 3u, 3u * levels::n_blocks(n, hop) - 1u) : 0));
        for (uint64_t k = 0; k < tiles; k++) {
            const levels::Tile t = levels::tile_at(n, pl, k);
            std::printf("%s[%llu, %u, %llu, %u]", k ? ", " : "", (unsigned long long)t.t0, t.ns, (unsigned long long)t.block0, t.part);
        }
        std::printf("]}\n");
        return 0;
    }
    if (mode == "tile" && argc == 9) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        const uint32_t B = (uint32_t)std::atoi(argv[4]), C = (uint32_t)std::atoi(argv[5]);
        const uint64_t n = std::strtoull(argv[6], nullptr, 10);
        const uint32_t hop = (uint32_t)std::strtoul(argv[7], nullptr, 10), lead0 = (uint32_t)std::atoi(argv[8]);
        if (B < 1u || B > 4u || C < 1u || C > 8u || in.size() != n * C * 4u || lead0 > 7u) fail("bad tile arguments");
        const uint32_t per = C * B;
        std::vector<uint8_t> pcm(n * per);
        for (uint64_t i = 0; i < n * C; i++) {
            int32_t x;
            std::memcpy(&x, &in[4u * i], 4);
            for (uint32_t b = 0; b < B; b++) pcm[i * B + b] = (uint8_t)((uint32_t)x >> (8u * b));
        }
        const levels::Plan pl = levels::plan(hop, per);
        const uint64_t nb = levels::n_blocks(n, hop), tiles = levels::n_tiles(n, pl);
        std::vector<levels::Acc> acc(nb * C, levels::acc_zero());
        uint64_t words_read = 0;
        for (uint64_t k = 0; k < tiles; k++) {
            const levels::Tile tl = levels::tile_at(n, pl, k);
            // the address the kernel would see: the window's first byte at lead0, this tile t0 * per further
            const uint32_t lead_here = (uint32_t)((lead0 + tl.t0 * per) & 7u);
            const size_t held = (lead_here + (size_t)tl.ns * per + 7u) / 8u;
            uint8_t *src = (uint8_t *)words_alloc(held);
            std::memcpy(src + lead_here, &pcm[tl.t0 * per], (size_t)tl.ns * per);
            uint64_t a0;
            uint32_t lead, n_words;
            levels::tile_words((uint64_t)(uintptr_t)(src + lead_here), tl.ns, per, a0, lead, n_words);
            if (a0 != (uint64_t)(uintptr_t)src || lead != lead_here || n_words != held || n_words > deliver::kTileWords)
                fail("tile_words names other words than those that hold the tile");
            uint64_t *lds = (uint64_t *)words_alloc(n_words);
            for (uint32_t i = 0; i < n_words; i++) lds[i] = ((const uint64_t *)(uintptr_t)a0)[i];
            words_read += n_words;
            const uint32_t *words = (const uint32_t *)lds;
            if (pl.mode == levels::LV_PARTS) {
                for (uint32_t ch = 0; ch < C; ch++)
                    for (uint32_t tid = 0; tid < 256u; tid++)
                        levels::acc_merge(acc[tl.block0 * C + ch], levels::tile_acc(words, lead, per, B, ch, tid, tl.ns, 256u));
            } else {
                const uint32_t blocks = (tl.ns + hop - 1u) / hop, lanes = pl.mode == levels::LV_WAVES ? levels::kWave : 1u;
                for (uint32_t b = 0; b < blocks; b++) {
                    const uint32_t first = b * hop, end = first + hop < tl.ns ? first + hop : tl.ns;
                    for (uint32_t ch = 0; ch < C; ch++)
                        for (uint32_t lane = 0; lane < lanes; lane++)
                            levels::acc_merge(acc[(tl.block0 + b) * C + ch],
                                              levels::tile_acc(words, lead, per, B, ch, first + lane, end, lanes));
                }
            }
            std::free(lds);
            std::free(src);
        }
        std::vector<Rec> out(nb * C);
        for (uint64_t i = 0; i < nb * C; i++) out[i] = {acc[i].peak, 0u, acc[i].sum, bits_of(levels::acc_energy(acc[i]))};
        write_file(argv[3], out.data(), out.size() * sizeof(Rec));
        std::printf("{\"records\": %llu, \"tiles\": %llu, \"mode\": %u, \"words\": %llu}\n", (unsigned long long)(nb * C),
                    (unsigned long long)tiles, pl.mode, (unsigned long long)words_read);
        return 0;
    }
    fail("unknown mode or wrong argument count");
    return 2;
}
