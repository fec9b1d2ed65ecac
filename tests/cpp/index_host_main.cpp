// index_host_main.cpp -- the frame index of libflacgpu.so's device path
// (zig-flac_amd/csrc/fg_index.hpp) run entirely on the host, stage by stage as the kernels of
// fg_index.hip run it, but serially and with the chunk geometry given on the command line.  A
// stand-alone program, built by tests/test_index_host.py with -fsanitize=address,undefined: every
// byte the shared code reads for good and for crafted streams is checked here before a GPU sees
// such input.
//
//   index_host_main DATA STREAM_BITS STREAM_RATE CHUNK GROUP [LEAD]
//
// DATA: a bare run of frames.  CHUNK: bytes per "lane"; GROUP: chunks per "workgroup"; LEAD: the
// data starts LEAD bytes into the first chunk (the device aligns chunks to the address).  Prints
// {"status": 0|1, "n_frames": n, "sizes": [...]}.  The data is copied into an allocation of
// exactly its length first, so a read outside it is a heap overflow the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_index.hpp"

using namespace fg;
using namespace fg::idx;

int main(int argc, char **argv) {
    if (argc < 6) {
        std::fprintf(stderr, "usage: index_host_main DATA STREAM_BITS STREAM_RATE CHUNK GROUP [LEAD]\n");
        return 2;
    }
    const uint32_t bits = (uint32_t)std::atoi(argv[2]), rate = (uint32_t)std::atoi(argv[3]);
    const uint32_t C = (uint32_t)std::atoi(argv[4]), G = (uint32_t)std::atoi(argv[5]);
    const uint32_t lead = argc > 6 ? (uint32_t)std::atoi(argv[6]) : 0u;
    if (C == 0 || G == 0 || lead >= C) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const uint64_t len = (uint64_t)std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t *data = (uint8_t *)std::malloc(len ? len : 1);  // exactly len bytes when there are any
    if (len && std::fread(data, 1, len, f) != len) return 2;
    std::fclose(f);
    if (len == 0) {
        std::printf("{\"status\": 0, \"n_frames\": 0, \"sizes\": []}\n");
        std::free(data);
        return 0;
    }

    const uint64_t n_chunks = (lead + len + C - 1) / C, n_groups = (n_chunks + G - 1) / G;
    // stage 1: every chunk's term, every group's XOR of them
    std::vector<uint32_t> term(n_chunks), grp(n_groups, 0);
    for (uint64_t j = 0; j < n_chunks; j++) {
        uint64_t a, b;
        chunk_bounds(j, C, lead, len, &a, &b);
        term[j] = chunk_term(dec::crc16_bytes(data + a, (uint32_t)(b - a)), b);
        grp[j / G] ^= term[j];
    }
    // stage 2: exclusive XOR scan of the group sums; the total is Q at the end of the data
    uint32_t q_end = 0;
    for (uint64_t g = 0; g < n_groups; g++) {
        const uint32_t t = grp[g];
        grp[g] = q_end;
        q_end ^= t;
    }
    // stage 3: candidates; every chunk starts from its own Q
    std::vector<uint8_t> cand(len, 0), sel(len, 0);
    for (uint64_t g = 0; g < n_groups; g++) {
        uint32_t q = grp[g];
        for (uint64_t j = g * G; j < n_chunks && j < (g + 1) * G; j++) {
            uint64_t a, b;
            chunk_bounds(j, C, lead, len, &a, &b);
            uint32_t P = running_crc(q, a);
            for (uint64_t x = a; x < b; x++) {
                const uint32_t next = x + 1 < len ? data[x + 1] : 0u;
                if (is_candidate(P, data[x], next, data, len, x, bits, rate)) cand[x] = 1;
                P = crc_byte_v(P, data[x]);
            }
            q ^= term[j];
        }
    }
    // stage 4: the minimum-distance rule, one "lane" per candidate
    auto win = [&](int64_t v) {
        uint32_t w = 0;
        for (int k = 0; k < 32; k++)
            if (v + k >= 0 && (uint64_t)(v + k) < len && cand[(size_t)(v + k)]) w |= 1u << k;
        return w;
    };
    auto hdr_of = [&](int64_t v) {
        uint32_t h = 0;
        if (!header_at(data + v, len - (uint64_t)v, bits, rate, &h)) std::abort();  // only asked of candidates
        return h;
    };
    auto mark = [&](int64_t v) {
        if (v < 0 || (uint64_t)v >= len || !cand[(size_t)v]) std::abort();
        sel[(size_t)v] = 1;
    };
    for (uint64_t x = 0; x < len; x++)
        if (cand[x]) resolve_from((int64_t)x, win, hdr_of, mark);
    // stages 5-8: count, place, verdict, sizes
    std::vector<uint64_t> starts;
    for (uint64_t x = 0; x < len; x++)
        if (sel[x]) starts.push_back(x);
    uint32_t last_hdr = 0;
    if (!starts.empty()) last_hdr = hdr_of((int64_t)starts.back());
    const uint32_t st = verdict(cand[0] != 0, q_end, starts.empty() ? 0 : starts.back(), last_hdr, len, starts.size(), ~0ull);
    std::printf("{\"status\": %u, \"n_frames\": %llu, \"sizes\": [", st, st ? 0ull : (unsigned long long)starts.size());
    if (st == IDX_OK)
        for (size_t i = 0; i < starts.size(); i++)
            std::printf("%s%llu", i ? ", " : "",
                        (unsigned long long)((i + 1 < starts.size() ? starts[i + 1] : len) - starts[i]));
    std::printf("]}\n");
    std::free(data);
    return 0;
}
