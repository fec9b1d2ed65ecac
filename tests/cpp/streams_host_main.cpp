// streams_host_main.cpp -- the many-streams forms of libflacgpu.so's device index and decode run
// entirely on the host: the per-stream geometry, carving and dispatch of fg_index.hpp (the stages
// of fg_index.hip, stream by stream over one concatenated buffer, every stream's arrays a carve of
// one pool that is exactly as large as the totals say), and the segment rules of fg_streams.hpp
// (the cut into chunks, the per-frame PCM offsets, the fold of frame results).  A stand-alone
// program, built by tests/test_streams_host.py with -fsanitize=address,undefined.
//
//   streams_host_main index BLOB N  (OFFSET LEN BITS RATE CAP) x N
//       BLOB holds the streams at their OFFSETs (any alignment); CAP: the stream's table entries.
//       Prints {"streams": [{"status", "n_frames", "offsets": [...], "sizes": [...]}], "untouched": bool}
//       (offsets relative to the blob; untouched: table entries past every n_frames, the guard
//       entries between the slices and every non-OK stream's slice still hold the fill).
//   streams_host_main segments MAX_FRAMES PER SEED  (FRAMES CAP_FRAMES) x N
//       N streams of FRAMES frames with block sizes and statuses drawn from SEED; stream s's PCM
//       region holds what its first CAP_FRAMES frames need.  Checks the offsets and the folded
//       results against plain loops (exit 1 on a difference) and prints {"segments": [[stream,
//       first, count, frame0, packed]], "chunks": [first segment of each chunk, ..., n_segments]}.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zig-flac_amd/csrc/fg_index.hpp"
#include "../../zig-flac_amd/csrc/fg_streams.hpp"

using namespace fg;
using namespace fg::idx;

namespace {

constexpr uint32_t GUARD = 3;  // table entries between two streams' slices

uint32_t mask_window(const uint64_t *m, uint64_t n_chunks, int64_t v) {
    const int64_t jj = v >> 6;
    const uint32_t sh = (uint32_t)(v & 63);
    const uint64_t lo = (jj >= 0 && (uint64_t)jj < n_chunks) ? m[jj] : 0ull;
    uint64_t r = lo >> sh;
    if (sh > 32u) {
        const uint64_t hi = (jj + 1 >= 0 && (uint64_t)(jj + 1) < n_chunks) ? m[jj + 1] : 0ull;
        r |= hi << (64u - sh);
    }
    return (uint32_t)r;
}

uint32_t cand_hdr(const IdxArgs &g, int64_t v) {
    const uint64_t x = (uint64_t)v - g.lead;
    uint32_t h = 0;
    return header_at(g.data + x, g.len - x, g.bits, g.rate, &h) ? h : 0u;
}

// one "workgroup" (blockIdx.x = grp) of each stage for stream g; it has exited if grp >= n_groups
void stage_terms(const IdxArgs &g, uint32_t grp) {
    uint32_t x = 0;
    for (uint64_t j = (uint64_t)grp * kIdxGroup; j < g.n_chunks && j < (uint64_t)(grp + 1u) * kIdxGroup; j++) {
        uint64_t a, b;
        chunk_bounds(j, kIdxChunk, g.lead, g.len, &a, &b);
        const uint32_t term = chunk_term(dec::crc16_bytes(g.data + a, (uint32_t)(b - a)), b);
        g.terms[j] = (uint16_t)term;
        x ^= term;
    }
    g.grp[grp] = x;
}
template <bool ADD>
void stage_scan(uint32_t *v, uint32_t n, uint32_t *total) {
    uint32_t carry = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t t = v[i];
        v[i] = carry;
        carry = ADD ? carry + t : carry ^ t;
    }
    *total = carry;
}
void stage_cands(const IdxArgs &g, uint32_t grp) {
    uint32_t q = g.grp[grp];
    for (uint64_t j = (uint64_t)grp * kIdxGroup; j < g.n_chunks && j < (uint64_t)(grp + 1u) * kIdxGroup; j++) {
        uint64_t a, b;
        chunk_bounds(j, kIdxChunk, g.lead, g.len, &a, &b);
        uint32_t P = running_crc(q, a);
        uint64_t mask = 0;
        for (uint64_t x = a; x < b; x++) {
            const uint32_t next = x + 1 < g.len ? g.data[x + 1] : 0u;
            if (is_candidate(P, g.data[x], next, g.data, g.len, x, g.bits, g.rate)) mask |= 1ull << ((x + g.lead) & 63u);
            P = crc_byte_v(P, g.data[x]);
        }
        g.cmask[j] = mask;
        g.smask[j] = 0;
        q ^= g.terms[j];
    }
}
void stage_resolve(const IdxArgs &g, uint32_t grp) {
    auto win = [&](int64_t v) { return mask_window(g.cmask, g.n_chunks, v); };
    auto hdr_of = [&](int64_t v) { return cand_hdr(g, v); };
    auto mark = [&](int64_t v) {
        if (v < 0 || (uint64_t)(v >> 6) >= g.n_chunks) std::abort();
        g.smask[v >> 6] |= 1ull << (v & 63);
    };
    for (uint64_t j = (uint64_t)grp * kIdxGroup; j < g.n_chunks && j < (uint64_t)(grp + 1u) * kIdxGroup; j++)
        for (uint64_t m = g.cmask[j]; m; m &= m - 1u)
            resolve_from((int64_t)(j * kIdxChunk + (uint64_t)__builtin_ctzll(m)), win, hdr_of, mark);
}
void stage_count(const IdxArgs &g, uint32_t grp) {
    uint32_t n = 0;
    for (uint64_t j = (uint64_t)grp * kIdxGroup; j < g.n_chunks && j < (uint64_t)(grp + 1u) * kIdxGroup; j++)
        n += (uint32_t)__builtin_popcountll(g.smask[j]);
    g.gcnt[grp] = n;
}
void stage_place(const IdxArgs &g, uint32_t grp) {
    uint64_t rank = g.gcnt[grp];
    const uint64_t n = g.ctl[1];
    for (uint64_t j = (uint64_t)grp * kIdxGroup; j < g.n_chunks && j < (uint64_t)(grp + 1u) * kIdxGroup; j++)
        for (uint64_t m = g.smask[j]; m; m &= m - 1u, rank++) {
            const int64_t v = (int64_t)(j * kIdxChunk + (uint64_t)__builtin_ctzll(m));
            const uint64_t x = (uint64_t)v - g.lead;
            if (rank < g.spos_cap) g.spos[rank] = (uint32_t)x;
            if (rank + 1u == n) {
                const bool cand0 = (mask_window(g.cmask, g.n_chunks, (int64_t)g.lead) & 1u) != 0;
                const uint32_t st = verdict(cand0, g.ctl[0], x, cand_hdr(g, v), g.len, n, g.cap);
                g.res->n_frames = st == IDX_INVALID ? 0ull : n;
                g.res->status = st;
                g.res->reserved = 0;
            }
        }
}
void stage_emit(const IdxArgs &g) {
    if (g.res->status != IDX_OK) return;
    const uint64_t n = g.res->n_frames;
    if (n > g.spos_cap) return;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t s = g.spos[i], e = i + 1u < n ? (uint64_t)g.spos[i + 1u] : g.len;
        g.offs[i] = g.base_off + s;
        g.bytes[i] = (uint32_t)(e - s);
    }
}

int run_index(int argc, char **argv) {
    if (argc < 4) return 2;
    const uint32_t n = (uint32_t)std::atoi(argv[3]);
    if (argc != 4 + 5 * (int)n || n == 0 || n > kIdxMaxStreams) return 2;
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const uint64_t blob_len = (uint64_t)std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    // exactly blob_len bytes, so a read outside them is a heap overflow; the streams' leads come from their addresses
    uint8_t *blob = (uint8_t *)std::malloc(blob_len ? blob_len : 1);
    if (blob_len && std::fread(blob, 1, blob_len, f) != blob_len) return 2;
    std::fclose(f);

    std::vector<IdxArgs> tab(n, IdxArgs{});
    std::vector<uint64_t> first(n), caps(n);
    uint64_t entries = GUARD;
    for (uint32_t s = 0; s < n; s++) {
        caps[s] = (uint64_t)std::atoll(argv[4 + 5 * s + 4]);
        first[s] = entries;
        entries += caps[s] + GUARD;
    }
    std::vector<uint64_t> offs(entries, 0xA5A5A5A5A5A5A5A5ull);
    std::vector<uint32_t> bytes(entries, 0xA5A5A5A5u);
    std::vector<IndexResult> res(n);
    IdxTotals tot;
    for (uint32_t s = 0; s < n; s++) {
        IdxArgs &g = tab[s];
        const uint64_t off = (uint64_t)std::atoll(argv[4 + 5 * s]), len = (uint64_t)std::atoll(argv[4 + 5 * s + 1]);
        if (off + len > blob_len) return 2;
        g.data = blob + off;
        stream_geometry(g, (uint64_t)(uintptr_t)g.data, len, caps[s]);
        g.bits = (uint32_t)std::atoi(argv[4 + 5 * s + 2]);
        g.rate = (uint32_t)std::atoi(argv[4 + 5 * s + 3]);
        g.offs = offs.data() + first[s];
        g.bytes = bytes.data() + first[s];
        g.res = &res[s];
        g.base_off = off;
        totals_add(tot, g);
    }
    // the pool: every array exactly as long as the totals say, so a carve that runs over is a heap overflow
    std::vector<uint64_t> cmask(tot.chunks), smask(tot.chunks);
    std::vector<uint32_t> grp(tot.groups), gcnt(tot.groups), ctl(4u * n), spos(tot.spos);
    std::vector<uint16_t> terms(tot.chunks);
    const IdxPool pool{cmask.data(), smask.data(), grp.data(), gcnt.data(), ctl.data(), spos.data(), terms.data()};
    IdxTotals at;
    for (uint32_t s = 0; s < n; s++) carve_stream(tab[s], pool, at);
    if (at.chunks != tot.chunks || at.groups != tot.groups || at.spos != tot.spos || at.max_groups != tot.max_groups) return 1;

    // the dispatch of launch_index_streams: each stage once over (group x, stream y); a "workgroup" past
    // its stream's groups exits
    auto grid = [&](void (*stage)(const IdxArgs &, uint32_t)) {
        for (uint32_t y = 0; y < n; y++)
            for (uint32_t x = 0; x < tot.max_groups; x++)
                if (x < tab[y].n_groups) stage(tab[y], x);
    };
    grid(stage_terms);
    for (uint32_t y = 0; y < n; y++)
        if (tab[y].len) stage_scan<false>(tab[y].grp, tab[y].n_groups, tab[y].ctl);
    grid(stage_cands);
    grid(stage_resolve);
    grid(stage_count);
    for (uint32_t y = 0; y < n; y++) {
        const IdxArgs &g = tab[y];
        if (g.len == 0) {
            *g.res = IndexResult{0, IDX_OK, 0};
            continue;
        }
        stage_scan<true>(g.gcnt, g.n_groups, g.ctl + 1);
        *g.res = IndexResult{0, IDX_INVALID, 0};
    }
    grid(stage_place);
    for (uint32_t y = 0; y < n; y++) stage_emit(tab[y]);

    bool untouched = true;
    std::vector<uint8_t> written(entries, 0);
    for (uint32_t s = 0; s < n; s++)
        if (res[s].status == IDX_OK)
            for (uint64_t i = 0; i < res[s].n_frames; i++) written[first[s] + i] = 1;
    for (uint64_t i = 0; i < entries; i++)
        if (!written[i] && (offs[i] != 0xA5A5A5A5A5A5A5A5ull || bytes[i] != 0xA5A5A5A5u)) untouched = false;
    std::printf("{\"streams\": [");
    for (uint32_t s = 0; s < n; s++) {
        std::printf("%s{\"status\": %u, \"n_frames\": %llu, \"offsets\": [", s ? ", " : "", res[s].status,
                    (unsigned long long)res[s].n_frames);
        const uint64_t m = res[s].status == IDX_OK ? res[s].n_frames : 0;
        for (uint64_t i = 0; i < m; i++) std::printf("%s%llu", i ? ", " : "", (unsigned long long)offs[first[s] + i]);
        std::printf("], \"sizes\": [");
        for (uint64_t i = 0; i < m; i++) std::printf("%s%u", i ? ", " : "", bytes[first[s] + i]);
        std::printf("]}");
    }
    std::printf("], \"untouched\": %s}\n", untouched ? "true" : "false");
    std::free(blob);
    return 0;
}

uint64_t rng_state;
uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

int run_segments(int argc, char **argv) {
    if (argc < 5 || (argc - 5) % 2) return 2;
    const uint32_t max_frames = (uint32_t)std::atoi(argv[2]), per = (uint32_t)std::atoi(argv[3]);
    rng_state = (uint64_t)std::atoll(argv[4]) * 2u + 1u;
    const uint32_t n = (uint32_t)(argc - 5) / 2u;
    if (max_frames == 0 || per == 0) return 2;
    using namespace fg::streams;
    std::vector<uint64_t> frames(n), cap_frames(n), base(n), cap(n);
    std::vector<std::vector<uint32_t>> block(n), status(n);
    uint64_t at = 64;
    for (uint32_t s = 0; s < n; s++) {
        frames[s] = (uint64_t)std::atoll(argv[5 + 2 * s]);
        cap_frames[s] = (uint64_t)std::atoll(argv[5 + 2 * s + 1]);
        uint64_t need = 0;
        for (uint64_t i = 0; i < frames[s]; i++) {
            const uint32_t r = rnd() % 8u;
            // 0: a header that did not parse (block 0, status HEADER); 1: damaged after a good header
            status[s].push_back(r == 0 ? dec::ST_HEADER : r == 1 ? dec::ST_CRC16 : dec::ST_OK);
            block[s].push_back(r == 0 ? 0u : (i + 1 == frames[s] ? 1u + rnd() % 256u : 256u));
            if (i < cap_frames[s]) need += (uint64_t)block[s].back() * per;
        }
        base[s] = at;
        cap[s] = need;
        at += need + 64;
    }
    std::vector<Segment> segs;
    std::vector<uint32_t> chunk_seg;
    cut_segments(frames, max_frames, segs, chunk_seg);
    // the plain loops: every stream's frames in order
    std::vector<std::vector<uint64_t>> want_off(n);
    std::vector<StreamResult> want(n), got(n);
    for (uint32_t s = 0; s < n; s++) {
        want[s] = got[s] = StreamResult{frames[s], 0, 0, 0, kNone, 0};
        uint64_t before = 0;
        for (uint64_t i = 0; i < frames[s]; i++) {
            const uint64_t rel = before * per, nb = (uint64_t)block[s][i] * per;
            const bool fits = rel + nb <= cap[s];
            want_off[s].push_back(fits ? base[s] + rel : kRefuse);
            uint32_t st = status[s][i];
            if (st == 0 && !fits) st = dec::ST_RANGE;
            if (st == 0) want[s].n_samples += block[s][i];
            else {
                want[s].bad_frames++;
                if (want[s].first_bad_frame == kNone) {
                    want[s].first_bad_frame = (uint32_t)i;
                    want[s].first_bad_status = st;
                }
            }
            before += block[s][i];
        }
    }
    // the chunks, as the kernels run them: one "wave" of 64 lanes per segment
    std::vector<uint64_t> carried(n, 0);
    const uint32_t n_chunks = chunk_seg.empty() ? 0u : (uint32_t)chunk_seg.size() - 1u;
    for (uint32_t k = 0; k < n_chunks; k++) {
        const Segment &last = segs[chunk_seg[k + 1] - 1u];
        const uint32_t nf = last.first + last.count;
        if (nf > max_frames || (k + 1u < n_chunks && nf != max_frames)) return 1;
        // exactly the chunk's frames: a segment that runs over is a heap overflow
        std::vector<uint32_t> blocks(nf, 0xA5A5A5A5u), stat(nf, 0xA5A5A5A5u);
        std::vector<uint64_t> pcm_off(nf, 0x5A5A5A5A5A5A5A5Aull);
        uint32_t expect_first = 0;
        for (uint32_t q = chunk_seg[k]; q < chunk_seg[k + 1]; q++) {
            const Segment &g = segs[q];
            if (g.first != expect_first || g.count == 0 || g.packed != (uint64_t)k * max_frames + g.first) return 1;
            expect_first += g.count;
            for (uint32_t i = 0; i < g.count; i++) blocks[g.first + i] = block[g.stream][g.frame0 + i];
        }
        for (uint32_t q = chunk_seg[k]; q < chunk_seg[k + 1]; q++) {  // k_seg_offsets
            const Segment &g = segs[q];
            uint64_t carry = carried[g.stream];
            for (uint32_t i0 = 0; i0 < g.count; i0 += 64u) {
                uint64_t inc = 0;
                for (uint32_t lane = 0; lane < 64u && i0 + lane < g.count; lane++) {
                    const uint32_t x = blocks[g.first + i0 + lane];
                    pcm_off[g.first + i0 + lane] = frame_pcm_offset(base[g.stream], cap[g.stream], carry + inc, x, per);
                    inc += x;
                }
                carry += inc;
            }
            carried[g.stream] = carry;
        }
        for (uint32_t q = chunk_seg[k]; q < chunk_seg[k + 1]; q++) {  // the reconstruct's capacity check, then k_seg_fold
            const Segment &g = segs[q];
            for (uint32_t i = 0; i < g.count; i++) {
                if (pcm_off[g.first + i] != want_off[g.stream][g.frame0 + i]) {
                    std::fprintf(stdout, "offset differs: stream %u frame %u\n", g.stream, g.frame0 + i);
                    return 1;
                }
                uint32_t st = status[g.stream][g.frame0 + i];
                if (st == 0 && pcm_off[g.first + i] == kRefuse) st = dec::ST_RANGE;
                stat[g.first + i] = st;
            }
            Fold lanes[64];
            for (uint32_t i = 0; i < g.count; i++) fold_frame(lanes[i & 63u], i, stat[g.first + i], blocks[g.first + i]);
            for (uint32_t d = 32; d >= 1; d >>= 1)
                for (uint32_t l = 0; l < d; l++) fold_merge(lanes[l], lanes[l + d]);
            fold_into(got[g.stream], lanes[0], g.frame0);
        }
    }
    for (uint32_t s = 0; s < n; s++)
        if (std::memcmp(&got[s], &want[s], sizeof(StreamResult)) != 0) {
            std::fprintf(stdout, "result differs: stream %u\n", s);
            return 1;
        }
    std::printf("{\"segments\": [");
    for (size_t q = 0; q < segs.size(); q++)
        std::printf("%s[%u, %u, %u, %u, %llu]", q ? ", " : "", segs[q].stream, segs[q].first, segs[q].count, segs[q].frame0,
                    (unsigned long long)segs[q].packed);
    std::printf("], \"chunks\": [");
    for (size_t k = 0; k < chunk_seg.size(); k++) std::printf("%s%u", k ? ", " : "", chunk_seg[k]);
    std::printf("]}\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && std::strcmp(argv[1], "index") == 0) return run_index(argc, argv);
    if (argc >= 2 && std::strcmp(argv[1], "segments") == 0) return run_segments(argc, argv);
    std::fprintf(stderr, "usage: streams_host_main index BLOB N (OFFSET LEN BITS RATE CAP)... | segments MAX PER SEED (FRAMES CAP_FRAMES)...\n");
    return 2;
}
