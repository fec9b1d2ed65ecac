// fg_index.hip -- the device frame index (gfx950): the frame offsets and sizes of a bare run of
// FLAC frames resident in HBM, equal to what the host index (fg_dec_api.cpp index_frames) finds.
// The method and its scalar pieces are fg_index.hpp's; here one lane owns a 64-byte chunk of the
// data and a workgroup of 256 lanes a 16 KiB group.  Chunks are aligned to the ADDRESS, so an
// inner chunk is four aligned 16-byte loads whatever the base's alignment; the first and the last
// chunk go byte by byte inside [data, data + len).
//
//   k_idx_terms    per chunk: CRC-16 of its bytes times z^(-8 end) -> terms[]; per group: their XOR
//   k_idx_scan     one workgroup: exclusive scan of the group sums (XOR); the total is Q(len)
//   k_idx_cands    per chunk: Q at its start (group prefix ^ wave/workgroup scan of the terms), the
//                  running CRC from there byte by byte, a bit per candidate -> cmask[]
//   k_idx_resolve  per candidate: the minimum-distance rule (resolve_from) -> smask[] (atomicOr: a
//                  walk may mark a start in another lane's chunk)
//   k_idx_count    per group: number of frame starts
//   k_idx_scan     exclusive scan of those (add); the total is the frame count
//   k_idx_place    per frame start: its rank -> spos[rank]; the last one writes the verdict
//   k_idx_emit     per frame: offset and size, only when the verdict is OK
//
// Every stage is its own launch and reads the counts of the stage before from device memory: no
// workgroup waits on another, and the host sizes every grid from len and cap alone.
//
// Many streams in one call (launch_index_streams): the same kernels instantiated with MANY, each
// picking its stream's IdxArgs from a table in device memory by blockIdx.y; the grids' x extents
// are the longest stream's, and a workgroup past its stream's groups exits at once.  The
// one-stream instances take their IdxArgs by value as before.
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_index.hpp"

namespace fg {

using namespace idx;

namespace {

constexpr uint32_t kChunk = kIdxChunk, kGroup = kIdxGroup;
static_assert(kChunk == 64, "one mask bit per byte of a chunk");

__device__ __forceinline__ uint32_t wave_xor_all(uint32_t x) {
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) x ^= __shfl_xor(x, d, 64);
    return x;
}
template <bool ADD>
__device__ __forceinline__ uint32_t wave_incl(uint32_t x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x = ADD ? x + y : x ^ y;
    }
    return x;
}
// exclusive scan over the workgroup (blockDim.x / 64 <= 16 waves); *total: the sum of all lanes
template <bool ADD>
__device__ __forceinline__ uint32_t block_excl(uint32_t x, uint32_t *s_wave, uint32_t *total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, nw = blockDim.x >> 6;
    const uint32_t inc = wave_incl<ADD>(x, lane);
    __syncthreads();  // s_wave may still be read from a previous call
    if (lane == 63u) s_wave[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t v = s_wave[w];
        if (w < wv) before = ADD ? before + v : before ^ v;
        all = ADD ? all + v : all ^ v;
    }
    *total = all;
    return ADD ? before + inc - x : before ^ inc ^ x;
}

// the chunk is whole and inside the data: its 64 bytes are four aligned 16-byte words
__device__ __forceinline__ bool chunk_is_inner(uint64_t a, uint64_t b) { return b - a == kChunk; }
__device__ __forceinline__ void load_inner(const IdxArgs &g, uint64_t a, uint32_t (&w)[16]) {
    const uint4 *p = (const uint4 *)(g.data + a);  // data + a is 16-byte aligned: a + lead is a multiple of 64
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 v = p[k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
    }
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[16], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// ---------------------------------------------------------------------------------------------
template <bool MANY>
__global__ void __launch_bounds__(kGroup) k_idx_terms(IdxArgs g0, const IdxArgs *tab) {
    IdxArgs g = g0;
    if constexpr (MANY) {
        g = tab[blockIdx.y];
        if (blockIdx.x >= g.n_groups) return;
    }
    __shared__ uint32_t s_x[kGroup / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * kGroup + tid;
    uint32_t term = 0;
    if (j < g.n_chunks) {
        uint64_t a, b;
        chunk_bounds(j, kChunk, g.lead, g.len, &a, &b);
        uint32_t crc = 0;
        if (chunk_is_inner(a, b)) {
            uint32_t w[16];
            load_inner(g, a, w);
#pragma unroll
            for (int k = 0; k < 64; k++) crc = crc_byte_v(crc, byte_of(w, k));
        } else {
            for (uint64_t x = a; x < b; x++) crc = crc_byte_v(crc, g.data[x]);
        }
        term = chunk_term(crc, b);
        g.terms[j] = (uint16_t)term;
    }
    const uint32_t x = wave_xor_all(term);
    if ((tid & 63u) == 0) s_x[tid >> 6] = x;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kGroup / 64; w++) t ^= s_x[w];
        g.grp[blockIdx.x] = t;
    }
}

// One workgroup: v[0, n) becomes its exclusive scan (XOR or add), *total the sum.  With a result:
// the default verdict (no frame start found: INVALID) that k_idx_place's last frame start replaces.
template <bool ADD>
__device__ __forceinline__ void scan_one(uint32_t *v, uint32_t n, uint32_t *total, IndexResult *res) {
    __shared__ uint32_t s_wave[16];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < n ? v[i] : 0u;
        uint32_t all;
        const uint32_t ex = block_excl<ADD>(x, s_wave, &all);
        if (i < n) v[i] = ADD ? carry + ex : carry ^ ex;
        carry = ADD ? carry + all : carry ^ all;
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (res) {
            res->n_frames = 0;
            res->status = IDX_INVALID;
            res->reserved = 0;
        }
    }
}
template <bool ADD>
__global__ void __launch_bounds__(1024) k_idx_scan(uint32_t *v, uint32_t n, uint32_t *total, IndexResult *res) {
    scan_one<ADD>(v, n, total, res);
}
// many streams: workgroup s scans stream s's group sums; a stream of no bytes is OK with 0 frames
template <bool ADD>
__global__ void __launch_bounds__(1024) k_idx_scan_streams(const IdxArgs *tab) {
    const IdxArgs g = tab[blockIdx.x];
    if (g.len == 0) {
        if (ADD && threadIdx.x == 0) {
            g.res->n_frames = 0;
            g.res->status = IDX_OK;
            g.res->reserved = 0;
        }
        return;
    }
    if constexpr (ADD) scan_one<true>(g.gcnt, g.n_groups, g.ctl + 1, g.res);
    else scan_one<false>(g.grp, g.n_groups, g.ctl, nullptr);
}

// 32 mask bits from grid position v on (v may be negative or past the end: zeros there)
__device__ __forceinline__ uint32_t mask_window(const uint64_t *m, uint64_t n_chunks, int64_t v) {
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
// header length of the clean header at grid position v (inside the data), 0: none there
__device__ __noinline__ uint32_t cand_hdr(const IdxArgs &g, int64_t v) {
    const uint64_t x = (uint64_t)v - g.lead;
    uint32_t h = 0;
    return header_at(g.data + x, g.len - x, g.bits, g.rate, &h) ? h : 0u;
}

template <bool MANY>
__global__ void __launch_bounds__(kGroup) k_idx_cands(IdxArgs g0, const IdxArgs *tab) {
    IdxArgs g = g0;
    if constexpr (MANY) {
        g = tab[blockIdx.y];
        if (blockIdx.x >= g.n_groups) return;
    }
    __shared__ uint32_t s_wave[kGroup / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)blockIdx.x * kGroup + tid;
    const bool live = j < g.n_chunks;
    uint32_t all;
    const uint32_t q = g.grp[blockIdx.x] ^ block_excl<false>(live ? g.terms[j] : 0u, s_wave, &all);
    if (!live) return;
    uint64_t a, b;
    chunk_bounds(j, kChunk, g.lead, g.len, &a, &b);
    uint32_t P = running_crc(q, a);
    uint64_t mask = 0;
    if (chunk_is_inner(a, b)) {
        uint32_t w[16];
        load_inner(g, a, w);
        const uint32_t after = b < g.len ? g.data[b] : 0u;
#pragma unroll
        for (int k = 0; k < 64; k++) {
            const uint32_t byte = byte_of(w, k), next = k < 63 ? byte_of(w, (k + 1) & 63) : after;
            if (sync_at_zero(P, byte, next)) mask |= 1ull << k;
            P = crc_byte_v(P, byte);
        }
    } else {
        for (uint64_t x = a; x < b; x++) {
            const uint32_t byte = g.data[x], next = x + 1 < g.len ? g.data[x + 1] : 0u;
            if (sync_at_zero(P, byte, next)) mask |= 1ull << ((x + g.lead) & 63u);
            P = crc_byte_v(P, byte);
        }
    }
    // the header parse, for the few positions that got this far (one copy of it, outside the byte loop)
    for (uint64_t m = mask; m; m &= m - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctzll(m);
        if (cand_hdr(g, (int64_t)(j * kChunk + k)) == 0) mask &= ~(1ull << k);
    }
    g.cmask[j] = mask;
    g.smask[j] = 0;
}

template <bool MANY>
__global__ void __launch_bounds__(kGroup) k_idx_resolve(IdxArgs g0, const IdxArgs *tab) {
    IdxArgs g = g0;
    if constexpr (MANY) {
        g = tab[blockIdx.y];
        if (blockIdx.x >= g.n_groups) return;
    }
    const uint64_t j = (uint64_t)blockIdx.x * kGroup + threadIdx.x;
    if (j >= g.n_chunks) return;
    auto win = [&](int64_t v) { return mask_window(g.cmask, g.n_chunks, v); };
    auto hdr_of = [&](int64_t v) { return cand_hdr(g, v); };
    // a marked position is a candidate: inside the data, so inside smask[0, n_chunks)
    auto mark = [&](int64_t v) { atomicOr((unsigned long long *)&g.smask[v >> 6], 1ull << (v & 63)); };
    for (uint64_t m = g.cmask[j]; m; m &= m - 1u)
        resolve_from((int64_t)(j * kChunk + (uint64_t)__builtin_ctzll(m)), win, hdr_of, mark);
}

template <bool MANY>
__global__ void __launch_bounds__(kGroup) k_idx_count(IdxArgs g0, const IdxArgs *tab) {
    IdxArgs g = g0;
    if constexpr (MANY) {
        g = tab[blockIdx.y];
        if (blockIdx.x >= g.n_groups) return;
    }
    __shared__ uint32_t s_wave[kGroup / 64];
    const uint64_t j = (uint64_t)blockIdx.x * kGroup + threadIdx.x;
    uint32_t all;
    block_excl<true>(j < g.n_chunks ? (uint32_t)__builtin_popcountll(g.smask[j]) : 0u, s_wave, &all);
    if (threadIdx.x == 0) g.gcnt[blockIdx.x] = all;
}

template <bool MANY>
__global__ void __launch_bounds__(kGroup) k_idx_place(IdxArgs g0, const IdxArgs *tab) {
    IdxArgs g = g0;
    if constexpr (MANY) {
        g = tab[blockIdx.y];
        if (blockIdx.x >= g.n_groups) return;
    }
    __shared__ uint32_t s_wave[kGroup / 64];
    const uint64_t j = (uint64_t)blockIdx.x * kGroup + threadIdx.x;
    const uint64_t sel = j < g.n_chunks ? g.smask[j] : 0ull;
    uint32_t all;
    uint64_t rank = (uint64_t)g.gcnt[blockIdx.x] + block_excl<true>((uint32_t)__builtin_popcountll(sel), s_wave, &all);
    const uint64_t n = g.ctl[1];
    for (uint64_t m = sel; m; m &= m - 1u, rank++) {
        const int64_t v = (int64_t)(j * kChunk + (uint64_t)__builtin_ctzll(m));
        const uint64_t x = (uint64_t)v - g.lead;
        if (rank < g.spos_cap) g.spos[rank] = (uint32_t)x;
        if (rank + 1u == n) {  // the last frame start: the verdict
            const bool cand0 = (mask_window(g.cmask, g.n_chunks, (int64_t)g.lead) & 1u) != 0;
            const uint32_t st = verdict(cand0, g.ctl[0], x, cand_hdr(g, v), g.len, n, g.cap);
            g.res->n_frames = st == IDX_INVALID ? 0ull : n;
            g.res->status = st;
            g.res->reserved = 0;
        }
    }
}

template <bool MANY>
__global__ void __launch_bounds__(256) k_idx_emit(IdxArgs g0, const IdxArgs *tab) {
    IdxArgs g = g0;
    if constexpr (MANY) g = tab[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (g.res->status != IDX_OK) return;
    const uint64_t n = g.res->n_frames;  // <= cap and <= spos_cap: a frame is at least 9 bytes
    if (i >= n || n > g.spos_cap) return;
    const uint64_t s = g.spos[i], e = i + 1u < n ? (uint64_t)g.spos[i + 1u] : g.len;
    g.offs[i] = g.base_off + s;
    g.bytes[i] = (uint32_t)(e - s);
}

}  // namespace

// queues the eight stages on st; g.len > 0
hipError_t launch_index(const IdxArgs &g, hipStream_t st) {
    const uint32_t ng = g.n_groups;
    const IdxArgs *one = nullptr;
    hipLaunchKernelGGL(k_idx_terms<false>, dim3(ng), dim3(kGroup), 0, st, g, one);
    hipLaunchKernelGGL(k_idx_scan<false>, dim3(1), dim3(1024), 0, st, g.grp, ng, g.ctl, (IndexResult *)nullptr);
    hipLaunchKernelGGL(k_idx_cands<false>, dim3(ng), dim3(kGroup), 0, st, g, one);
    hipLaunchKernelGGL(k_idx_resolve<false>, dim3(ng), dim3(kGroup), 0, st, g, one);
    hipLaunchKernelGGL(k_idx_count<false>, dim3(ng), dim3(kGroup), 0, st, g, one);
    hipLaunchKernelGGL(k_idx_scan<true>, dim3(1), dim3(1024), 0, st, g.gcnt, ng, g.ctl + 1, g.res);
    hipLaunchKernelGGL(k_idx_place<false>, dim3(ng), dim3(kGroup), 0, st, g, one);
    const uint64_t ne = (g.spos_cap + 255u) / 256u;
    if (ne) hipLaunchKernelGGL(k_idx_emit<false>, dim3((uint32_t)ne), dim3(256), 0, st, g, one);
    return hipGetLastError();
}

// The same eight stages, once, over the n <= kIdxMaxStreams streams of d_tab (device memory): the
// x extents come from the longest stream (max_groups groups, max_spos rank entries), y is the
// stream.  The launch count does not depend on n.
hipError_t launch_index_streams(const IdxArgs *d_tab, uint32_t n, uint32_t max_groups, uint64_t max_spos, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const IdxArgs none{};
    const dim3 grid(max_groups, n);
    if (max_groups) hipLaunchKernelGGL(k_idx_terms<true>, grid, dim3(kGroup), 0, st, none, d_tab);
    hipLaunchKernelGGL(k_idx_scan_streams<false>, dim3(n), dim3(1024), 0, st, d_tab);
    if (max_groups) {
        hipLaunchKernelGGL(k_idx_cands<true>, grid, dim3(kGroup), 0, st, none, d_tab);
        hipLaunchKernelGGL(k_idx_resolve<true>, grid, dim3(kGroup), 0, st, none, d_tab);
        hipLaunchKernelGGL(k_idx_count<true>, grid, dim3(kGroup), 0, st, none, d_tab);
    }
    hipLaunchKernelGGL(k_idx_scan_streams<true>, dim3(n), dim3(1024), 0, st, d_tab);
    if (max_groups) hipLaunchKernelGGL(k_idx_place<true>, grid, dim3(kGroup), 0, st, none, d_tab);
    const uint64_t ne = (max_spos + 255u) / 256u;
    if (ne) hipLaunchKernelGGL(k_idx_emit<true>, dim3((uint32_t)ne, n), dim3(256), 0, st, none, d_tab);
    return hipGetLastError();
}

}  // namespace fg
