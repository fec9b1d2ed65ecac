// fg_levels.hip -- the kernels of the level measurement (gfx950); the rules are fg_levels.hpp's.
//
//   k_window_levels  in the slot of k_window_copy, per window (blockIdx.y), after the last chunk:
//                    the peak, sum and energy of every block and channel of the window's decoded
//                    samples.  A workgroup takes tiles of at most tile_samples(per) samples that
//                    never cross a block boundary (levels::tile_at); the aligned 8-byte words that
//                    hold a tile go to LDS as in k_window_elements (no word past the one that holds
//                    the tile's last byte is read), and the tile is reduced out of LDS by its
//                    plan's mode: a thread a (block, channel) where a block is shorter than a wave,
//                    a wave a block where a tile holds several, all four waves where a block is a
//                    tile or longer.  Where a block has one part its three numbers are written at
//                    once; where it has several, every (block, part) leaves one exact Acc a channel
//   k_levels_fold    per window, only where blocks have several parts: a wave sums the parts of a
//                    (block, channel) and writes its three numbers
//
// Every accumulator is an integer and every combination exact, so the bits written depend on
// neither the grid nor the order in which workgroups run.  A window that is not clean writes
// nothing.  Bounds: a tile's words lie inside the window's covering frames in the scratch; record
// out_off[w] + j * C + c has j < ceil(n / hop), which the capacity rule has checked; partial
// (j * P + p) * C + c of a window lies below the n_blocks * P * C the host carved for it.
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_deliver.hpp"
#include "fg_device.hpp"
#include "fg_levels.hpp"
#include "fg_streams.hpp"
#include "fg_window.hpp"

namespace fg {

using namespace window;

namespace {

// The wave's Acc from its lanes'; every lane of the wave takes part.  The low energy words are
// summed as two 32-bit halves (64 of them stay below 2^38), so no carry is lost.
__device__ __forceinline__ levels::Acc wave_acc(const levels::Acc &a) {
    levels::Acc r;
    const uint64_t s0 = wave_sum64(a.e_lo & 0xFFFFFFFFull), s1 = wave_sum64(a.e_lo >> 32);
    r.e_lo = s0 + (s1 << 32);
    r.e_hi = wave_sum64(a.e_hi) + (s1 >> 32) + (r.e_lo < s0 ? 1u : 0u);
    r.sum = (int64_t)wave_sum64((uint64_t)a.sum);
    r.peak = wave_max32(a.peak);
    r.pad = 0;
    return r;
}

struct Out {
    uint32_t *peak;
    int64_t *sum;
    double *energy;
};

__device__ __forceinline__ void store_levels(const Out &o, uint64_t at, const levels::Acc &a) {
    o.peak[at] = a.peak;
    o.sum[at] = a.sum;
    o.energy[at] = levels::acc_energy(a);
}

__device__ __forceinline__ uint32_t wave_index() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__global__ void __launch_bounds__(256) k_window_levels(const Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                                                        const uint64_t *src_base, const uint64_t *dst_off, const uint64_t *part_base,
                                                        levels::Acc *parts, Out out, levels::Plan pl, uint32_t C, uint32_t B) {
    __shared__ uint64_t s_src[deliver::kTileWords];
    __shared__ levels::Acc s_wave[4][deliver::kMixMaxChannels];
    const uint32_t w = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = wave_index();
    const Cover c = recs[w];
    if (c.status != WIN_OK || res[w].bad_frames != 0 || c.n_samples == 0) return;
    const uint64_t n = c.n_samples, at0 = dst_off[w];
    const uint32_t per = C * B, hop = pl.hop;
    const uint8_t *src = scratch + src_base[w] + c.skip * per;
    const uint64_t tiles = levels::n_tiles(n, pl);
    const uint32_t *words = (const uint32_t *)s_src;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const levels::Tile tl = levels::tile_at(n, pl, tile);
        uint64_t a0;
        uint32_t lead, n_words;
        levels::tile_words((uint64_t)(uintptr_t)(src + tl.t0 * per), tl.ns, per, a0, lead, n_words);  // n_words <= kTileWords
        for (uint32_t i = tid; i < n_words; i += 256u) s_src[i] = ((const uint64_t *)(uintptr_t)a0)[i];
        __syncthreads();
        if (pl.mode == levels::LV_PARTS) {
            for (uint32_t ch = 0; ch < C; ch++) {
                const levels::Acc a = wave_acc(levels::tile_acc(words, lead, per, B, ch, tid, tl.ns, 256u));
                if (lane == 0) s_wave[wv][ch] = a;
            }
            __syncthreads();
            if (tid < C) {
                levels::Acc a = s_wave[0][tid];
                for (uint32_t k = 1; k < 4u; k++) levels::acc_merge(a, s_wave[k][tid]);
                if (pl.parts == 1u) store_levels(out, at0 + tl.block0 * C + tid, a);
                else parts[part_base[w] + (tl.block0 * pl.parts + tl.part) * C + tid] = a;
            }
        } else {
            const uint32_t nb = (tl.ns + hop - 1u) / hop;  // the tile's blocks, the last one perhaps short
            if (pl.mode == levels::LV_WAVES) {
                for (uint32_t b = wv; b < nb; b += 4u) {  // uniform in the wave
                    const uint32_t first = b * hop, end = first + hop < tl.ns ? first + hop : tl.ns;
                    for (uint32_t ch = 0; ch < C; ch++) {
                        const levels::Acc a = wave_acc(levels::tile_acc(words, lead, per, B, ch, first + lane, end, levels::kWave));
                        if (lane == 0) store_levels(out, at0 + (tl.block0 + b) * C + ch, a);
                    }
                }
            } else {
                for (uint32_t item = tid; item < nb * C; item += 256u) {
                    const uint32_t b = item / C, ch = item - b * C;
                    const uint32_t first = b * hop, end = first + hop < tl.ns ? first + hop : tl.ns;
                    store_levels(out, at0 + (tl.block0 + b) * C + ch, levels::tile_acc(words, lead, per, B, ch, first, end, 1u));
                }
            }
        }
        __syncthreads();  // s_src and s_wave are written again by the next tile
    }
}

__global__ void __launch_bounds__(256) k_levels_fold(const Cover *recs, const streams::StreamResult *res, const uint64_t *dst_off,
                                                      const uint64_t *part_base, const levels::Acc *parts, Out out, levels::Plan pl,
                                                      uint32_t C) {
    const uint32_t w = blockIdx.y, lane = threadIdx.x & 63u, wv = wave_index();
    const Cover c = recs[w];
    if (c.status != WIN_OK || res[w].bad_frames != 0 || c.n_samples == 0) return;
    const uint64_t n = c.n_samples, items = levels::n_blocks(n, pl.hop) * C;
    const levels::Acc *mine = parts + part_base[w];
    for (uint64_t item = (uint64_t)blockIdx.x * 4u + wv; item < items; item += (uint64_t)gridDim.x * 4u) {  // uniform in the wave
        const uint64_t j = item / C, np = levels::parts_of(levels::block_len(n, pl.hop, j), pl.T);
        const uint32_t ch = (uint32_t)(item - j * C);
        levels::Acc a = levels::acc_zero();
        for (uint64_t p = lane; p < np; p += levels::kWave) levels::acc_merge(a, mine[(j * pl.parts + p) * C + ch]);
        a = wave_acc(a);
        if (lane == 0) store_levels(out, dst_off[w] + item, a);
    }
}

}  // namespace

// n <= 65535 (gridDim.y); max_samples: the most any clean window measures, which sizes the grids.
// parts: the Acc records of the windows whose blocks have several parts, window w's from
// part_base[w] on (levels::partial_records of them); unused where pl.parts = 1.
hipError_t launch_window_levels(const Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                                const uint64_t *src_base, const uint64_t *dst_off, const uint64_t *part_base, void *parts,
                                uint32_t *peak, int64_t *sum, double *energy, uint32_t hop, uint32_t C, uint32_t B, uint32_t n,
                                uint64_t max_samples, hipStream_t st) {
    if (n == 0 || max_samples == 0) return hipSuccess;
    const levels::Plan pl = levels::plan(hop, C * B);
    const Out out{peak, sum, energy};
    const uint64_t tiles = levels::n_tiles(max_samples, pl);
    const uint32_t gx = (uint32_t)(tiles > 1024u ? 1024u : tiles);
    hipLaunchKernelGGL(k_window_levels, dim3(gx, n), dim3(256), 0, st, recs, res, scratch, src_base, dst_off, part_base,
                       (levels::Acc *)parts, out, pl, C, B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || pl.parts == 1u) return e;
    const uint64_t groups = (levels::n_blocks(max_samples, hop) * C + 3u) / 4u;
    hipLaunchKernelGGL(k_levels_fold, dim3((uint32_t)(groups > 1024u ? 1024u : groups), n), dim3(256), 0, st, recs, res, dst_off,
                       part_base, (const levels::Acc *)parts, out, pl, C);
    return hipGetLastError();
}

}  // namespace fg
