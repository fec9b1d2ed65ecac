// fg_window.hip -- the kernels of the sample-window decode (gfx950); the rules are fg_window.hpp's.
//
//   k_pos_blocks      per table entry of every stream: the frame's block size, from at most 16
//                     bytes of its header, into the stream's slice of the position table
//   k_pos_scan        per stream, one workgroup: the exclusive sum of those block sizes in place,
//                     256 frames an iteration with a carried total; the total to d_stream_samples
//   k_window_cover    per window: binary search of its stream's positions -> a Cover record
//   k_window_init     per window: its scratch StreamResult and carried sample count, for the
//                     chunk loop in which a window is what a stream is in fg_dec_streams.hip
//   k_window_copy     per window (blockIdx.y), after the last chunk: the delivered bytes from the
//                     window's decoded covering frames to the caller's region
//   k_window_elements in place of k_window_copy, one kernel in three instantiations.  <MIX_NONE>, for
//                     flacgpu_decode_windows_device_as: the delivered samples converted to tensor
//                     elements (fg_deliver.hpp), interleaved or planar, the rest of a padded window
//                     zeroed.  <MIX_MASKS>, for flacgpu_decode_windows_device_mix: the same pass with a
//                     channel count other than the source's, every output channel the exact mean
//                     of a set of source channels, one of them, or silence.  <MIX_WEIGHTS>, for
//                     flacgpu_decode_windows_device_to with a weight matrix: every output channel
//                     the fused multiply-add chain of deliver::mixw_value over all source channels.
//                     All write rows by deliver::fill_row_slot, which the host programs of the tests
//                     run as well
//   k_window_results  per window: its flacgpu_window_result
//
// Every index is bounded by what the index left and the host sized: a frame i of stream s is
// touched only where i < n_frames <= table_caps[s] of an OK index result; a window w < n_windows.
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_deliver.hpp"
#include "fg_index.hpp"
#include "fg_levels.hpp"
#include "fg_streams.hpp"
#include "fg_window.hpp"

namespace fg {

using namespace window;

namespace {

// the frames of stream s that have positions: those of an OK index that fit the stream's slice
__device__ __forceinline__ uint64_t pos_frames(const idx::IndexResult *ires, const PosStream &ps, uint32_t s) {
    const idx::IndexResult r = ires[s];
    return (r.status == idx::IDX_OK && r.n_frames <= ps.table_cap) ? r.n_frames : 0ull;
}

__global__ void __launch_bounds__(256) k_pos_blocks(const uint8_t *data, const PosStream *streams, const uint64_t *f_off,
                                                     const uint32_t *f_bytes, const idx::IndexResult *ires, uint64_t *pos) {
    const uint32_t s = blockIdx.y;
    const PosStream ps = streams[s];
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= pos_frames(ires, ps, s)) return;
    const uint64_t e = ps.table_first + i;
    pos[e] = block_at(data + f_off[e], f_bytes[e], ps.bits, ps.rate);
}

__global__ void __launch_bounds__(256) k_pos_scan(const PosStream *streams, const idx::IndexResult *ires, uint64_t *pos,
                                                   uint64_t *totals) {
    __shared__ uint64_t s_wave[4];
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const PosStream ps = streams[s];
    const uint64_t n = pos_frames(ires, ps, s);
    uint64_t *p = pos + ps.table_first;
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 256u) {
        const uint64_t i = i0 + tid;
        const uint64_t x = i < n ? p[i] : 0ull;
        uint64_t inc = x;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t y = __shfl_up((unsigned long long)inc, d, 64);
            if (lane >= d) inc += y;
        }
        if (lane == 63u) s_wave[wv] = inc;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint64_t t = s_wave[k];
            if (k < wv) before += t;
            all += t;
        }
        if (i < n) p[i] = carry + before + (inc - x);
        carry += all;
        __syncthreads();  // s_wave is written again by the next iteration
    }
    if (tid == 0) totals[s] = carry;
}

__global__ void __launch_bounds__(256) k_window_cover(const WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos,
                                                       const uint64_t *totals, uint32_t unit, uint32_t flags, uint32_t hop,
                                                       Cover *recs, uint32_t n) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    const WindowArg a = args[w];
    const idx::IndexResult r = ires[a.stream];
    Cover c;
    if (r.status != idx::IDX_OK) {
        c = cover(nullptr, 0, 0, a.start, a.count);
        c.status = WIN_BAD_INDEX;
    } else {
        c = cover(pos + a.table_first, r.n_frames, totals[a.stream], a.start, a.count);
        // the byte copy: unit = per, no flags, so n_samples * per > cap with no product to overflow
        // the levels (hop != 0): unit = the channels, the capacity in records of a block and channel
        if (hop ? levels::too_small(c.n_samples, hop, unit, a.cap) : deliver::too_small(c.n_samples, a.count, flags, a.cap, unit))
            c.status = WIN_TOO_SMALL;
    }
    recs[w] = c;
}

__global__ void __launch_bounds__(256) k_window_init(const Cover *recs, streams::StreamResult *res, uint64_t *carried,
                                                      uint32_t n) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    const Cover c = recs[w];
    streams::StreamResult r;
    r.n_frames = c.status == WIN_OK ? c.n_frames : 0u;
    r.n_samples = 0;
    r.index_status = idx::IDX_OK;
    r.bad_frames = 0;
    r.first_bad_frame = streams::kNone;
    r.first_bad_status = 0;
    res[w] = r;
    carried[w] = 0;
}

__device__ __forceinline__ bool window_clean(const Cover &c, const streams::StreamResult &r) {
    return c.status == WIN_OK && r.bad_frames == 0;
}

// src_base[w]: the window's covering frames in the scratch (16-byte aligned, the scratch readable
// up to the next 8-byte boundary past every region); dst_off[w]: the caller's region in out.
__global__ void __launch_bounds__(256) k_window_copy(const Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                                                      const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off,
                                                      uint32_t per) {
    const uint32_t w = blockIdx.y;
    const Cover c = recs[w];
    if (!window_clean(c, res[w]) || c.n_samples == 0) return;
    const uint8_t *src = scratch + src_base[w] + c.skip * per;
    uint8_t *dst = out + dst_off[w];
    const uint64_t nb = c.n_samples * per;
    const CopyPlan p = copy_plan((uint64_t)(uintptr_t)dst, nb);
    if (blockIdx.x == 0) {
        const uint32_t t = threadIdx.x;
        if (t < p.head) dst[t] = src[t];
        else if (t >= 16u && t - 16u < p.tail) {
            const uint64_t at = p.head + 16u * p.units + (t - 16u);
            dst[at] = src[at];
        }
    }
    for (uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x; u < p.units; u += (uint64_t)gridDim.x * 256u) {
        uint64_t q0, q1;
        load_unit(src + p.head + 16u * u, q0, q1);
        *(uint4 *)(dst + p.head + 16u * u) = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
    }
}

// One element of a tile: source element si of the tile's `have` (sample-major, channel-minor, as
// they lie in the LDS words from byte `lead` on), or zero past them (the padding).
__device__ __forceinline__ uint32_t tile_element(const uint32_t *words, uint32_t lead, uint32_t si, uint32_t have,
                                                 const deliver::Delivery &dv) {
    if (si >= have) return 0u;
    return deliver::element(deliver::sample_in_words(words, lead + si * dv.sample_bytes, dv.sample_bytes), 8u * dv.sample_bytes,
                            dv.format);
}

// One element of a mixed tile: output channel `mask` of the tile's sample t, or zero past its
// `nsrc` decoded samples (the padding).
__device__ __forceinline__ uint32_t mix_tile_element(const uint32_t *words, uint32_t lead, uint32_t t, uint32_t nsrc, uint32_t per,
                                                     uint32_t mask, const deliver::Delivery &dv) {
    if (t >= nsrc) return 0u;
    return deliver::mix_element(words, lead + t * per, dv.sample_bytes, mask, dv.format);
}

// One element of a weighted tile: the chain of deliver::mixw_value over row w of the weights for the
// tile's sample t, or zero past its `nsrc` decoded samples (the padding).
__device__ __forceinline__ uint32_t mixw_tile_element(const uint32_t *words, uint32_t lead, uint32_t t, uint32_t nsrc, uint32_t per,
                                                      const float *w, const deliver::Delivery &dv) {
    if (t >= nsrc) return 0u;
    return deliver::mixw_element(words, lead + t * per, dv.sample_bytes, dv.channels, w, dv.format);
}

// In place of k_window_copy: window w (blockIdx.y) as K channels of dv.format elements to out +
// dst_off[w] elements; K = dv.channels, or with a Mix dv.out_channels, output channel k of a sample
// then made of the source channels in dv.masks[k] (MIX_MASKS: deliver::mix_element) or of all of
// them under row k of dv.weights (MIX_WEIGHTS: deliver::mixw_element; the K * C <= 64 weights go
// from device memory to LDS once a workgroup, before the first tile, and are indexed there: a
// by-value argument indexed dynamically would be forced into scratch).  A workgroup takes tiles
// of tile_samples(per) consecutive source samples: the aligned 8-byte words of the scratch that
// hold a tile's source bytes go to LDS (no word past the one that holds the window's last byte is
// read; a tile of padding alone reads nothing), then every row of the tile -- a plane's part, or
// the interleaved tile of samples * K elements -- is written slot by slot, one thread a slot
// (deliver::fill_row_slot): whole 16-byte units built from LDS, the head and the tail elements one
// at a time.  A window that is not clean writes nothing; one with no samples still writes its
// padding.
template <uint32_t Mix>
__global__ void __launch_bounds__(256) k_window_elements(const Cover *recs, const streams::StreamResult *res, const WindowArg *args,
                                                          const uint8_t *scratch, const uint64_t *src_base, uint8_t *out,
                                                          const uint64_t *dst_off, deliver::Delivery dv) {
    __shared__ uint64_t s_src[deliver::kTileWords];
    const uint32_t w = blockIdx.y, tid = threadIdx.x;
    const Cover c = recs[w];
    if (!window_clean(c, res[w])) return;
    const uint64_t count = args[w].count, n = c.n_samples;
    const uint64_t total = deliver::written_samples(n, count, dv.flags);
    if (total == 0) return;
    const uint32_t C = dv.channels, K = Mix != deliver::MIX_NONE ? dv.out_channels : C, per = C * dv.sample_bytes;
    const uint32_t esz = deliver::elem_size(dv.format), per_unit = 16u / esz, T = deliver::tile_samples(per);
    const bool planar = (dv.flags & deliver::DELIVER_PLANAR) != 0;
    uint64_t masks = 0;  // mask k in byte k: indexed by shifts, so that the argument is never addressed
    if (Mix == deliver::MIX_MASKS) {
#pragma unroll
        for (uint32_t k = 0; k < deliver::kMixMaxChannels; k++) masks |= (uint64_t)dv.masks[k] << (8u * k);
    }
    __shared__ float s_w[deliver::kMixMaxChannels * deliver::kMixMaxChannels];
    if (Mix == deliver::MIX_WEIGHTS) {  // read after the first tile's barrier
        if (tid < K * C) s_w[tid] = dv.weights[tid];
    }
    const uint8_t *src = scratch + src_base[w] + c.skip * per;
    uint8_t *dst = out + dst_off[w] * esz;
    const uint64_t n_tiles = (total + T - 1u) / T;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * T;
        const uint32_t ns = (uint32_t)(total - t0 < T ? total - t0 : T);          // samples written
        const uint32_t nsrc = t0 < n ? (uint32_t)(n - t0 < T ? n - t0 : T) : 0u;  // of them decoded ones
        uint32_t lead = 0;
        if (nsrc) {
            const uintptr_t a = (uintptr_t)(src + t0 * per), a0 = a & ~(uintptr_t)7;
            lead = (uint32_t)(a - a0);
            const uint32_t n_words = (lead + nsrc * per + 7u) / 8u;  // <= kTileWords
            for (uint32_t i = tid; i < n_words; i += 256u) s_src[i] = ((const uint64_t *)a0)[i];
        }
        __syncthreads();
        const uint32_t *words = (const uint32_t *)s_src;
        const uint32_t rows = planar ? K : 1u, row_elems = planar ? ns : ns * K;
        const uint32_t max_units = row_elems / per_unit, slots = max_units + 2u;  // a row's units, its head, its tail
        for (uint32_t item = tid; item < rows * slots; item += 256u) {
            const uint32_t r = item / slots, k = item - r * slots;
            uint8_t *row = dst + (planar ? (uint64_t)r * count + t0 : t0 * K) * esz;
            if (Mix == deliver::MIX_WEIGHTS) {
                deliver::fill_row_slot(row, row_elems, esz, k, max_units, [&](uint32_t e) {
                    const uint32_t t = planar ? e : e / K, ch = planar ? r : e - t * K;
                    return mixw_tile_element(words, lead, t, nsrc, per, s_w + ch * C, dv);
                });
            } else if (Mix == deliver::MIX_MASKS) {
                // row element e: sample e of plane r, or sample e / K, channel e % K of the interleaved row
                deliver::fill_row_slot(row, row_elems, esz, k, max_units, [&](uint32_t e) {
                    const uint32_t t = planar ? e : e / K, ch = planar ? r : e - t * K;
                    return mix_tile_element(words, lead, t, nsrc, per, (uint32_t)(masks >> (8u * ch)) & 0xFFu, dv);
                });
            } else {
                const uint32_t mul = planar ? C : 1u, add = planar ? r : 0u;  // row element e is source element e * mul + add
                deliver::fill_row_slot(row, row_elems, esz, k, max_units,
                                       [&](uint32_t e) { return tile_element(words, lead, e * mul + add, nsrc * C, dv); });
            }
        }
        __syncthreads();  // s_src is written again by the next tile
    }
}

__global__ void __launch_bounds__(256) k_window_results(const Cover *recs, const streams::StreamResult *res, WindowResult *out,
                                                         uint32_t n) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= n) return;
    const Cover c = recs[w];
    const streams::StreamResult r = res[w];
    WindowResult o;
    o.n_samples = window_clean(c, r) ? c.n_samples : 0ull;
    o.first_frame = c.first_frame;
    o.n_frames = c.status == WIN_OK ? c.n_frames : 0u;
    o.status = c.status;
    o.first_bad_frame = streams::kNone;
    o.first_bad_status = 0;
    if (c.status == WIN_OK && r.bad_frames != 0) {
        o.status = WIN_BAD_FRAME;
        o.first_bad_frame = (uint32_t)c.first_frame + r.first_bad_frame;  // counted in its stream
        o.first_bad_status = r.first_bad_status;
    }
    out[w] = o;
}

}  // namespace

// n_streams <= 65535 (gridDim.y); max_cap: the largest table_caps[] of the call
hipError_t launch_positions(const uint8_t *data, const PosStream *d_streams, uint32_t n_streams, uint64_t max_cap,
                            const uint64_t *f_off, const uint32_t *f_bytes, const idx::IndexResult *ires, uint64_t *pos,
                            uint64_t *totals, hipStream_t st) {
    if (n_streams == 0) return hipSuccess;
    if (max_cap) {
        const uint64_t gx = (max_cap + 255u) / 256u;
        if (gx > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_pos_blocks, dim3((uint32_t)gx, n_streams), dim3(256), 0, st, data, d_streams, f_off, f_bytes, ires,
                           pos);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_pos_scan, dim3(n_streams), dim3(256), 0, st, d_streams, ires, pos, totals);
    return hipGetLastError();
}

// unit, flags: the capacity rule's (deliver::too_small); the byte copy passes per and 0.  hop != 0:
// the capacity rule of the levels (levels::too_small) with unit = the channels
hipError_t launch_window_cover(const WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos, const uint64_t *totals,
                               uint32_t unit, uint32_t flags, uint32_t hop, Cover *recs, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_window_cover, dim3((n + 255u) / 256u), dim3(256), 0, st, args, ires, pos, totals, unit, flags, hop,
                       recs, n);
    return hipGetLastError();
}

hipError_t launch_window_init(const Cover *recs, streams::StreamResult *res, uint64_t *carried, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_window_init, dim3((n + 255u) / 256u), dim3(256), 0, st, recs, res, carried, n);
    return hipGetLastError();
}

// n <= 65535 (gridDim.y); max_bytes: the most any window delivers, which sizes gridDim.x
hipError_t launch_window_copy(const Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                              const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off, uint32_t per, uint32_t n,
                              uint64_t max_bytes, hipStream_t st) {
    if (n == 0 || max_bytes == 0) return hipSuccess;
    const uint64_t blocks = (max_bytes / 16u + 255u) / 256u;
    const uint32_t gx = (uint32_t)(blocks < 1u ? 1u : (blocks > 256u ? 256u : blocks));
    hipLaunchKernelGGL(k_window_copy, dim3(gx, n), dim3(256), 0, st, recs, res, scratch, src_base, out, dst_off, per);
    return hipGetLastError();
}

// n <= 65535 (gridDim.y); max_samples: the most any window writes, padding included, which sizes
// gridDim.x: the tiles are of source samples with a mix or without
hipError_t launch_window_elements(const Cover *recs, const streams::StreamResult *res, const WindowArg *args,
                                  const uint8_t *scratch, const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off,
                                  const deliver::Delivery &dv, uint32_t n, uint64_t max_samples, hipStream_t st) {
    if (n == 0 || max_samples == 0) return hipSuccess;
    const uint32_t T = deliver::tile_samples(dv.channels * dv.sample_bytes);
    const uint64_t tiles = (max_samples + T - 1u) / T;
    const uint32_t gx = (uint32_t)(tiles > 1024u ? 1024u : tiles);
    const auto kernel = dv.mix == deliver::MIX_WEIGHTS ? k_window_elements<deliver::MIX_WEIGHTS>
                        : dv.mix                       ? k_window_elements<deliver::MIX_MASKS>
                                                       : k_window_elements<deliver::MIX_NONE>;
    hipLaunchKernelGGL(kernel, dim3(gx, n), dim3(256), 0, st, recs, res, args, scratch, src_base, out, dst_off, dv);
    return hipGetLastError();
}

hipError_t launch_window_results(const Cover *recs, const streams::StreamResult *res, WindowResult *out, uint32_t n,
                                 hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_window_results, dim3((n + 255u) / 256u), dim3(256), 0, st, recs, res, out, n);
    return hipGetLastError();
}

}  // namespace fg
