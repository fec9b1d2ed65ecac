// fg_resample.hip -- the kernels of the resampled delivery of sample windows (gfx950); the rules
// are fg_resample.hpp's, the rows fg_deliver.hpp's, the records fg_window.hpp's.
//
//   k_resample_cover   per window, in place of k_window_cover: the window is stated in OUTPUT
//                      samples; its delivered count n and the source samples [lo, hi) the filter
//                      needs for them come from the stream's total, and the Cover record is the cover
//                      of [lo, hi) with n_samples = n: the chunk loop, k_window_init and
//                      k_window_results then run as for every other window call
//   k_window_resample  in place of k_window_elements, one kernel in three instantiations (the modes of
//                      deliver::Delivery::mix: none, channel masks, a weight matrix).  A workgroup takes tiles of output samples: a tile's source
//                      span, halo included, goes from the window's decoded covering frames to LDS as
//                      F32 elements, one skewed plane an output channel (the mix applied once a
//                      source sample, zeros where the span leaves the stream), then every row of the
//                      tile is written slot by slot by deliver::fill_row_slot, an element the FIR of
//                      resample::fir over LDS and the T coefficients of its phase
//
// Every index is bounded as in fg_window.hip; a source sample is read only inside [lo, hi), which
// the covering frames hold, and an LDS plane holds the tile's whole span (resample::tile_plan).
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_deliver.hpp"
#include "fg_index.hpp"
#include "fg_resample.hpp"
#include "fg_streams.hpp"
#include "fg_window.hpp"

namespace fg {

using namespace window;

namespace {

__global__ void __launch_bounds__(256) k_resample_cover(const WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos,
                                                         const uint64_t *totals, resample::Ratio rt, uint32_t unit, uint32_t flags,
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
        const uint64_t total = totals[a.stream];
        if (total > (1ull << 40)) {  // no stream's positions: the whole span, which the host refuses
            c = cover(pos + a.table_first, r.n_frames, total, 0, total);
        } else {
            uint64_t nout = resample::delivered(resample::out_total(rt, total), a.start, a.count), lo, hi;
            resample::source_range(rt, total, a.start, nout, &lo, &hi);
            c = cover(pos + a.table_first, r.n_frames, total, lo, hi - lo);
            if (c.n_samples != hi - lo) {  // a table that does not cover its own total
                c = cover(nullptr, 0, 0, 0, 0);
                nout = 0;
            }
            c.n_samples = nout;
            if (deliver::too_small(nout, a.count, flags, a.cap, unit)) c.status = WIN_TOO_SMALL;
        }
    }
    recs[w] = c;
}

// Window w (blockIdx.y) of the resampled delivery: n = recs[w].n_samples output samples from
// args[w].start on, as K channels of dv.format elements to out + dst_off[w] elements, laid out and
// padded as k_window_elements does.  src_base[w] + skip * per is source sample lo of the window's
// source range [lo, hi) in the scratch.  tile, plane: resample::tile_plan's for (rt, K); the
// dynamic LDS is K planes.  coeffs: the table of rt, L rows of T.
template <uint32_t Mix>
__global__ void __launch_bounds__(256) k_window_resample(const Cover *recs, const streams::StreamResult *res, const WindowArg *args,
                                                          const uint64_t *totals, const uint8_t *scratch, const uint64_t *src_base,
                                                          uint8_t *out, const uint64_t *dst_off, deliver::Delivery dv,
                                                          resample::Ratio rt, uint32_t tile_n, uint32_t plane, const float *coeffs) {
    extern __shared__ float s_x[];
    const uint32_t w = blockIdx.y, tid = threadIdx.x;
    const Cover c = recs[w];
    if (c.status != WIN_OK || res[w].bad_frames != 0) return;
    const WindowArg a = args[w];
    const uint64_t count = a.count, n = c.n_samples;
    const uint64_t written = deliver::written_samples(n, count, dv.flags);
    if (written == 0) return;
    const uint32_t C = dv.channels, K = Mix != deliver::MIX_NONE ? dv.out_channels : C, B = dv.sample_bytes, per = C * B;
    const uint32_t format = dv.format, esz = deliver::elem_size(format), per_unit = 16u / esz, T = rt.T;
    const bool planar = (dv.flags & deliver::DELIVER_PLANAR) != 0;
    uint64_t masks = 0;  // mask k in byte k: indexed by shifts, so that the argument is never addressed
    if (Mix == deliver::MIX_MASKS) {
#pragma unroll
        for (uint32_t k = 0; k < deliver::kMixMaxChannels; k++) masks |= (uint64_t)dv.masks[k] << (8u * k);
    }
    uint64_t lo, hi;
    resample::source_range(rt, totals[a.stream], a.start, n, &lo, &hi);
    const uint8_t *src = scratch + src_base[w] + c.skip * per;  // source sample lo
    uint8_t *dst = out + dst_off[w] * esz;
    const uint64_t n_tiles = (written + tile_n - 1u) / tile_n;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * tile_n;
        const uint32_t ns = (uint32_t)(written - t0 < tile_n ? written - t0 : tile_n);      // samples written
        const uint32_t nfir = t0 < n ? (uint32_t)(n - t0 < tile_n ? n - t0 : tile_n) : 0u;  // of them filtered ones
        uint64_t first = 0;  // the source index of the tile's first output sample: tap 0 of it is LDS element 0
        if (nfir) {
            first = resample::source_index(rt, a.start + t0, nullptr);
            const uint64_t last = resample::source_index(rt, a.start + t0 + nfir - 1u, nullptr);
            const uint32_t len = (uint32_t)(last - first) + T;  // <= tile_span(rt, tile_n)
            const int64_t s0 = (int64_t)first - (int64_t)rt.Hw + 1;
            if (Mix == deliver::MIX_WEIGHTS) {
                // a plane at a time: row ch of the weights in registers (a uniform read of device memory
                // under constant indices, no argument or array is addressed), then the chain of
                // deliver::mixw_step once a source sample
                for (uint32_t ch = 0; ch < K; ch++) {
                    float wr[deliver::kMixMaxChannels];
#pragma unroll
                    for (uint32_t cc = 0; cc < deliver::kMixMaxChannels; cc++) wr[cc] = cc < C ? dv.weights[ch * C + cc] : 0.0f;
                    for (uint32_t j = tid; j < len; j += 256u) {
                        const int64_t i = s0 + (int64_t)j;
                        float y = 0.0f;  // +0.0f outside the stream
                        if (i >= (int64_t)lo && i < (int64_t)hi) {
                            const uintptr_t at = (uintptr_t)(src + (uint64_t)(i - (int64_t)lo) * per), at0 = at & ~(uintptr_t)3;
                            const uint32_t *words = (const uint32_t *)at0;
                            const uint32_t off = (uint32_t)(at - at0);
#pragma unroll
                            for (uint32_t cc = 0; cc < deliver::kMixMaxChannels; cc++)
                                if (cc < C && wr[cc] != 0.0f)
                                    y = deliver::mixw_step(y, wr[cc], deliver::sample_in_words(words, off + cc * B, B), 8u * B);
                        }
                        s_x[ch * plane + resample::skew(j)] = y;
                    }
                }
            } else {
                for (uint32_t item = tid; item < len * K; item += 256u) {
                    const uint32_t ch = item / len, j = item - ch * len;
                    const int64_t i = s0 + (int64_t)j;
                    uint32_t v = 0u;  // +0.0f outside the stream
                    if (i >= (int64_t)lo && i < (int64_t)hi) {
                        const uintptr_t at = (uintptr_t)(src + (uint64_t)(i - (int64_t)lo) * per), at0 = at & ~(uintptr_t)3;
                        const uint32_t *words = (const uint32_t *)at0;
                        const uint32_t off = (uint32_t)(at - at0);
                        if (Mix == deliver::MIX_MASKS)
                            v = deliver::mix_element(words, off, B, (uint32_t)(masks >> (8u * ch)) & 0xFFu, deliver::SAMPLE_F32);
                        else
                            v =deliver::f32_bits(deliver::sample_in_words(words, off + ch * B, B), 8u * B);
                    }
                    s_x[ch * plane + resample::skew(j)] = __uint_as_float(v);
                }
            }
        }
        __syncthreads();
        const uint32_t rows = planar ? K : 1u, row_elems = planar ? ns : ns * K;
        const uint32_t max_units = row_elems / per_unit, slots = max_units + 2u;  // a row's units, its head, its tail
        for (uint32_t item = tid; item < rows * slots; item += 256u) {
            const uint32_t r = item / slots, k = item - r * slots;
            uint8_t *row = dst + (planar ? (uint64_t)r * count + t0 : t0 * K) * esz;
            // row element e: sample e of plane r, or sample e / K, channel e % K of the interleaved row
            deliver::fill_row_slot(row, row_elems, esz, k, max_units, [&](uint32_t e) {
                const uint32_t t = planar ? e : e / K, ch = planar ? r : e - t * K;
                if (t >= nfir) return 0u;  // the padding
                uint32_t p;
                const uint32_t base = (uint32_t)(resample::source_index(rt, a.start + t0 + t, &p) - first);
                const float *x = s_x + ch * plane;
                const float y = resample::fir(coeffs + (uint64_t)p * T, T, [&](uint32_t tap) { return x[resample::skew(base + tap)]; });
                const uint32_t f = __float_as_uint(y);
                if (Mix == deliver::MIX_WEIGHTS) return deliver::mixw_narrow(y, format);  // |y| can pass the f16 range
                if (format == deliver::SAMPLE_F32) return f;
                return (uint32_t)(format == deliver::SAMPLE_F16 ? deliver::f16_bits(f) : deliver::bf16_bits(f));
            });
        }
        __syncthreads();  // s_x is written again by the next tile
    }
}

}  // namespace

// in place of launch_window_cover; unit: the output channels K
hipError_t launch_resample_cover(const WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos, const uint64_t *totals,
                                 const resample::Ratio &rt, uint32_t unit, uint32_t flags, Cover *recs, uint32_t n,
                                 hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_resample_cover, dim3((n + 255u) / 256u), dim3(256), 0, st, args, ires, pos, totals, rt, unit, flags, recs,
                       n);
    return hipGetLastError();
}

// n <= 65535 (gridDim.y); max_samples: the most output samples any window writes, padding
// included, which sizes gridDim.x; coeffs: the device table of rt
hipError_t launch_window_resample(const Cover *recs, const streams::StreamResult *res, const WindowArg *args, const uint64_t *totals,
                                  const uint8_t *scratch, const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off,
                                  const deliver::Delivery &dv, const resample::Ratio &rt, const float *coeffs, uint32_t n,
                                  uint64_t max_samples, hipStream_t st) {
    if (n == 0 || max_samples == 0) return hipSuccess;
    const resample::TilePlan tp = resample::tile_plan(rt, dv.out_channels);
    const uint64_t tiles = (max_samples + tp.tile - 1u) / tp.tile;
    const uint32_t gx = (uint32_t)(tiles > 1024u ? 1024u : tiles);
    const auto kernel = dv.mix == deliver::MIX_WEIGHTS ? k_window_resample<deliver::MIX_WEIGHTS>
                        : dv.mix                       ? k_window_resample<deliver::MIX_MASKS>
                                                       : k_window_resample<deliver::MIX_NONE>;
    hipLaunchKernelGGL(kernel, dim3(gx, n), dim3(256), tp.lds_bytes, st, recs, res, args, totals, scratch, src_base, out, dst_off,
                       dv, rt, tp.tile, tp.plane, coeffs);
    return hipGetLastError();
}

}  // namespace fg
