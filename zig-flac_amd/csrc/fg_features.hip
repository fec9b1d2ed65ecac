// fg_features.hip -- the kernel of the feature delivery of sample windows (gfx950); the rules are
// fg_features.hpp's, the narrowing fg_deliver.hpp's, the results fg_window.hpp's.
//
//   k_features   stage 2 of flacgpu_decode_windows_device_features.  Stage 1 (the window delivery
//                itself, planar F32 with padding) has left every window's extended span in the
//                context's scratch, one plane a channel, and its results.  A workgroup (blockIdx.y:
//                the window) takes tiles of frames of one channel: the tile's span goes to LDS, the
//                DFT is the product [frames x N] . [N x 2B] on v_mfma_f32_16x16x4_f32 with the taps
//                fed in ascending n, the filter bank the product [frames x B] . [B x R] fed in
//                ascending b over the powers in LDS.
//
// The f32-input MFMA adds its four products to the accumulator one after the other, k ascending,
// each a correctly rounded fused multiply-add: an accumulator element is the chain of the rule, bit
// for bit.  A wave's two accumulators of a tile -- the cos and the sin column of the same 16 bins
// -- are independent, which covers the instruction's dependent latency.  Operands the tile does not
// have (frames short of 16, bins or rows short of 16, taps past N) are zero: fmaf(0, v, acc) = acc.
//
// Operand tables are laid out for the instruction: block (column tile ct, k block kb) is 64 lanes
// of 4 floats, lane l's float s the entry of column ct * 16 + (l & 15) at k = kb * 16 + 4 s + (l >> 4),
// so one 16-byte load a lane feeds four instructions and a wave's load is 1 KiB contiguous.
//
// Every index is bounded: a sample is read at plane offsets below `count`, which stage 1 wrote
// (its padding included); an element is written at (k * rows + r) * frames + t < K * rows * frames
// of the window's region, which the host checked against its capacity; LDS by feat_geometry.
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_deliver.hpp"
#include "fg_features.hpp"
#include "fg_resample.hpp"
#include "fg_streams.hpp"
#include "fg_window.hpp"

namespace fg {

using namespace window;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void emit(uint8_t *out, uint64_t e, uint32_t format, float v) {
    const uint32_t f = feat::element(v, format);
    if (format == deliver::SAMPLE_F32) ((uint32_t *)out)[e] = f;
    else ((uint16_t *)out)[e] = (uint16_t)f;
}

// MT: accumulator tiles of 16 frames a wave holds (2 for a tile of 32 frames, else 1)
template <uint32_t MT>
__global__ void __launch_bounds__(256) k_features(const FeatWindow *wins, const WindowResult *stage1, const uint64_t *totals,
                                                   resample::Ratio rt, const float *x, const float *table, const float *filters,
                                                   uint8_t *out, WindowResult *results, feat::Params ft, FeatGeometry g, uint32_t K,
                                                   uint32_t format) {
    extern __shared__ float s_mem[];
    float *s_x = s_mem, *s_p = s_mem + g.plane;
    const uint32_t w = blockIdx.y, tid = threadIdx.x;
    const FeatWindow a = wins[w];
    WindowResult r1 = stage1[w];
    const bool ok = r1.status == WIN_OK && !a.too_small;
    if (blockIdx.x == 0 && tid == 0) {
        uint64_t total = totals[a.stream];
        if (rt.L) total = resample::out_total(rt, total);
        r1.n_samples = ok ? feat::delivered(ft, total, a.start, a.frames) : 0ull;
        if (a.too_small) r1.status = WIN_TOO_SMALL;
        results[w] = r1;
    }
    if (!ok || a.frames == 0) return;
    const uint32_t N = ft.n_fft, H = ft.hop, B = feat::bins(ft), R = ft.n_rows, n_rows = feat::rows(ft);
    const uint32_t TF = g.frames, frames = a.frames;
    const uint32_t wave = tid >> 6, lane = tid & 63u, li = lane & 15u, lk = lane >> 4;
    const uint32_t nkb = (N + 15u) / 16u, nbt = g.bins_pad / 16u, nrt = (R + 15u) / 16u;
    const uint32_t tiles = (frames + TF - 1u) / TF;
    const uint64_t items = (uint64_t)K * tiles;
    uint8_t *dst = out + a.out_off * deliver::elem_size(format);
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t k = (uint32_t)(item / tiles), t0 = (uint32_t)(item - (uint64_t)k * tiles) * TF;
        const uint32_t nf = frames - t0 < TF ? frames - t0 : TF;
        const uint32_t len = (nf - 1u) * H + N;  // <= g.span
        const float *xp = x + a.x_off + (uint64_t)k * a.count;
        const uint64_t e0 = (uint64_t)t0 * H;  // of the window's span
        for (uint32_t j = tid; j < len; j += 256u) {
            const uint64_t e = e0 + j;  // < span(frames) = clip + count
            s_x[resample::skew(j)] = e >= a.clip ? xp[e - a.clip] : 0.0f;
        }
        __syncthreads();
        const uint64_t row0 = (uint64_t)k * n_rows;
        // ---- the DFT: columns bt * 16 + li of the cos and of the sin plane --------------------------
        for (uint32_t bt = wave; bt < nbt; bt += 4u) {
            f32x4 re[MT], im[MT];
#pragma unroll
            for (uint32_t m = 0; m < MT; m++) re[m] = im[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const f32x4 *tb = (const f32x4 *)table + ((uint64_t)bt * nkb * 2u) * 64u + lane;
            for (uint32_t kb = 0; kb < nkb; kb++) {
                const f32x4 tc = tb[(uint64_t)kb * 128u], ts = tb[(uint64_t)kb * 128u + 64u];
#pragma unroll
                for (uint32_t s = 0; s < 4u; s++) {
                    const uint32_t n = kb * 16u + 4u * s + lk;
#pragma unroll
                    for (uint32_t m = 0; m < MT; m++) {
                        const uint32_t f = m * 16u + li;
                        const bool have = f < nf && n < N;
                        const float xv = s_x[resample::skew(have ? f * H + n : 0u)];
                        const float av = have ? xv : 0.0f;
                        re[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, tc[s], re[m], 0, 0, 0);
                        im[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ts[s], im[m], 0, 0, 0);
                    }
                }
            }
            // accumulator register q of lane l: frame (l >> 4) * 4 + q, column l & 15
            const uint32_t b = bt * 16u + li;
#pragma unroll
            for (uint32_t m = 0; m < MT; m++)
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) {
                    const uint32_t f = m * 16u + lk * 4u + q;
                    const float P = feat::power(re[m][q], im[m][q]);
                    if (R) {
                        if (f < TF) s_p[b * g.p_stride + f] = P;  // columns past B: the table's zeros, P = +0.0f
                    } else if (f < nf && b < B) {
                        emit(dst, (row0 + b) * frames + t0 + f, format, P);
                    }
                }
        }
        if (R) {
            __syncthreads();
            // ---- the filter bank: rows rt_ * 16 + li over the powers, every entry of F, b ascending --
            for (uint32_t rt_ = wave; rt_ < nrt; rt_ += 4u) {
                f32x4 acc[MT];
#pragma unroll
                for (uint32_t m = 0; m < MT; m++) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                const f32x4 *fb = (const f32x4 *)filters + ((uint64_t)rt_ * nbt) * 64u + lane;
                for (uint32_t bb = 0; bb < nbt; bb++) {
                    const f32x4 fv = fb[(uint64_t)bb * 64u];
#pragma unroll
                    for (uint32_t s = 0; s < 4u; s++) {
                        const uint32_t b = bb * 16u + 4u * s + lk;  // < bins_pad
#pragma unroll
                        for (uint32_t m = 0; m < MT; m++) {
                            const uint32_t f = m * 16u + li;
                            const float pv = s_p[b * g.p_stride + (f < TF ? f : 0u)];
                            const float av = f < nf ? pv : 0.0f;
                            acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, fv[s], acc[m], 0, 0, 0);
                        }
                    }
                }
                const uint32_t r = rt_ * 16u + li;
#pragma unroll
                for (uint32_t m = 0; m < MT; m++)
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) {
                        const uint32_t f = m * 16u + lk * 4u + q;
                        if (f < nf && r < R) emit(dst, (row0 + r) * frames + t0 + f, format, acc[m][q]);
                    }
            }
        }
        __syncthreads();  // s_x and s_p are written again by the next tile
    }
}

}  // namespace

// n <= 65535 (gridDim.y); max_items: the most (channel, tile) pairs of any window, which sizes
// gridDim.x; every window gets its result, whether it has frames or not
hipError_t launch_features(const FeatWindow *wins, const window::WindowResult *stage1, const uint64_t *totals,
                           const resample::Ratio &rt, const float *x, const float *table, const float *filters, uint8_t *out,
                           window::WindowResult *results, const feat::Params &ft, uint32_t K, uint32_t format, uint32_t n,
                           uint64_t max_items, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const FeatGeometry g = feat_geometry(ft.n_fft, ft.hop, ft.n_rows);
    const uint32_t gx = (uint32_t)(max_items > 1024u ? 1024u : (max_items ? max_items : 1u));
    if (g.frames == 32u)
        hipLaunchKernelGGL(k_features<2>, dim3(gx, n), dim3(64u * g.waves), g.lds_bytes, st, wins, stage1, totals, rt, x, table,
                           filters, out, results, ft, g, K, format);
    else
        hipLaunchKernelGGL(k_features<1>, dim3(gx, n), dim3(64u * g.waves), g.lds_bytes, st, wins, stage1, totals, rt, x, table,
                           filters, out, results, ft, g, K, format);
    return hipGetLastError();
}

}  // namespace fg
