// fg_fir.hip -- the kernel of the filtered delivery of sample windows (gfx950); the rules are
// fg_fir.hpp's, the narrowing fg_features.hpp's (feat::element), the results fg_window.hpp's.
//
//   k_window_fir   stage 2 of flacgpu_decode_windows_device_fir.  Stage 1 (the window delivery
//                  itself, planar F32 with padding) has left every window's span -- its samples and
//                  the T - 1 - d before and the d after them -- in the context's scratch, one plane a
//                  channel, and its results.  A workgroup (blockIdx.y: the window) takes tiles of
//                  2048 outputs of one channel; a wave holds two accumulators of 16 x 16 outputs,
//                  D[i][j] = y[tb + 16 i + j].  The taps run in chunks of at most 256 steps: per
//                  chunk the tile's sample span and the chunk's taps, zero-extended, go to LDS, and
//                  every step is one v_mfma_f32_16x16x4_f32 an accumulator over A[i][u] =
//                  x[tb + 16 i + 15 - u] and the Toeplitz operand B[u][j] = h[u + j - 15].
//
// The f32-input MFMA adds its four products to the accumulator one after the other, k ascending,
// each a correctly rounded fused multiply-add: with u ascending through the chunks an accumulator
// element is the chain of the rule, and the steps before and after a column's T taps multiply a zero
// tap by a finite sample (a staged sample, or zero where the span has none).
//
// Every index is bounded.  Samples: fir::span_at reads plane offsets below s_count, which stage 1
// wrote (its padding included), and gives zero elsewhere.  Taps: fir::tap_at reads row offsets in
// [0, T) of row r < rows, inside [tap_off, tap_off + rows * T), which the host checked against the
// caller's taps_len.  Elements: t < count of channel k < K, at out_off + t * K + k or out_off +
// k * count + t, below the K * count the capacity rule (deliver::too_small) checked.  LDS: sample
// slots q < g.span at fir::lds_pos(q) < g.plane, tap slots p < g.tap_words, within
// fir_geometry(kMaxTaps).lds_bytes, which the launch allocates (a shorter filter's is no larger).
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_deliver.hpp"
#include "fg_features.hpp"
#include "fg_fir.hpp"
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

constexpr uint32_t ACCS = kFirAccs;

__global__ void __launch_bounds__(256) k_window_fir(const FirWindow *wins, const WindowResult *stage1, const uint64_t *totals,
                                                     resample::Ratio rt, const float *x, const float *taps, uint8_t *out,
                                                     WindowResult *results, uint32_t K, uint32_t format, uint32_t flags) {
    extern __shared__ float s_mem[];
    const uint32_t w = blockIdx.y, tid = threadIdx.x;
    const FirWindow a = wins[w];
    WindowResult r1 = stage1[w];
    uint64_t total = totals[a.stream];
    if (rt.L) total = resample::out_total(rt, total);
    const uint64_t n = resample::delivered(total, a.start, a.count);
    // the statuses in the order of the window delivery: the index, the capacity, the frames
    if (r1.status != WIN_BAD_INDEX && deliver::too_small(n, a.count, flags, a.cap, K)) {
        r1.status = WIN_TOO_SMALL;
        r1.n_frames = 0;
        r1.first_bad_frame = streams::kNone;
        r1.first_bad_status = 0;
    }
    const bool ok = r1.status == WIN_OK;
    if (blockIdx.x == 0 && tid == 0) {
        r1.n_samples = ok ? n : 0ull;
        results[w] = r1;
    }
    const uint64_t written = deliver::written_samples(n, a.count, flags);
    if (!ok || written == 0) return;
    const uint32_t T = a.taps;
    const FirGeometry g = fir_geometry(T);
    float *s_x = s_mem, *s_h = s_mem + g.plane;
    const uint32_t wave = tid >> 6, lane = tid & 63u, li = lane & 15u, lk = lane >> 4;
    const uint32_t n_steps = fir::steps(T), count = a.count;
    const bool planar = (flags & deliver::DELIVER_PLANAR) != 0;
    const uint64_t tiles = (written + g.tile - 1u) / g.tile, items = (uint64_t)K * tiles;
    uint8_t *dst = out + a.out_off * deliver::elem_size(format);
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t k = (uint32_t)(item / tiles);
        const uint64_t t0 = (item - (uint64_t)k * tiles) * g.tile, tw = t0 + (uint64_t)wave * (ACCS * 256u);
        const float *xp = x + a.x_off + (uint64_t)k * a.s_count;
        const float *row = taps + a.tap_off + (a.rows == 1u ? 0u : (uint64_t)k * T);
        f32x4 acc[ACCS];
#pragma unroll
        for (uint32_t m = 0; m < ACCS; m++) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (t0 < n) {  // a tile of padding alone computes nothing
            for (uint32_t u0 = 0; u0 < n_steps; u0 += g.chunk) {
                const int64_t lo = fir::stage_lo(t0, T, u0, g.chunk);
                for (uint32_t q = tid; q < g.span; q += 256u) s_x[fir::lds_pos(q)] = fir::span_at(xp, a.s_count, a.clip, lo + q);
                for (uint32_t p = tid; p < g.tap_words; p += 256u) s_h[p] = fir::tap_at(row, T, fir::stage_tap(u0, p));
                __syncthreads();
                if (tw < n) {  // a wave whose outputs are all padding issues nothing
                    const uint32_t nu = n_steps - u0 < g.chunk ? n_steps - u0 : g.chunk;  // a multiple of 4
                    for (uint32_t uu = lk; uu < nu; uu += 4u) {
                        const float bv = s_h[fir::b_slot(uu, li)];
#pragma unroll
                        for (uint32_t m = 0; m < ACCS; m++) {
                            const float av = s_x[fir::lds_pos(fir::a_slot(wave * (ACCS * 16u) + m * 16u + li, uu, g.chunk))];
                            acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[m], 0, 0, 0);
                        }
                    }
                }
                __syncthreads();  // s_x and s_h are written again by the next chunk
            }
        }
        // accumulator register q of lane l: row (l >> 4) * 4 + q of the 16, column l & 15
#pragma unroll
        for (uint32_t m = 0; m < ACCS; m++)
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint64_t t = tw + m * 256u + 16u * (lk * 4u + q) + li;
                if (t >= written) continue;
                const float v = t < n ? fir::plus_zero(acc[m][q]) : 0.0f;
                emit(dst, planar ? (uint64_t)k * count + t : t * K + k, format, v);
            }
    }
}

}  // namespace

// n <= 65535 (gridDim.y); max_items: the most (channel, tile) pairs of any window, which sizes
// gridDim.x; every window gets its result, whether it has samples or not
hipError_t launch_window_fir(const FirWindow *wins, const window::WindowResult *stage1, const uint64_t *totals,
                             const resample::Ratio &rt, const float *x, const float *taps, uint8_t *out,
                             window::WindowResult *results, uint32_t K, uint32_t format, uint32_t flags, uint32_t n,
                             uint64_t max_items, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const FirGeometry g = fir_geometry(fir::kMaxTaps);
    const uint32_t gx = (uint32_t)(max_items > 1024u ? 1024u : (max_items ? max_items : 1u));
    hipLaunchKernelGGL(k_window_fir, dim3(gx, n), dim3(64u * g.waves), g.lds_bytes, st, wins, stage1, totals, rt, x, taps, out,
                       results, K, format, flags);
    return hipGetLastError();
}

}  // namespace fg
