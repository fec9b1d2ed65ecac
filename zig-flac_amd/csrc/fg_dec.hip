// fg_dec.hip -- the device FLAC frame decoder / verifier (gfx950): frames resident in HBM, in the
// layout the encode entry points leave them, back to interleaved PCM and / or compared with it.
//
//   k_dec_parse   one lane per frame: header parse + subframe walk of fg_dec.hpp (sequential by
//                 nature: every Rice code's length depends on its bits); leaves one DecSub per
//                 subframe, the block size and the provisional status.
//   k_dec_recon   persistent grid over frames (atomic ticket), one wave64 per subframe: lane s
//                 decodes segment s (seg_len(block size) = 64, 128 or 256 samples) into LDS, the
//                 wave restores the samples (FIXED:
//                 nested running sums by wave scans; LPC: the serial chain on one lane, history
//                 in registers), then the workgroup undoes the stereo decorrelation, checks the
//                 CRC-16 and the sample range, and writes / compares the interleaved PCM in
//                 16-byte units from LDS.
//
// Hostile bytes: every bitstream read goes through the bounded BitReader; every LDS / PCM write
// is indexed by i < block_size <= the context's block size, for which dec_geometry (fg_geom.hpp)
// sized the planes (<= 16384; <= 8192 with 64-bit planes).
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>

#include "fg_common.hpp"
#include "fg_dec.hpp"
#include "fg_geom.hpp"

namespace fg {

using namespace dec;

namespace {

// Two instantiations of everything below: BIG = false for a context whose frames have at most 4096
// samples -- the segment shift 6 and the plane stride kPlane are compile-time constants, the code
// such a context ran before larger frames existed -- and BIG = true, where the shift is the
// frame's (seg_shift(bs): 6, 7 or 8) and the stride the context's (DecGeom::plane_words).
constexpr uint32_t kPlane = 4096 + 4096 / 64;  // one subframe's samples, one pad word per segment
// sample i of a plane, S = the frame's segment shift: lane s's L = 2^S consecutive samples start
// one bank further than lane s-1's (stride L + 1 words, odd), so the per-lane walks of the 64 lanes
// touch 64 different banks, as they did with L = 64.  i + (i >> 6) for every L would start the lanes
// 65 L / 64 words apart: 130 or 260, even.  (Reasoned from the 64 banks of 4 bytes; not measured.)
// The largest index, bs - 1 + ((bs - 1) >> S) with bs <= B = 4096 << (S - 6), is below B + 64 <= B + B / 64.
__device__ __forceinline__ uint32_t phys(uint32_t i, uint32_t S) { return i + (i >> S); }

enum : uint32_t { FLAG_RANGE = 1, FLAG_SUB = 2, FLAG_TRUNC = 4 };

// ---------------------------------------------------------------------------------------------
template <bool BIG>
__global__ void __launch_bounds__(64) k_dec_parse(Args a) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f == 0) {
        *a.ticket = 0;
        *a.bad = 0;
    }
    if (f >= a.n_frames) return;
    FrameHdr h;
    uint32_t body = 0;
    // BIG = false: a.block <= 4096 (launch_dec_parse), so no frame with longer segments is walked
    const uint32_t st = parse_frame_upto<BIG ? 8u : 6u>(a.frames + a.frame_off[f], a.frame_bytes[f], a.rate, a.channels, a.bits,
                                                        a.block, h, a.subs + (size_t)f * a.channels, body);
    Result r;
    r.status = st;
    r.block_size = h.block_size;
    r.number = h.number;
    r.sample_rate = h.sample_rate;
    r.first_bad = 0;
    r.channel_assign = (uint8_t)h.channel_assign;
    r.bits = (uint8_t)h.bits;
    for (int k = 0; k < 6; k++) r.pad[k] = 0;
    a.results[f] = r;
    a.blocks[f] = (h.block_size && h.block_size <= a.block) ? h.block_size : 0u;
    a.body[f] = body;
}

// ---------------------------------------------------------------------------------------------
template <typename U>
__device__ __forceinline__ U wave_incl_scan(U x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const U y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// x[i] = r[i] + ((sum_j c[j] x[i-1-j]) >> shift) for i >= order, in place, on the calling lane.
// The shift makes it a serial chain; the last M samples stay in registers (a ring indexed at
// compile time), the taps past `order` are zero.  i64 accumulation as in the verifier decoder.
template <typename T, int M>
__device__ __forceinline__ void lpc_chain(T *pl, uint32_t bs, uint32_t order, const int32_t (&cf)[M], uint32_t shift,
                                          uint32_t S) {
    using U = typename std::make_unsigned<T>::type;
    T h[M];
#pragma unroll
    for (int u = 0; u < M; u++) h[u] = 0;
    for (uint32_t base = 0; base < bs; base += M) {
        // the next M residuals first: their LDS latency stays off the chain (nothing below writes them
        // before it has used them)
        T r[M];
#pragma unroll
        for (int u = 0; u < M; u++) r[u] = base + (uint32_t)u < bs ? pl[phys(base + (uint32_t)u, S)] : (T)0;
#pragma unroll
        for (int u = 0; u < M; u++) {
            const uint32_t i = base + (uint32_t)u;
            if (i < bs) {
                T x = r[u];
                if (i >= order) {
                    uint64_t acc = 0;
#pragma unroll
                    for (int j = 0; j < M; j++)
                        acc += (uint64_t)(int64_t)cf[j] * (uint64_t)(int64_t)h[(u - 1 - j + 2 * M) % M];
                    x = (T)((U)x + (U)((int64_t)acc >> shift));
                    pl[phys(i, S)] = x;
                }
                h[u] = x;
            }
        }
    }
}

template <typename T, int M, bool BIG>
__device__ __noinline__ void lpc_restore(T *pl, const uint8_t *p, uint32_t len, const DecSub &d, uint32_t bs, uint32_t sh) {
    const uint32_t S = BIG ? sh : 6u;
    int32_t cf[M];
#pragma unroll
    for (int j = 0; j < M; j++) {
        cf[j] = 0;
        if ((uint32_t)j < d.order) {
            BitReader b = br_make(p, len, d.coef_pos + (uint32_t)j * d.prec);
            cf[j] = (int32_t)br_s(b, d.prec);
        }
    }
    lpc_chain<T, M>(pl, bs, d.order, cf, d.shift, S);
}

// One wave restores one subframe into its plane (samples after the waste shift).  Lane s owns
// segment s: samples [L s, L s + L), L = 2^S = seg_len(bs).
template <typename T, bool BIG>
__device__ void restore_subframe(T *pl, const uint8_t *p, uint32_t len, const DecSub &d, uint32_t bs, uint32_t sh,
                                 uint32_t lane, uint32_t *flags) {
    using U = typename std::make_unsigned<T>::type;
    const uint32_t sbps = d.sbps, order = d.order;
    const uint32_t S = BIG ? sh : 6u, L = 1u << S;
    if (!BIG) __builtin_assume(bs <= 4096u);  // decode_segment's seg_len(bs) folds to 64
    if (d.type == SUB_CONSTANT) {
        BitReader b = br_make(p, len, d.warm_pos);
        const T v = (T)br_s(b, sbps);
        for (uint32_t i = lane; i < bs; i += 64u) pl[phys(i, S)] = v;
    } else if (d.type == SUB_VERBATIM) {
        for (uint32_t j = 0; j < L; j++) {
            const uint32_t i = L * lane + j;
            if (i < bs) {
                BitReader b = br_make(p, len, d.warm_pos + i * sbps);
                pl[phys(i, S)] = (T)br_s(b, sbps);
            }
        }
    } else {
        // residuals: lane s decodes segment s, then the continuity check against segment s + 1
        uint32_t err = 0;
        const uint32_t end = decode_segment(p, len, d, bs, lane, err, [&](uint32_t i, int64_t v) {
            if (i < bs) pl[phys(i, S)] = (T)v;
        });
        const uint32_t next = lane < 63u ? d.seg_pos[lane + 1u] : d.end_pos;
        if (end != next) atomicOr(flags, FLAG_SUB);
        if (err) atomicOr(flags, FLAG_TRUNC);
        if (d.type == SUB_LPC) {
            if (lane < order) {
                BitReader b = br_make(p, len, d.warm_pos + lane * sbps);
                pl[phys(lane, S)] = (T)br_s(b, sbps);
            }
            __threadfence_block();
            if (lane == 0) {
                if (order <= 8u) lpc_restore<T, 8, BIG>(pl, p, len, d, bs, S);
                else if (order <= 12u) lpc_restore<T, 12, BIG>(pl, p, len, d, bs, S);
                else lpc_restore<T, 32, BIG>(pl, p, len, d, bs, S);
            }
        } else if (order > 0) {
            // FIXED order k: k nested running sums (RFC 9639 9.2.5: the predictors are the k-th
            // differences).  Level j turns the j-th differences of samples k.. into the (j-1)-th:
            // a prefix sum whose start value is the (j-1)-th difference at sample k-1, from the
            // warm-up.  Per level: lane-local sum, wave exclusive scan of the lane totals, second
            // lane-local pass.  Sums wrap in U: exact whenever the true values fit T.
            U w[4] = {0, 0, 0, 0};  // w[m] = warm-up sample k-1-m
#pragma unroll
            for (uint32_t m = 0; m < 4u; m++)
                if (m < order) {
                    BitReader b = br_make(p, len, d.warm_pos + (order - 1u - m) * sbps);
                    w[m] = (U)(T)br_s(b, sbps);
                }
            const U init[4] = {w[0], (U)(w[0] - w[1]), (U)(w[0] - 2u * w[1] + w[2]),
                               (U)(w[0] - 3u * w[1] + 3u * w[2] - w[3])};
            __threadfence_block();
            for (uint32_t lvl = order; lvl >= 1u; lvl--) {
                const U ini = lvl == 1u ? init[0] : lvl == 2u ? init[1] : lvl == 3u ? init[2] : init[3];
                U tot = 0;
                for (uint32_t j = 0; j < L; j++) {
                    const uint32_t i = L * lane + j;
                    if (i >= order && i < bs) tot += (U)pl[phys(i, S)];
                }
                U run = wave_incl_scan<U>(tot, lane) - tot + ini;
                for (uint32_t j = 0; j < L; j++) {
                    const uint32_t i = L * lane + j;
                    if (i >= order && i < bs) {
                        run += (U)pl[phys(i, S)];
                        pl[phys(i, S)] = (T)run;
                    }
                }
            }
            if (lane == 0)
                for (uint32_t m = 0; m < 4u; m++)
                    if (m < order) pl[phys(order - 1u - m, S)] = (T)w[m];
        }
    }
    __threadfence_block();
    if (d.waste)  // 9.2.2: the wasted bits come back as zeros
        for (uint32_t i = lane; i < bs; i += 64u) pl[phys(i, S)] = (T)((U)pl[phys(i, S)] << d.waste);
}

// The interleaved little-endian PCM of the frame region [base, base + nb), in 16-byte units of the
// absolute address: written (CMP = false) or compared with what is there (CMP = true: the first
// differing interleaved sample goes to *first_bad by atomicMin).  Channels c0 .. c0 + wc - 1 are in
// `planes` (`plane` elements apart, the frame's segment shift S); a unit that is not whole (the
// region's edges, or channels of another round) goes byte by byte.
template <typename T, bool CMP>
__device__ void emit(const T *planes, uint32_t plane, uint32_t S, uint32_t C, uint32_t c0, uint32_t wc, uint32_t bps,
                     uint32_t nb, uint8_t *base, uint32_t tid, uint32_t nt, uint32_t *first_bad) {
    const uintptr_t A = (uintptr_t)base, U0 = A & ~(uintptr_t)15;
    const uint32_t units = (uint32_t)((A + nb - U0 + 15u) >> 4);
    for (uint32_t u = tid; u < units; u += nt) {
        const int32_t gb0 = (int32_t)((intptr_t)(U0 + 16u * (uintptr_t)u) - (intptr_t)A);  // region byte of the unit's byte 0
        const int32_t lo = gb0 < 0 ? 0 : gb0, hi = gb0 + 16 < (int32_t)nb ? gb0 + 16 : (int32_t)nb;
        uint32_t e = (uint32_t)lo / bps;
        uint32_t i = e / C, c = e - i * C;
        uint64_t q0 = 0, q1 = 0;
        uint32_t mask = 0;
        for (; (int32_t)(e * bps) < hi; e++) {
            if (c >= c0 && c < c0 + wc) {
                const uint64_t v = (uint64_t)(int64_t)planes[(c - c0) * plane + phys(i, S)];
                for (uint32_t o = 0; o < bps; o++) {
                    const int32_t b = (int32_t)(e * bps + o);
                    if (b >= lo && b < hi) {
                        const uint32_t k = (uint32_t)(b - gb0);
                        const uint64_t byte = (v >> (8u * o)) & 255u;
                        if (k < 8u) q0 |= byte << (8u * k);
                        else q1 |= byte << (8u * (k - 8u));
                        mask |= 1u << k;
                    }
                }
            }
            if (++c == C) {
                c = 0;
                i++;
            }
        }
        uint8_t *dst = base + gb0;
        if (mask == 0xFFFFu) {
            if (!CMP) {
                *(uint4 *)dst = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
            } else {
                const uint4 x = *(const uint4 *)dst;
                const uint64_t d0 = q0 ^ ((uint64_t)x.x | ((uint64_t)x.y << 32)), d1 = q1 ^ ((uint64_t)x.z | ((uint64_t)x.w << 32));
                if (d0 | d1) {
                    const uint32_t k = d0 ? (uint32_t)__builtin_ctzll(d0) >> 3 : 8u + ((uint32_t)__builtin_ctzll(d1) >> 3);
                    atomicMin(first_bad, (uint32_t)(gb0 + (int32_t)k) / bps);
                }
            }
        } else {
            for (uint32_t k = 0; k < 16u; k++)
                if (mask & (1u << k)) {
                    const uint8_t byte = (uint8_t)((k < 8u ? q0 >> (8u * k) : q1 >> (8u * (k - 8u))) & 255u);
                    if (!CMP) dst[k] = byte;
                    else if (dst[k] != byte) atomicMin(first_bad, (uint32_t)(gb0 + (int32_t)k) / bps);
                }
        }
    }
}

// W waves = W subframes at a time; a frame of more channels than W takes several rounds.
// plane_words: DecGeom's (BIG = false: kPlane, a constant here).
template <typename T, bool BIG>
__global__ void __launch_bounds__(512) k_dec_recon(Args a, uint32_t W, uint32_t plane_words) {
    extern __shared__ __align__(16) uint8_t smem[];
    T *planes = (T *)smem;
    __shared__ uint32_t s_f, s_flags, s_crc, s_bad;
    static_assert(4 * sizeof(uint32_t) == kDecStaticLds, "dec_geometry's LDS budget leaves room for these");
    const uint32_t plane = BIG ? plane_words : kPlane;
    const uint32_t tid = threadIdx.x, nt = blockDim.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t C = a.channels, bps = a.bps;
    for (;;) {
        __syncthreads();
        if (tid == 0) {
            s_f = atomicAdd(a.ticket, 1u);
            s_flags = 0;
            s_crc = 0;
            s_bad = 0xFFFFFFFFu;
        }
        __syncthreads();
        const uint32_t f = s_f;
        if (f >= a.n_frames) break;
        Result *R = &a.results[f];
        uint32_t st = R->status, first_bad = 0;
        const uint8_t *p = a.frames + a.frame_off[f];
        const uint32_t len = a.frame_bytes[f], bs = R->block_size, chc = R->channel_assign, body = a.body[f];
        const uint32_t S = BIG ? seg_shift(bs) : 6u;  // st == 0: bs <= a.block, which the planes were sized for
        if (st == 0) {
            // CRC-16 over the body: thread t folds the t-th of nt equal pieces (the first ones
            // start before the frame: leading zeros leave an init-0 CRC at 0) byte by byte, then
            // shifts it past the pieces after it: times z^(8 cb (nt-1-t)) mod P
            const uint32_t cb = (body + nt - 1u) / nt;
            const int64_t start = (int64_t)body - (int64_t)(nt - tid) * cb;
            uint32_t crc = 0;
            for (uint32_t k = 0; k < cb; k++) {
                const int64_t idx = start + k;
                if (idx >= 0) crc = crc_byte_v(crc, p[idx]);
            }
            uint32_t g = 1, sq = 0x100u;  // g = z^(8 cb)
            for (uint32_t e = cb; e; e >>= 1) {
                if (e & 1u) g = crc_mulmod_v(g, sq);
                sq = crc_mulmod_v(sq, sq);
            }
            uint32_t m = 1;
            for (uint32_t e = nt - 1u - tid; e; e >>= 1) {
                if (e & 1u) m = crc_mulmod_v(m, g);
                g = crc_mulmod_v(g, g);
            }
            crc = crc_mulmod_v(crc, m);
            if (crc) atomicXor(&s_crc, crc);
            __syncthreads();
            if (s_crc != (((uint32_t)p[body] << 8) | p[body + 1u])) st = ST_CRC16;
            else if (body + 2u != len) st = ST_SYNC;  // bytes after the CRC-16 are no frame
        }
        if (st == 0 && a.exp_number && (R->number != a.exp_number[f] || bs != a.exp_n[f])) {
            st = ST_MISMATCH;
            first_bad = 0xFFFFFFFFu;
        }
        const uint32_t nb = bs * C * bps;
        const uint64_t off = a.pcm_off ? a.pcm_off[f] : (st == 0 ? a.samp_off[f] * C * bps : 0);
        if (st == 0 && a.out && (off > a.cap || nb > a.cap - off)) st = ST_RANGE;
        if (st == 0) {
            // one round when the planes of all channels fit; else a checking pass, then a writing one
            const uint32_t npass = C > W ? 2u : 1u;
            for (uint32_t pass = 0; pass < npass && st == 0; pass++) {
                for (uint32_t c0 = 0; c0 < C; c0 += W) {
                    const uint32_t wc = C - c0 < W ? C - c0 : W;
                    __syncthreads();
                    if (wv < wc) {
                        const uint32_t c = c0 + wv;
                        restore_subframe<T, BIG>(planes + wv * plane, p, len, a.subs[(size_t)f * C + c], bs, S, lane, &s_flags);
                    }
                    __syncthreads();
                    if (C == 2u && chc >= 8u) {  // 9.1.3: left/side, side/right, mid/side
                        using U = typename std::make_unsigned<T>::type;
                        for (uint32_t i = tid; i < bs; i += nt) {
                            const uint32_t q = phys(i, S);
                            const U x = (U)planes[q], s = (U)planes[plane + q];
                            if (chc == 8u) planes[plane + q] = (T)(x - s);
                            else if (chc == 9u) planes[q] = (T)(x + s);
                            else {
                                const U mid = x * 2u + (s & 1u);
                                planes[q] = (T)(mid + s) >> 1;
                                planes[plane + q] = (T)(mid - s) >> 1;
                            }
                        }
                        __syncthreads();
                    }
                    if (pass == 0) {
                        uint32_t bad = 0;
                        for (uint32_t e = tid; e < wc * bs; e += nt) {
                            const uint32_t w = e / bs, i = e - w * bs;
                            if (!sample_in_range((int64_t)planes[w * plane + phys(i, S)], a.bits)) bad = 1;
                        }
                        if (bad) atomicOr(&s_flags, FLAG_RANGE);
                        __syncthreads();
                    }
                    if (pass + 1u == npass && s_flags == 0) {
                        if (a.out) emit<T, false>(planes, plane, S, C, c0, wc, bps, nb, a.out + off, tid, nt, nullptr);
                        if (a.expect)
                            emit<T, true>(planes, plane, S, C, c0, wc, bps, nb, const_cast<uint8_t *>(a.expect) + off, tid, nt,
                                          &s_bad);
                    }
                }
                __syncthreads();
                const uint32_t fl = s_flags;
                if (fl & FLAG_SUB) st = ST_SUBFRAME;
                else if (fl & FLAG_TRUNC) st = ST_TRUNCATED;
                else if (fl & FLAG_RANGE) st = ST_RANGE;
            }
            if (st == 0 && s_bad != 0xFFFFFFFFu) {
                st = ST_MISMATCH;
                first_bad = s_bad;
            }
        }
        if (tid == 0) {
            R->status = st;
            R->first_bad = first_bad;
            if (st) atomicAdd(a.bad, 1u);
        }
    }
}

template <typename KernelT>
hipError_t launch_recon(KernelT k, const Args &a, const DecGeom &g, hipStream_t st) {
    struct Occ {
        const void *fn;
        uint32_t W, lds;
        int device, grid;
    };
    static Occ cache[64];
    static int n_cache = 0;
    static std::mutex mu;
    const uint32_t W = g.W, lds = g.lds;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    int grid = 0;
    uint32_t asked = 0;  // the most dynamic LDS this kernel has been allowed on this device
    {
        std::lock_guard<std::mutex> lock(mu);
        for (int i = 0; i < n_cache; i++)
            if (cache[i].fn == (const void *)k && cache[i].device == dev) {
                if (cache[i].W == W && cache[i].lds == lds) grid = cache[i].grid;
                if (cache[i].lds > asked) asked = cache[i].lds;
            }
    }
    if (!grid) {
        // (the kernel's few static words count against the 160 KiB too: ask for what the planes need;
        // never for less than an earlier geometry of the same kernel was given)
        if (lds > asked) {
            e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        int cus = 0, nb = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) return e;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k, (int)(64u * W), (size_t)lds);
        if (e != hipSuccess) return e;
        grid = (nb > 0 ? nb : 1) * (cus > 0 ? cus : 256);
        std::lock_guard<std::mutex> lock(mu);
        if (n_cache < 64) cache[n_cache++] = {(const void *)k, W, lds, dev, grid};
    }
    const uint32_t ng = a.n_frames < (uint32_t)grid ? a.n_frames : (uint32_t)grid;
    hipLaunchKernelGGL(k, dim3(ng), dim3(64u * W), lds, st, a, W, g.plane_words);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_dec_parse(const Args &a, hipStream_t st) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.block <= 4096u) hipLaunchKernelGGL(k_dec_parse<false>, dim3((a.n_frames + 63u) / 64u), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(k_dec_parse<true>, dim3((a.n_frames + 63u) / 64u), dim3(64), 0, st, a);
    return hipGetLastError();
}

// Waves, plane size and LDS are dec_geometry's (fg_geom.hpp) for the context's channels, depth and
// block size: i32 planes at 8/16/24 bits, i64 planes at 32 (the 33-bit side channel, and the 64-bit
// sums of the verifier decoder).  A context of blocks up to 4096 runs the BIG = false kernels.
hipError_t launch_dec_recon(const Args &a, hipStream_t st) {
    if (a.n_frames == 0) return hipSuccess;
    const DecGeom g = dec_geometry(a.channels, a.bits, a.block);
    if (!g.ok) return hipErrorInvalidValue;  // no context is opened with such a block size
    if (a.block <= 4096u) {
        static_assert(kPlane == 4096 + 4096 / 64, "dec_geometry's plane of a block of at most 4096");
        if (g.plane_words != kPlane) return hipErrorInvalidValue;
        return a.bits == 32u ? launch_recon(k_dec_recon<int64_t, false>, a, g, st)
                             : launch_recon(k_dec_recon<int32_t, false>, a, g, st);
    }
    return a.bits == 32u ? launch_recon(k_dec_recon<int64_t, true>, a, g, st)
                         : launch_recon(k_dec_recon<int32_t, true>, a, g, st);
}

// verify: the expected PCM offset, frame number and sample count of every frame, from a plan's frame table
__global__ void k_dec_expect(const FrameJob *jobs, uint64_t n, uint64_t *pcm_off, uint64_t *number, uint32_t *ns) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const FrameJob job = jobs[j];
    if (job.slot >= n) return;
    pcm_off[job.slot] = job.pcm_off;
    number[job.slot] = job.number;
    ns[job.slot] = job.n;
}
hipError_t launch_dec_expect(const FrameJob *jobs, uint64_t n, uint64_t *pcm_off, uint64_t *number, uint32_t *ns,
                             hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dec_expect, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, jobs, n, pcm_off, number, ns);
    return hipGetLastError();
}

}  // namespace fg
