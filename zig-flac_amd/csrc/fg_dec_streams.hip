// fg_dec_streams.hip -- the small kernels around k_dec_parse / k_dec_recon (fg_dec.hip) for decode
// chunks that hold frames of several streams (gfx950).  The rules are fg_streams.hpp's; a segment
// (one stream's frames inside one chunk) is one wave64 here.
//
//   k_streams_init     per stream: its result from the index result, its carried sample count 0
//   k_streams_gather   per segment: its frames' table entries from the stream's slice of the index
//                      table to the packed table the chunks are slices of
//   k_seg_offsets      per segment, between parse and reconstruct: per-frame PCM byte offsets from
//                      the parsed block sizes (segmented exclusive scan + the stream's base and
//                      carried count); the carried count moves on
//   k_seg_fold         per segment, after reconstruct: the frames' results into the stream's
//   k_streams_md5_lens per stream: the bytes to hash (0 for a stream that is not clean)
//   k_streams_md5_mask per stream: 16 zero bytes for a stream that is not clean
//
// Every index is bounded by what the host cut: first + count <= the chunk's frames <= max_frames,
// stream < n_streams.
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_dec.hpp"
#include "fg_index.hpp"
#include "fg_streams.hpp"

namespace fg {

using namespace streams;

namespace {

__global__ void __launch_bounds__(256) k_streams_init(const idx::IndexResult *ires, StreamResult *res, uint64_t *carried,
                                                       uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    StreamResult r;
    r.n_frames = ires[s].n_frames;
    r.n_samples = 0;
    r.index_status = ires[s].status;
    r.bad_frames = 0;
    r.first_bad_frame = kNone;
    r.first_bad_status = 0;
    res[s] = r;
    carried[s] = 0;
}

__global__ void __launch_bounds__(256) k_streams_gather(const Segment *segs, const uint64_t *table_first,
                                                         const uint64_t *f_off, const uint32_t *f_bytes, uint64_t *p_off,
                                                         uint32_t *p_bytes) {
    const Segment g = segs[blockIdx.x];
    const uint64_t src = table_first[g.stream] + g.frame0;
    for (uint32_t i = threadIdx.x; i < g.count; i += 256u) {
        p_off[g.packed + i] = f_off[src + i];
        p_bytes[g.packed + i] = f_bytes[src + i];
    }
}

__global__ void __launch_bounds__(64) k_seg_offsets(const Segment *segs, const uint32_t *blocks, const uint64_t *pcm_base,
                                                     const uint64_t *pcm_cap, uint64_t *carried, uint32_t per,
                                                     uint64_t *pcm_off) {
    const Segment g = segs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint64_t base = pcm_base[g.stream], cap = pcm_cap[g.stream];
    uint64_t carry = carried[g.stream];
    for (uint32_t i0 = 0; i0 < g.count; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const uint32_t x = i < g.count ? blocks[g.first + i] : 0u;
        uint32_t inc = x;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if (lane >= d) inc += y;
        }
        if (i < g.count) pcm_off[g.first + i] = frame_pcm_offset(base, cap, carry + (inc - x), x, per);
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) carried[g.stream] = carry;  // every lane read it before the loop: one wave
}

__global__ void __launch_bounds__(64) k_seg_fold(const Segment *segs, const dec::Result *results, StreamResult *res) {
    const Segment g = segs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    Fold f;
    for (uint32_t i = lane; i < g.count; i += 64u) {
        const dec::Result r = results[g.first + i];
        fold_frame(f, i, r.status, r.block_size);
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        Fold o;
        o.samples = __shfl_xor((unsigned long long)f.samples, d, 64);
        o.bad = __shfl_xor(f.bad, d, 64);
        o.first_bad = __shfl_xor(f.first_bad, d, 64);
        o.first_status = __shfl_xor(f.first_status, d, 64);
        fold_merge(f, o);
    }
    if (lane == 0) {
        StreamResult r = res[g.stream];
        fold_into(r, f, g.frame0);
        res[g.stream] = r;
    }
}

__device__ __forceinline__ bool stream_clean(const StreamResult &r) { return r.index_status == idx::IDX_OK && r.bad_frames == 0; }

__global__ void __launch_bounds__(256) k_streams_md5_lens(const StreamResult *res, uint32_t per, uint64_t *lens, uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    const StreamResult r = res[s];
    lens[s] = stream_clean(r) ? r.n_samples * per : 0ull;
}

__global__ void __launch_bounds__(256) k_streams_md5_mask(const StreamResult *res, uint8_t *digests, uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    if (stream_clean(res[s])) return;
    for (uint32_t k = 0; k < 16u; k++) digests[16u * (uint64_t)s + k] = 0;
}

}  // namespace

hipError_t launch_streams_init(const idx::IndexResult *ires, StreamResult *res, uint64_t *carried, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_streams_init, dim3((n + 255u) / 256u), dim3(256), 0, st, ires, res, carried, n);
    return hipGetLastError();
}

hipError_t launch_streams_gather(const Segment *segs, uint32_t n_segs, const uint64_t *table_first, const uint64_t *f_off,
                                 const uint32_t *f_bytes, uint64_t *p_off, uint32_t *p_bytes, hipStream_t st) {
    if (n_segs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_streams_gather, dim3(n_segs), dim3(256), 0, st, segs, table_first, f_off, f_bytes, p_off, p_bytes);
    return hipGetLastError();
}

hipError_t launch_seg_offsets(const Segment *segs, uint32_t n_segs, const uint32_t *blocks, const uint64_t *pcm_base,
                              const uint64_t *pcm_cap, uint64_t *carried, uint32_t per, uint64_t *pcm_off, hipStream_t st) {
    if (n_segs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_offsets, dim3(n_segs), dim3(64), 0, st, segs, blocks, pcm_base, pcm_cap, carried, per, pcm_off);
    return hipGetLastError();
}

hipError_t launch_seg_fold(const Segment *segs, uint32_t n_segs, const dec::Result *results, StreamResult *res,
                           hipStream_t st) {
    if (n_segs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_fold, dim3(n_segs), dim3(64), 0, st, segs, results, res);
    return hipGetLastError();
}

hipError_t launch_streams_md5_lens(const StreamResult *res, uint32_t per, uint64_t *lens, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_streams_md5_lens, dim3((n + 255u) / 256u), dim3(256), 0, st, res, per, lens, n);
    return hipGetLastError();
}

hipError_t launch_streams_md5_mask(const StreamResult *res, uint8_t *digests, uint32_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_streams_md5_mask, dim3((n + 255u) / 256u), dim3(256), 0, st, res, digests, n);
    return hipGetLastError();
}

}  // namespace fg
