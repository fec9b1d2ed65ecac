// fg_quantize.hip -- the kernel that turns tensor elements into the encoder's PCM (gfx950); the
// rules and the PCM writer are fg_quantize.hpp's.
//
//   k_elements_pcm   flacgpu_pcm_from_elements_device: many streams in one launch, the stream from
//                    blockIdx.y, its row of the device table uniform over the workgroup.  A lane
//                    takes units of 4 consecutive interleaved samples: it reads their 4 elements
//                    (2 or 4 bytes each, at any element alignment, so element by element) and
//                    stores the unit's B = bits / 8 whole words.  Consecutive lanes take
//                    consecutive units: a wave's loads cover one contiguous run of 256 elements a
//                    plane (interleaved: of the source) and its stores one contiguous run of
//                    256 B bytes, 4 to 16 bytes a lane.  The workgroups of a stream stride over its
//                    units.  Clipped elements are counted in a register, summed over the wave by
//                    shuffles, and added by one lane with one atomicAdd a wave that has any.
//
// Every index is bounded: a unit u < units(n) reads interleaved samples i < n = T * C, that is
// source elements below C * plane_stride (planar, plane_stride >= T) or T * C, and stores words
// below pcm_words(n, B) of the stream's PCM, which the host checked against the buffer's capacity
// and the next stream's offset.
#include <hip/hip_runtime.h>

#include "fg_common.hpp"
#include "fg_quantize.hpp"

namespace fg {

using namespace quantize;

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxGridX = 1u << 16;  // workgroups a stream's units are strided over

template <uint32_t B>
__global__ void __launch_bounds__(kThreads) k_elements_pcm(const Stream *tab, uint8_t *pcm, unsigned long long *clipped, uint32_t C,
                                                            uint32_t format, uint32_t planar) {
    const Stream st = tab[blockIdx.y];
    const uint64_t n = st.samples * C, nu = units(n);
    uint32_t *words = (uint32_t *)(pcm + st.pcm_off);
    const uint64_t step = (uint64_t)gridDim.x * kThreads;
    uint32_t count = 0;
    if (n >> 32) {
        for (uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x; u < nu; u += step)
            count += convert_unit<uint64_t>(st, words, u, n, C, B, format, planar != 0u);
    } else {
        for (uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x; u < nu; u += step)
            count += convert_unit<uint32_t>(st, words, u, n, C, B, format, planar != 0u);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
    if ((threadIdx.x & 63u) == 0u && count) atomicAdd(&clipped[blockIdx.y], (unsigned long long)count);
}

}  // namespace

// d_clipped[s] is zeroed on st before the launch.  max_units: the units of the longest stream.
hipError_t launch_elements_pcm(const Stream *d_tab, uint32_t n_streams, uint64_t max_units, uint8_t *d_pcm, uint64_t *d_clipped,
                               uint32_t C, uint32_t B, uint32_t format, bool planar, hipStream_t st) {
    if (!n_streams) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_clipped, 0, (uint64_t)n_streams * 8u, st);
    if (e != hipSuccess || !max_units) return e;
    const uint64_t wgs = (max_units + kThreads - 1u) / kThreads;
    const dim3 grid((uint32_t)(wgs < kMaxGridX ? wgs : kMaxGridX), n_streams);
    unsigned long long *cl = (unsigned long long *)d_clipped;
    const uint32_t pl = planar ? 1u : 0u;
    switch (B) {
        case 1: hipLaunchKernelGGL(k_elements_pcm<1>, grid, dim3(kThreads), 0, st, d_tab, d_pcm, cl, C, format, pl); break;
        case 2: hipLaunchKernelGGL(k_elements_pcm<2>, grid, dim3(kThreads), 0, st, d_tab, d_pcm, cl, C, format, pl); break;
        case 3: hipLaunchKernelGGL(k_elements_pcm<3>, grid, dim3(kThreads), 0, st, d_tab, d_pcm, cl, C, format, pl); break;
        default: hipLaunchKernelGGL(k_elements_pcm<4>, grid, dim3(kThreads), 0, st, d_tab, d_pcm, cl, C, format, pl); break;
    }
    return hipGetLastError();
}

}  // namespace fg
