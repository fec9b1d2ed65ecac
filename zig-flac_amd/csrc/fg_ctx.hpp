// fg_ctx.hpp -- the context and plan behind the C ABI's opaque handles, and the small host
// helpers every device-driving translation unit uses: error mapping, stream choice, kernel timing
// brackets, the grow-only device buffer.  Private to fg_api.cpp, fg_dec_host.cpp and fg_comm.cpp;
// fg_file.cpp and fg_multi.cpp see a context only through the accessors of fg_internal.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/flacgpu.h"
#include "fg_common.hpp"
#include "fg_geom.hpp"
#include "fg_md5_host.hpp"

struct DecScratch;  // fg_dec_host.cpp: decode scratch of a context
struct IdxScratch;  // fg_dec_host.cpp: index scratch of a context

namespace fg {

struct TimedLaunch {
    int kernel;
    hipEvent_t start, stop;
};

}  // namespace fg

struct flacgpu_ctx {
    int device = 0;
    flacgpu_config cfg{};
    uint32_t max_frames = 0;
    // flacgpu_open_decoder: cfg holds the stream and block_size = max_block (the encode options zero),
    // g only C, B, bits and md5_kernel; of everything below only `stream`, the event pool, the timing
    // and host MD5 state and the decoder scratch exist.  Every encode entry point refuses it.
    bool decode_only = false;
    fg::Knobs k;    // the environment's knobs when the context was opened
    fg::EncGeom g;  // kernel variants, thread counts, LDS and image sizes: enc_geometry(cfg, k)

    // ---- streams and events ----
    hipStream_t stream = nullptr, aux = nullptr;
    hipStream_t dl = nullptr;  // download stream of the pipelined host-buffer path
    hipStream_t up = nullptr;  // its upload stream (chunk i+1's upload beside chunk i's encode)
    hipStream_t ovl = nullptr;  // overlapped encode: scan + pack of range i
    hipEvent_t fork = nullptr, join = nullptr;
    std::vector<hipEvent_t> event_pool;

    // ---- encode buffers ----
    uint16_t *d_crc_pow = nullptr, *d_crc_join = nullptr, *d_crc_pow4 = nullptr;
    uint16_t *d_crc_pows = nullptr;  // CRC fold shifts for the split pack's thread count
    uint16_t *d_crc_powf = nullptr;  // CRC fold shifts for the fused kernel's 256 threads
    uint16_t *d_crc_x8 = nullptr;    // z^(8 * 2^i) mod P, i < 24
    uint32_t *d_err = nullptr, *d_ctr = nullptr;
    fg::FrameJob *d_jobs = nullptr;
    uint8_t *d_desc = nullptr;
    uint32_t *d_fbytes = nullptr;
    uint64_t *d_offsets = nullptr, *d_total = nullptr;
    uint8_t *d_pcm = nullptr;
    uint64_t pcm_cap = 0;
    uint8_t *d_out = nullptr;
    uint64_t out_cap = 0;
    uint64_t *d_scan_part = nullptr;  // per-4096-frame block sums of the multi-workgroup scan
    uint32_t scan_part_cap = 0;
    uint64_t *d_status = nullptr;  // fused encode: per-slot status words, grow-only
    uint64_t status_cap = 0;
    uint64_t *d_cum = nullptr;  // [chunk] bytes of the frames before the chunk's slot range
    uint32_t grid_reserve = 0;  // per call: slots the next analysis / pack launches leave free
    // overlapped encode (encode_core): the full frames in `ovl_chunks` ranges, the analysis of
    // range i+1 on `stream` beside the scan + pack of range i on `ovl`, each grid capped to
    // ovl_ana / ovl_pack workgroups per CU so both are resident on every CU (flacgpu_set_overlap)
    uint32_t ovl_chunks = 0, ovl_ana = 2, ovl_pack = 2, ovl_min_frames = 4096;

    // ---- pipelined host-buffer path (encode_pipelined) ----
    hipEvent_t up_done[kPipeSets] = {};  // a chunk set's upload landed (GPU-side waits)
    hipEvent_t set_done[kPipeSets] = {};  // a chunk set's encode finished (GPU-side waits)
    hipEvent_t dl_done[kPipeSets] = {};   // a chunk set's frames downloaded (GPU-side waits)
    // host waits of the pipelined host-buffer path (the download stream, the end; the chunk sets'
    // own events are set_done above):
    // blocking-sync events, so a waiting thread sleeps instead of spinning on a core the MD5 pool
    // and the other files' threads need (FLACGPU_SPIN_SYNC=1: spinning events, A/B)
    hipEvent_t hw[4] = {nullptr, nullptr, nullptr, nullptr};

    // ---- decision records, kernel timing, clock stamps ----
    fg::FrameRec *d_records = nullptr;
    bool records_on = false;
    bool records_keep = false;  // encode_files with records: every file's records, concatenated
    std::vector<fg::FrameRec> h_records;
    bool timing = false;
    std::vector<fg::TimedLaunch> pending;
    uint64_t launches[FLACGPU_K_COUNT] = {};
    double ms[FLACGPU_K_COUNT] = {};
    unsigned long long *d_stamps = nullptr;

    // ---- MD5 ----
    // streaming MD5 (one stream): a host core by default (FLACGPU_MD5_HOST), or one GPU
    // lane fed by bounded chunks (FLACGPU_MD5_DEVICE, opt-in)
    int md5_engine = FLACGPU_MD5_HOST;
    fg::HostMd5 host_md5;
    uint32_t *d_md5_state = nullptr;
    uint32_t *d_md5_blocks = nullptr;
    uint8_t md5_buf[64] = {};
    uint32_t md5_fill = 0;
    uint64_t md5_len = 0;

    // ---- decoder scratch ----
    DecScratch *dec = nullptr;  // frame decoder / verifier: allocated by the first decode call
    IdxScratch *idx = nullptr;  // device frame index: allocated by the first index call
};

struct flacgpu_plan {
    flacgpu_ctx *ctx = nullptr;
    uint32_t n_streams = 0;
    uint32_t B = 0;
    uint64_t n_frames = 0, n_full = 0, n_tail = 0;
    fg::FrameJob *d_jobs = nullptr;  // full jobs first, then tail jobs
    uint64_t *d_md5_offs = nullptr, *d_md5_lens = nullptr;
    uint8_t *d_md5_fin = nullptr;  // per-stream final-segment flags (NULL: all final)
    uint64_t md5_max_len = 0;      // longest stream segment (bytes): the MD5 chain of one call
    uint64_t max_number = 0;       // largest frame number in the table (u36 check on advance)
    std::vector<uint64_t> first_frame;
    std::vector<uint32_t> full_slots;  // slot of each full job (host copy: ranges of the overlapped encode)
    // host copies of the MD5 segments (the host engine, flacgpu_md5_plan_host)
    std::vector<uint64_t> h_md5_offs, h_md5_lens;
    std::vector<uint8_t> h_md5_fin;  // empty: all final
    uint64_t md5_total = 0;          // bytes of all segments
    uint64_t out_bound = 0;
    uint8_t *d_desc = nullptr;  // per-plan descriptor area when larger than the context's
};

namespace fg {

namespace dec {
struct Args;
struct Result;
}
namespace idx {
struct IdxArgs;
struct IndexResult;
}
namespace streams {
struct Segment;
struct StreamResult;
}
namespace window {
struct PosStream;
struct WindowArg;
struct Cover;
struct WindowResult;
}
namespace deliver {
struct Delivery;
}
namespace resample {
struct Ratio;
}

// shared by the translation units that include this header, not exported from libflacgpu.so
#define FG_LOCAL __attribute__((visibility("hidden")))
// fg_api.cpp
FG_LOCAL hipEvent_t get_event(flacgpu_ctx *c);
// fg_dec_host.cpp: free the decode and index scratch of a context (flacgpu_close)
FG_LOCAL void dec_release(flacgpu_ctx *c);
// fg_misc.hip
hipError_t launch_scan(const uint32_t *sizes, uint64_t *offsets, uint64_t *total, uint32_t n, uint64_t *part,
                       hipStream_t st, const uint64_t *base = nullptr);
// fg_dec.hip
hipError_t launch_dec_parse(const dec::Args &a, hipStream_t st);
hipError_t launch_dec_recon(const dec::Args &a, hipStream_t st);
hipError_t launch_dec_expect(const FrameJob *jobs, uint64_t n, uint64_t *pcm_off, uint64_t *number, uint32_t *ns,
                             hipStream_t st);
// fg_index.hip
hipError_t launch_index(const idx::IdxArgs &g, hipStream_t st);
hipError_t launch_index_streams(const idx::IdxArgs *d_tab, uint32_t n, uint32_t max_groups, uint64_t max_spos,
                                hipStream_t st);
// fg_dec_streams.hip
hipError_t launch_streams_init(const idx::IndexResult *ires, streams::StreamResult *res, uint64_t *carried, uint32_t n,
                               hipStream_t st);
hipError_t launch_streams_gather(const streams::Segment *segs, uint32_t n_segs, const uint64_t *table_first,
                                 const uint64_t *f_off, const uint32_t *f_bytes, uint64_t *p_off, uint32_t *p_bytes,
                                 hipStream_t st);
hipError_t launch_seg_offsets(const streams::Segment *segs, uint32_t n_segs, const uint32_t *blocks, const uint64_t *pcm_base,
                              const uint64_t *pcm_cap, uint64_t *carried, uint32_t per, uint64_t *pcm_off, hipStream_t st);
hipError_t launch_seg_fold(const streams::Segment *segs, uint32_t n_segs, const dec::Result *results,
                           streams::StreamResult *res, hipStream_t st);
hipError_t launch_streams_md5_lens(const streams::StreamResult *res, uint32_t per, uint64_t *lens, uint32_t n, hipStream_t st);
hipError_t launch_streams_md5_mask(const streams::StreamResult *res, uint8_t *digests, uint32_t n, hipStream_t st);
// fg_window.hip
hipError_t launch_positions(const uint8_t *data, const window::PosStream *d_streams, uint32_t n_streams, uint64_t max_cap,
                            const uint64_t *f_off, const uint32_t *f_bytes, const idx::IndexResult *ires, uint64_t *pos,
                            uint64_t *totals, hipStream_t st);
hipError_t launch_window_cover(const window::WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos,
                               const uint64_t *totals, uint32_t unit, uint32_t flags, window::Cover *recs, uint32_t n,
                               hipStream_t st);
hipError_t launch_window_init(const window::Cover *recs, streams::StreamResult *res, uint64_t *carried, uint32_t n,
                              hipStream_t st);
hipError_t launch_window_copy(const window::Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                              const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off, uint32_t per, uint32_t n,
                              uint64_t max_bytes, hipStream_t st);
// k_window_elements<dv.mix>: the delivery as tensor elements, with a channel mix or without
hipError_t launch_window_elements(const window::Cover *recs, const streams::StreamResult *res, const window::WindowArg *args,
                                  const uint8_t *scratch, const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off,
                                  const deliver::Delivery &dv, uint32_t n, uint64_t max_samples, hipStream_t st);
hipError_t launch_window_results(const window::Cover *recs, const streams::StreamResult *res, window::WindowResult *out,
                                 uint32_t n, hipStream_t st);
// fg_resample.hip: the cover and the delivery of windows stated at another sample rate
hipError_t launch_resample_cover(const window::WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos,
                                 const uint64_t *totals, const resample::Ratio &rt, uint32_t unit, uint32_t flags,
                                 window::Cover *recs, uint32_t n, hipStream_t st);
// k_window_resample<dv.mix>: in place of k_window_elements, through the polyphase FIR of rt
hipError_t launch_window_resample(const window::Cover *recs, const streams::StreamResult *res, const window::WindowArg *args,
                                  const uint64_t *totals, const uint8_t *scratch, const uint64_t *src_base, uint8_t *out,
                                  const uint64_t *dst_off, const deliver::Delivery &dv, const resample::Ratio &rt,
                                  const float *coeffs, uint32_t n, uint64_t max_samples, hipStream_t st);
// fg_misc.hip
hipError_t launch_md5_streams(const uint8_t *base, const uint64_t *offs, const uint64_t *lens, const uint8_t *fin,
                              uint32_t n, Md5State *states, uint8_t *digests, hipStream_t st, int kernel, int prio);

struct FG_LOCAL Timed {
    flacgpu_ctx *c;
    int k;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(flacgpu_ctx *c_, int k_, hipStream_t st_) : c(c_), k(k_), st(st_) {
        if (c->timing) {
            a = get_event(c);
            b = get_event(c);
            if (a) hipEventRecord(a, st);
        }
    }
    ~Timed() {
        if (c->timing && a && b) {
            hipEventRecord(b, st);
            c->pending.push_back({k, a, b});
        }
    }
};

FG_LOCAL inline int hip_err(hipError_t e) { return e == hipSuccess ? FLACGPU_OK : (e == hipErrorOutOfMemory ? FLACGPU_ERR_OUT_OF_MEMORY : FLACGPU_ERR_DEVICE); }

// first statement of every entry point that encodes or needs an encode buffer, after its NULL checks
#define FG_ENCODER_ONLY(c)                                        \
    do {                                                          \
        if ((c)->decode_only) return FLACGPU_ERR_INVALID_CONFIG;  \
    } while (0)

#define HIPCHK(x)                               \
    do {                                        \
        hipError_t e_ = (x);                    \
        if (e_ != hipSuccess) return fg::hip_err(e_); \
    } while (0)

// The C ABI's hip_stream: NULL = the context's own stream, FLACGPU_STREAM_LEGACY = the HIP null
// stream (legacy default-stream semantics: the handle-0 stream of a framework), else a hipStream_t.
FG_LOCAL inline hipStream_t pick_stream(const flacgpu_ctx *c, void *hip_stream) {
    if (!hip_stream) return c->stream;
    if (hip_stream == FLACGPU_STREAM_LEGACY) return (hipStream_t)0;
    return (hipStream_t)hip_stream;
}

// The library's grow-only device buffers: p holds cap elements.  Nothing to do where `need` of
// them fit; otherwise the old buffer is freed and one of `need` elements allocated, after *sync has
// drained where work queued on that stream may still use the old one (NULL: the caller knows that
// none does).  On failure p and cap are left {nullptr, 0}.
template <class T, class N>
FG_LOCAL inline hipError_t grow(T *&p, N &cap, uint64_t need, const hipStream_t *sync = nullptr) {
    if (need <= cap) return hipSuccess;
    hipError_t e = sync ? hipStreamSynchronize(*sync) : hipSuccess;
    if (e != hipSuccess) return e;
    hipFree(p);
    p = nullptr;
    cap = 0;
    e = hipMalloc(&p, need * sizeof(T));
    if (e != hipSuccess) {
        p = nullptr;
        return e;
    }
    cap = (N)need;
    return hipSuccess;
}

}  // namespace fg
