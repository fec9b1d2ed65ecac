// fg_ctx.hpp -- the context and plan behind the C ABI's opaque handles, and the small host
// helpers every device-driving translation unit uses: error mapping, stream choice, kernel timing
// brackets.  What they hold is held in the owners of fg_own.hpp.  Private to fg_api.cpp,
// fg_dec_host.cpp and fg_comm.cpp; fg_file.cpp and fg_multi.cpp see a context only through the
// accessors of fg_internal.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "../../include/flacgpu.h"
#include "fg_common.hpp"
#include "fg_geom.hpp"
#include "fg_md5_host.hpp"
#include "fg_own.hpp"

namespace fg {

namespace dec {
struct Result;
struct DecSub;
}

struct FG_LOCAL TimedLaunch {
    int kernel;
    Event start, stop;
};

// What the streams of a context hold.  An encoder's max_block is its block size; a decode-only
// context's is the largest block it accepts.
struct StreamFormat {
    uint32_t channels, bits, bytes_per_sample, sample_rate, max_block;
};

// Everything only an encoder has (flacgpu_open).  Members are destroyed last to first: the buffers,
// then the events, then the streams.
struct FG_LOCAL EncState {
    flacgpu_config cfg{};
    EncGeom g;  // kernel variants, thread counts, LDS and image sizes: enc_geometry(cfg, k)

    // ---- streams and events ----
    Stream aux;
    Stream dl;   // download stream of the pipelined host-buffer path
    Stream up;   // its upload stream (chunk i+1's upload beside chunk i's encode)
    Stream ovl;  // overlapped encode: scan + pack of range i
    Event fork, join;
    // pipelined host-buffer path (encode_pipelined), GPU-side waits
    Event up_done[kPipeSets];   // a chunk set's upload landed
    Event set_done[kPipeSets];  // a chunk set's encode finished
    Event dl_done[kPipeSets];   // a chunk set's frames downloaded
    // host waits of the pipelined host-buffer path (the download stream, the end; the chunk sets'
    // own events are set_done above):
    // blocking-sync events, so a waiting thread sleeps instead of spinning on a core the MD5 pool
    // and the other files' threads need (FLACGPU_SPIN_SYNC=1: spinning events, A/B)
    Event hw[4];

    // ---- encode buffers ----
    DevBuf<uint16_t> d_crc_pow, d_crc_join, d_crc_pow4;
    DevBuf<uint16_t> d_crc_pows;  // CRC fold shifts for the split pack's thread count
    DevBuf<uint16_t> d_crc_powf;  // CRC fold shifts for the fused kernel's 256 threads
    DevBuf<uint16_t> d_crc_x8;    // z^(8 * 2^i) mod P, i < 24
    DevBuf<uint32_t> d_err, d_ctr;
    DevBuf<FrameJob> d_jobs;
    DevBuf<uint8_t> d_desc;
    DevBuf<uint32_t> d_fbytes;
    DevBuf<uint64_t> d_offsets, d_total;
    DevBuf<uint8_t> d_pcm, d_out;
    DevBuf<uint64_t> d_status;  // fused encode: per-slot status words, grow-only
    DevBuf<uint64_t> d_cum;     // [chunk] bytes of the frames before the chunk's slot range
    uint32_t grid_reserve = 0;  // per call: slots the next analysis / pack launches leave free
    // overlapped encode (encode_core): the full frames in `ovl_chunks` ranges, the analysis of
    // range i+1 on the context's stream beside the scan + pack of range i on `ovl`, each grid capped
    // to ovl_ana / ovl_pack workgroups per CU so both are resident on every CU (flacgpu_set_overlap)
    uint32_t ovl_chunks = 0, ovl_ana = 2, ovl_pack = 2, ovl_min_frames = 4096;

    // ---- decision records, clock stamps ----
    DevBuf<FrameRec> d_records;
    bool records_on = false;
    bool records_keep = false;  // encode_files with records: every file's records, concatenated
    std::vector<FrameRec> h_records;
    DevBuf<unsigned long long> d_stamps;

    // ---- the device MD5 engine (FLACGPU_MD5_DEVICE, opt-in): one GPU lane fed by bounded chunks ----
    DevBuf<uint32_t> d_md5_state, d_md5_blocks;
    uint8_t md5_buf[64] = {};
    uint32_t md5_fill = 0;
    uint64_t md5_len = 0;

    // ---- elements to PCM (flacgpu_pcm_from_elements_device): the stream table of a call, grow-only ----
    DevBuf<uint8_t> d_quant;
};

// Decode scratch of a context (allocated by its first decode call, max_frames frames), one
// allocation: the subframe descriptors k_dec_parse leaves for k_dec_recon, the parsed block sizes
// and their scan, the expected frame table of a verify, and a chunk's frame table and results in
// the host-buffer decodes (decode_chunk).  Those decodes' frames and PCM are grow-only.  The feature
// delivery (fg_features.hpp) adds what its first stage leaves for k_features: the windows' extended
// spans as planar F32 (feat_x) and their records and stage-1 results (feat_win), grow-only; the
// filtered delivery (fg_fir.hpp) leaves the same there for k_window_fir.  The
// weighted channel mix (fg_deliver.hpp) adds the weight matrices of the window calls, found again by
// their content (mix_weights: the last kMaxMixWeights of them).
struct FG_LOCAL MixWeights {
    uint32_t rows, cols;
    std::vector<float> host;  // [rows][cols], what the caller passed
    DevBuf<float> dev;        // the same floats
};
constexpr size_t kMaxMixWeights = 16;
struct FG_LOCAL DecScratch {
    DevBuf<uint8_t> buf;
    uint64_t *samp_off, *total, *exp_off, *exp_number, *d_foff;
    dec::Result *d_results;
    dec::DecSub *subs;
    uint32_t *blocks, *body, *exp_n, *d_fbytes, *ctl, *d_bad;  // ctl: [0] ticket
    DevBuf<uint8_t> d_frames, d_pcm;
    DevBuf<float> feat_x;
    DevBuf<uint8_t> feat_win;
    std::vector<MixWeights> mix_weights;
};

// Index scratch of a context, grow-only: the arrays of idx::IdxArgs, sized from the call's len and
// cap (buf); and the frame table and result of the whole-file decode, which indexes the file it
// uploaded (table).  The many-streams decode adds the packed frame table with the per-stream arrays
// and segment table of a call (packed), and the per-file results and digests of
// flacgpu_decode_files (files).  The window decode adds the stream table of a positions call (pos),
// the windows of a call as the caller states them with their cover records (win_in), what the chunk
// loop over the covering frames needs (win), those frames' PCM (win_pcm), and the delivered bytes
// and results of flacgpu_decode_files_windows (win_out).  The resampled delivery adds the
// coefficient tables of the ratios it has served, kept until the context is closed (tables).  The
// feature delivery adds, in k_features' operand layout, the STFT tables of the n_fft it has served
// (feat_tables, kept as the resampler's) and the filter banks, found again by their content
// (feat_filters: the last kMaxFeatFilters of them).
struct FG_LOCAL ResampleTable {
    uint32_t L, M;
    DevBuf<float> coeffs;  // L rows of T
};
struct FG_LOCAL FeatTable {
    uint32_t n_fft;
    DevBuf<float> blocks;
};
struct FG_LOCAL FeatFilter {
    uint32_t rows, bins;
    std::vector<float> host;  // [rows][bins], what the caller passed
    DevBuf<float> blocks;
};
constexpr size_t kMaxFeatFilters = 16;
struct FG_LOCAL IdxScratch {
    DevBuf<uint8_t> buf, table, packed, files, pos, win_in, win, win_pcm, win_out;
    std::vector<ResampleTable> tables;
    std::vector<FeatTable> feat_tables;
    std::vector<FeatFilter> feat_filters;
};

}  // namespace fg

// A context: the shared part, which is all the decode layer reads, and three parts that are there
// or not -- `enc` on an encoder (decode-only: !enc), `dec` and `idx` once a decode or index call
// has needed them.  flacgpu_close deletes the context and the owners release everything.  Members
// are destroyed last to first, so the order of declaration is the teardown order read upwards: the
// three parts (each its buffers, then its events, then its streams), d_scan_part, the timing events
// and the event pool, and the context's own stream last.
struct FG_LOCAL flacgpu_ctx {
    int device = 0;
    fg::StreamFormat fmt{};
    uint32_t max_frames = 0;
    fg::Knobs k;  // the environment's knobs when the context was opened
    fg::Stream stream;
    std::vector<fg::Event> event_pool;
    // kernel timing
    bool timing = false;
    std::vector<fg::TimedLaunch> pending;
    uint64_t launches[FLACGPU_K_COUNT] = {};
    double ms[FLACGPU_K_COUNT] = {};
    // streaming MD5 (one stream): a host core by default (FLACGPU_MD5_HOST), or EncState's device engine
    int md5_engine = FLACGPU_MD5_HOST;
    fg::HostMd5 host_md5;
    int md5_kernel = 1;  // the batched stream MD5 (plans, decoded streams): EncGeom::md5_kernel's rule
    fg::DevBuf<uint64_t> d_scan_part;  // per-4096-frame block sums of the multi-workgroup scan, grow-only

    std::unique_ptr<fg::EncState> enc;    // flacgpu_open; NULL on a decode-only context (flacgpu_open_decoder)
    std::unique_ptr<fg::DecScratch> dec;  // frame decoder / verifier: allocated by the first decode call
    std::unique_ptr<fg::IdxScratch> idx;  // device frame index: allocated by the first index call
};

struct FG_LOCAL flacgpu_plan {
    flacgpu_ctx *ctx = nullptr;
    uint32_t n_streams = 0;
    uint32_t B = 0;
    uint64_t n_frames = 0, n_full = 0, n_tail = 0;
    fg::DevBuf<fg::FrameJob> d_jobs;  // full jobs first, then tail jobs
    fg::DevBuf<uint64_t> d_md5_offs, d_md5_lens;
    fg::DevBuf<uint8_t> d_md5_fin;  // per-stream final-segment flags (empty: all final)
    uint64_t md5_max_len = 0;       // longest stream segment (bytes): the MD5 chain of one call
    uint64_t max_number = 0;        // largest frame number in the table (u36 check on advance)
    std::vector<uint64_t> first_frame;
    std::vector<uint32_t> full_slots;  // slot of each full job (host copy: ranges of the overlapped encode)
    // host copies of the MD5 segments (the host engine, flacgpu_md5_plan_host)
    std::vector<uint64_t> h_md5_offs, h_md5_lens;
    std::vector<uint8_t> h_md5_fin;  // empty: all final
    uint64_t md5_total = 0;          // bytes of all segments
    uint64_t out_bound = 0;
    fg::DevBuf<uint8_t> d_desc;  // per-plan descriptor area when larger than the context's
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
namespace feat {
struct Params;
}
namespace quantize {
struct Stream;
}
struct FeatWindow;
struct FirWindow;

// fg_api.cpp: an event of the context's pool, or a new one (empty: none could be created)
FG_LOCAL Event get_event(flacgpu_ctx *c);
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
                               const uint64_t *totals, uint32_t unit, uint32_t flags, uint32_t hop, window::Cover *recs,
                               uint32_t n, hipStream_t st);
hipError_t launch_window_init(const window::Cover *recs, streams::StreamResult *res, uint64_t *carried, uint32_t n,
                              hipStream_t st);
hipError_t launch_window_copy(const window::Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                              const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off, uint32_t per, uint32_t n,
                              uint64_t max_bytes, hipStream_t st);
// k_window_elements<dv.mix>: the delivery as tensor elements, without a channel mix, with masks or with weights
hipError_t launch_window_elements(const window::Cover *recs, const streams::StreamResult *res, const window::WindowArg *args,
                                  const uint8_t *scratch, const uint64_t *src_base, uint8_t *out, const uint64_t *dst_off,
                                  const deliver::Delivery &dv, uint32_t n, uint64_t max_samples, hipStream_t st);
hipError_t launch_window_results(const window::Cover *recs, const streams::StreamResult *res, window::WindowResult *out,
                                 uint32_t n, hipStream_t st);
// fg_levels.hip: k_window_levels in place of k_window_copy, then k_levels_fold where blocks have several parts
hipError_t launch_window_levels(const window::Cover *recs, const streams::StreamResult *res, const uint8_t *scratch,
                                const uint64_t *src_base, const uint64_t *dst_off, const uint64_t *part_base, void *parts,
                                uint32_t *peak, int64_t *sum, double *energy, uint32_t hop, uint32_t C, uint32_t B, uint32_t n,
                                uint64_t max_samples, hipStream_t st);
// fg_resample.hip: the cover and the delivery of windows stated at another sample rate
hipError_t launch_resample_cover(const window::WindowArg *args, const idx::IndexResult *ires, const uint64_t *pos,
                                 const uint64_t *totals, const resample::Ratio &rt, uint32_t unit, uint32_t flags,
                                 window::Cover *recs, uint32_t n, hipStream_t st);
// k_window_resample<dv.mix>: in place of k_window_elements, through the polyphase FIR of rt
hipError_t launch_window_resample(const window::Cover *recs, const streams::StreamResult *res, const window::WindowArg *args,
                                  const uint64_t *totals, const uint8_t *scratch, const uint64_t *src_base, uint8_t *out,
                                  const uint64_t *dst_off, const deliver::Delivery &dv, const resample::Ratio &rt,
                                  const float *coeffs, uint32_t n, uint64_t max_samples, hipStream_t st);
// fg_features.hip: stage 2 of the feature delivery, over the planar F32 spans stage 1 left in x
hipError_t launch_features(const FeatWindow *wins, const window::WindowResult *stage1, const uint64_t *totals,
                           const resample::Ratio &rt, const float *x, const float *table, const float *filters, uint8_t *out,
                           window::WindowResult *results, const feat::Params &ft, uint32_t K, uint32_t format, uint32_t n,
                           uint64_t max_items, hipStream_t st);
// fg_fir.hip: stage 2 of the filtered delivery, over the planar F32 spans stage 1 left in x
hipError_t launch_window_fir(const FirWindow *wins, const window::WindowResult *stage1, const uint64_t *totals,
                             const resample::Ratio &rt, const float *x, const float *taps, uint8_t *out,
                             window::WindowResult *results, uint32_t K, uint32_t format, uint32_t flags, uint32_t n,
                             uint64_t max_items, hipStream_t st);
// fg_quantize.hip: k_elements_pcm<B> over a device table of n_streams quantize::Stream rows
hipError_t launch_elements_pcm(const quantize::Stream *d_tab, uint32_t n_streams, uint64_t max_units, uint8_t *d_pcm,
                               uint64_t *d_clipped, uint32_t C, uint32_t B, uint32_t format, bool planar, hipStream_t st);
// fg_misc.hip
hipError_t launch_md5_streams(const uint8_t *base, const uint64_t *offs, const uint64_t *lens, const uint8_t *fin,
                              uint32_t n, Md5State *states, uint8_t *digests, hipStream_t st, int kernel, int prio);

struct FG_LOCAL Timed {
    flacgpu_ctx *c;
    int k;
    hipStream_t st;
    Event a, b;
    Timed(flacgpu_ctx *c_, int k_, hipStream_t st_) : c(c_), k(k_), st(st_) {
        if (c->timing) {
            a = get_event(c);
            b = get_event(c);
            if (a) hipEventRecord(a.get(), st);
        }
    }
    ~Timed() {
        if (c->timing && a && b) {
            hipEventRecord(b.get(), st);
            c->pending.push_back({k, std::move(a), std::move(b)});
        }
    }
};

FG_LOCAL inline int hip_err(hipError_t e) { return e == hipSuccess ? FLACGPU_OK : (e == hipErrorOutOfMemory ? FLACGPU_ERR_OUT_OF_MEMORY : FLACGPU_ERR_DEVICE); }

// first statement of every entry point that encodes or needs an encode buffer, after its NULL checks
#define FG_ENCODER_ONLY(c)                                        \
    do {                                                          \
        if (!(c)->enc) return FLACGPU_ERR_INVALID_CONFIG;      \
    } while (0)

#define HIPCHK(x)                               \
    do {                                        \
        hipError_t e_ = (x);                    \
        if (e_ != hipSuccess) return fg::hip_err(e_); \
    } while (0)

// The C ABI's hip_stream: NULL = the context's own stream, FLACGPU_STREAM_LEGACY = the HIP null
// stream (legacy default-stream semantics: the handle-0 stream of a framework), else a hipStream_t.
FG_LOCAL inline hipStream_t pick_stream(const flacgpu_ctx *c, void *hip_stream) {
    if (!hip_stream) return c->stream.get();
    if (hip_stream == FLACGPU_STREAM_LEGACY) return (hipStream_t)0;
    return (hipStream_t)hip_stream;
}

}  // namespace fg
