/*
 * flacgpu.h -- C ABI of libflacgpu.so, the MI355X (gfx950) FLAC block encoder.
 *
 * Drop-in boundary for toastori/zig-flac's per-block encode path
 * (reference: src/lib.zig re-exports; the hot call is Encoder.writeFrame,
 * src/lib/encoder.zig:234-284).  Plain pointers and sizes only; no torch or
 * HIP types in any signature except the opaque `void *hip_stream` of the
 * device-resident entry points.  Each entry point cites the reference
 * interface it replaces.  The Zig `extern` declarations a maintainer adds to
 * the reference are in INTEGRATION.md.
 *
 * Output bytes are identical to the reference encoder's for the same input
 * (see DESIGN.md for the parity evidence and the one documented divergence,
 * a reference undefined-behaviour case).
 *
 * Threading: one context per GPU per host thread; a context is not
 * thread-safe.  All functions return FLACGPU_OK (0) or a negative error code.
 *
 * Streams: `void *hip_stream` is a hipStream_t, except two values: NULL selects
 * the context's own (non-blocking) stream, and FLACGPU_STREAM_LEGACY selects the
 * HIP null stream (legacy default-stream semantics), which orders the work
 * against default-stream producers and consumers (e.g. a framework whose
 * current stream handle is 0).
 */
#ifndef FLACGPU_H
#define FLACGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLACGPU_ABI_VERSION 5

/* the HIP null (legacy default) stream as a hip_stream argument */
#define FLACGPU_STREAM_LEGACY ((void *)1)

/* Error codes (map to the Zig error set
 * {OutOfMemory, WriteFailed, DeviceError, InvalidConfig, InvalidInput}). */
enum {
    FLACGPU_OK = 0,
    FLACGPU_ERR_INVALID_CONFIG = -1, /* Config outside what the reference accepts */
    FLACGPU_ERR_INVALID_INPUT = -2,  /* bad pointer / size / alignment */
    FLACGPU_ERR_OUT_OF_MEMORY = -3,  /* Allocator.Error.OutOfMemory (encoder.zig:48) */
    FLACGPU_ERR_OUTPUT_TOO_SMALL = -4, /* Writer.Error.WriteFailed analogue */
    FLACGPU_ERR_DEVICE = -5,         /* HIP runtime failure or no gfx950 device */
    FLACGPU_ERR_INTERNAL = -6        /* device-side invariant violated */
};

/* Encoder.Config + Config.Feature (encoder.zig:609-656) and the per-frame
 * FrameInfo fields that are constant over a stream (encoder.zig:658-663). */
typedef struct {
    uint32_t sample_rate;          /* FrameInfo.sample_rate (u20) */
    uint16_t block_size;           /* Config.block_size: 1..4096 (default 4096, encoder.zig:644) */
    uint8_t channels;              /* 1..8 */
    uint8_t bits_per_sample;       /* 8, 16, 24 or 32 (frame_writer.zig:221-233) */
    uint8_t stereo_decorrelation;  /* Feature.stereo_decorrelation (default 1) */
    uint8_t max_rice_part_order;   /* Feature.max_rice_order, 0..8 (default 8) */
    uint8_t max_rice_param;        /* Feature.max_rice_param, 1..30 (default 30) */
    uint8_t prediction;            /* Feature.prediction: 0 = fixed (the only value the
                                      reference implements; it never reads the field).
                                      Build-defined extension: 1..12 = also search LPC
                                      orders 1..prediction (DESIGN.md "LPC") */
} flacgpu_config;

/* Config.default(channels, bit_depth) (encoder.zig:642-655). */
flacgpu_config flacgpu_config_default(uint32_t channels, uint32_t bits_per_sample, uint32_t sample_rate);

typedef struct flacgpu_ctx flacgpu_ctx;

/* Encoder.init (encoder.zig:44-118): allocates all device scratch up front
 * for up to `max_frames_per_call` frames per call (0 = 32768).  device is the
 * HIP ordinal. */
int flacgpu_open(int device, const flacgpu_config *cfg, uint32_t max_frames_per_call, flacgpu_ctx **out);
/* Encoder.deinit (encoder.zig:121-164). */
void flacgpu_close(flacgpu_ctx *ctx);

const char *flacgpu_strerror(int code);
int flacgpu_abi_version(void);

/* How this libflacgpu.so was built (no reference counterpart: library introspection).
 * FLACGPU_BUILD_DIAG: a diagnostic build (`make diag`) with the measured-slower alternative
 * kernels / schedules and the diagnostic environment knobs compiled in; the release build has
 * none of them.  FLACGPU_BUILD_STAMPS: per-phase clock stamps (-DFG_STAMPS). */
#define FLACGPU_BUILD_DIAG 1u
#define FLACGPU_BUILD_STAMPS 2u
uint32_t flacgpu_build_flags(void);

/* maxFrameBytes (encoder.zig:583-595) of the reference, and the tight bound
 * the GPU path uses for its per-frame LDS image. */
size_t flacgpu_reference_max_frame_bytes(const flacgpu_config *cfg);
size_t flacgpu_frame_bound_bytes(const flacgpu_config *cfg);

/* ---- Host-buffer entry points (synchronous) ---------------------------- */

/* Batched Encoder.writeFrame (encoder.zig:234) driven the way wav2flac.encode
 * drives it (wav2flac.zig:66-97): `pcm` holds n_samples interleaved
 * little-endian samples of bytes_per_sample (= bits/8) bytes, exactly as a WAV
 * data chunk stores them (WavReader.fillSamples, wav_reader.zig:44-91).  Frames
 * of cfg.block_size samples are numbered from first_frame_number; the last
 * one may be short.  Writes the concatenated frames to out[0..*out_len) and
 * the per-frame byte counts (the u24 writeFrame returns) to frame_bytes[],
 * in frame order.  As in the reference, the caller drives the MD5
 * separately (flacgpu_md5_update with the same bytes). */
int flacgpu_encode_frames(flacgpu_ctx *ctx, const void *pcm, uint32_t bytes_per_sample, uint64_t n_samples,
                          uint64_t first_frame_number, uint8_t *out, size_t out_cap, size_t *out_len,
                          uint32_t *frame_bytes);

/* ---- Multi-GPU host-buffer encode (SURVEY.md §8(b) "flacgpu_open_multi") --
 * One process, n_devices contexts (device ordinals may repeat).  A call shards
 * the input's frames into contiguous ranges, one per context, encodes them
 * concurrently (one host thread per context, each with its own PCIe link) and
 * concatenates the frames in frame order into out -- the bitstream
 * concatenation step of the multi-rank path, done in host memory because the
 * caller's output already lives there.  Same arguments, errors and output as
 * flacgpu_encode_frames (byte-identical to one context encoding it all). */
typedef struct flacgpu_multi flacgpu_multi;
int flacgpu_open_multi(int n_devices, const int *devices, const flacgpu_config *cfg, uint32_t max_frames_per_call,
                       flacgpu_multi **out);
void flacgpu_close_multi(flacgpu_multi *m);
int flacgpu_multi_encode_frames(flacgpu_multi *m, const void *pcm, uint32_t bytes_per_sample, uint64_t n_samples,
                                uint64_t first_frame_number, uint8_t *out, size_t out_cap, size_t *out_len,
                                uint32_t *frame_bytes);

/* ---- Multi-rank encode: one process per GPU, RCCL over xGMI (SURVEY.md §8(b)
 *      "flacgpu_open_multi ... shards frames and gathers via RCCL", §8(e); BASELINE
 *      config 4) -----------------------------------------------------------------
 * The sharded form of wav2flac's block loop (wav2flac.zig:66-97): frame f of a
 * stream depends only on its samples and its number (encoder.zig:234-284), so the
 * ranks encode disjoint frames, and the only exchange is the gather of the
 * variable-length bitstreams and the per-frame sizes (the u24 writeFrame returns,
 * replayed by updateFrameSize in frame order, metadata.zig:35-40) to rank 0.
 * librccl.so.1 is loaded on first use (an RCCL already in the process, e.g. a
 * framework's, is reused; else /opt/rocm/lib); without it these return
 * FLACGPU_ERR_DEVICE.  Every call below is collective: every rank of the
 * communicator makes it, in the same order.  A communicator is used by one host
 * thread at a time (as a flacgpu_ctx is): its count buffers are per communicator. */
typedef struct flacgpu_comm flacgpu_comm;
#define FLACGPU_COMM_ID_BYTES 128
/* Rank 0 creates the communicator id; the host hands it to every rank (a file,
 * a socket, torch.distributed's store: any channel).  No GPU work. */
int flacgpu_comm_unique_id(uint8_t id[FLACGPU_COMM_ID_BYTES]);
/* Join the communicator as `rank` of `world` on HIP device `device` (one rank
 * per GPU: RCCL rejects two ranks on one device). */
int flacgpu_comm_init(const uint8_t id[FLACGPU_COMM_ID_BYTES], int world, int rank, int device,
                      flacgpu_comm **out);
void flacgpu_comm_destroy(flacgpu_comm *comm);
int flacgpu_comm_rank(const flacgpu_comm *comm);
int flacgpu_comm_size(const flacgpu_comm *comm);

/* Gather every rank's device-resident frames to rank 0, in rank order, into ONE
 * device buffer (xGMI point-to-point; nothing crosses PCIe).  Each rank gives its
 * n_frames frames: d_frames (device) holding nbytes valid bytes -- or, if
 * d_nbytes is non-NULL, the count in device memory (a u64, e.g. the d_total of
 * flacgpu_encode_plan_device_ex, read without a separate host sync) -- and
 * d_sizes (device u32 per frame).  Rank 0 passes d_recv (capacity recv_cap
 * bytes) and d_recv_sizes (capacity recv_sizes_cap entries); rank 0's own frames
 * are copied to their head unless d_frames == d_recv (encoded in place).  Every
 * rank gets *total_bytes / *total_frames (NULL: not wanted) = the gathered
 * totals.  Queued on hip_stream (NULL: the HIP null stream) and synchronised
 * with it once (the counts are read on the host to size the transfers).  If
 * rank 0's capacities are too small, EVERY rank returns
 * FLACGPU_ERR_OUTPUT_TOO_SMALL and nothing is transferred. */
int flacgpu_gather_frames_device(flacgpu_comm *comm, const uint8_t *d_frames, uint64_t nbytes, const uint64_t *d_nbytes,
                                 const uint32_t *d_sizes, uint64_t n_frames, uint8_t *d_recv, uint64_t recv_cap,
                                 uint32_t *d_recv_sizes, uint64_t recv_sizes_cap, uint64_t *total_bytes,
                                 uint64_t *total_frames, void *hip_stream);

/* flacgpu_encode_frames across the ranks of comm: every rank passes the SAME
 * arguments (pcm = the whole stream in host memory, e.g. each rank's mmap of the
 * WAV data chunk; n_samples; first_frame_number).  The frames are cut into
 * windows of world x max_frames_per_call frames; rank r encodes the r-th slice of
 * every window on its GPU, and each window's frames are gathered to rank 0's GPU
 * over RCCL and appended to rank 0's out (frame order).  Rank 0 gets exactly the
 * bytes and frame sizes flacgpu_encode_frames would write for the whole input;
 * other ranks get *out_len = 0 (out / frame_bytes unused, may be NULL).  A failure
 * on any rank is returned by every rank.  ctx must be open on comm's device with
 * the same config on every rank. */
int flacgpu_encode_frames_sharded(flacgpu_ctx *ctx, flacgpu_comm *comm, const void *pcm, uint32_t bytes_per_sample,
                                  uint64_t n_samples, uint64_t first_frame_number, uint8_t *out, size_t out_cap,
                                  size_t *out_len, uint32_t *frame_bytes);

/* Encoder.writeFrame for one frame, exactly the reference call: the caller
 * provides planar i32 samples (the reference's Encoder.samples[ch][0..n],
 * encoder.zig:23, each within bits_per_sample signed range), the frame number
 * (u36) and n = FrameInfo.samples_count (1..block_size).  Writes the frame to
 * out and its size to *frame_bytes. */
int flacgpu_encode_frame_planar(flacgpu_ctx *ctx, const int32_t *const planes[8], uint32_t n,
                                uint64_t frame_number, uint8_t *out, size_t out_cap, uint32_t *frame_bytes);

/* ---- Streaming MD5 (md5.zig, fed by wav_reader.zig:66; finalised by
 *      Encoder.finalizeStreamInfoMd5, encoder.zig:168-170) -------------------
 * One stream's MD5 is a strictly sequential chain.  The default engine hashes
 * on a host core (about 10x one GPU lane's rate, and the bytes are already in
 * host memory on this path); FLACGPU_MD5_DEVICE runs the chain on one GPU
 * lane (opt-in; the device-resident plans below hash many streams at once, one
 * lane per stream).  set_engine resets the running hash. */
enum { FLACGPU_MD5_HOST = 0, FLACGPU_MD5_DEVICE = 1 };
int flacgpu_md5_set_engine(flacgpu_ctx *ctx, int engine);
int flacgpu_md5_get_engine(const flacgpu_ctx *ctx);
int flacgpu_md5_init(flacgpu_ctx *ctx);
int flacgpu_md5_update(flacgpu_ctx *ctx, const void *data, size_t len);
int flacgpu_md5_final(flacgpu_ctx *ctx, uint8_t digest[16]);

/* ---- Device-resident entry points (asynchronous on hip_stream) --------- */

/* A plan describes a batch of independent streams (files) laid out in one
 * device PCM buffer: stream s holds stream_samples[s] interleaved samples
 * starting at byte offset stream_offsets[s] (4-byte aligned).  Frames of
 * every stream are numbered from 0.  The plan precomputes the frame table
 * (device memory) so repeated calls launch no host work. */
typedef struct flacgpu_plan flacgpu_plan;
int flacgpu_plan_create(flacgpu_ctx *ctx, uint32_t n_streams, const uint64_t *stream_offsets,
                        const uint64_t *stream_samples, uint32_t bytes_per_sample, flacgpu_plan **out);
void flacgpu_plan_destroy(flacgpu_plan *plan);
uint64_t flacgpu_plan_frames(const flacgpu_plan *plan);
/* Bytes of device output capacity the plan may need (sum of frame bounds). */
uint64_t flacgpu_plan_out_bound(const flacgpu_plan *plan);
/* First frame index of stream s inside the plan's frame table. */
uint64_t flacgpu_plan_stream_first_frame(const flacgpu_plan *plan, uint32_t s);

/* A plan whose streams are SEGMENTS of longer streams (a stream spans several
 * batches, as the reference's block loop spans a whole file, wav2flac.zig:66-97):
 * stream s's frames are numbered from first_frame_numbers[s] (NULL: 0) and
 * final_segment[s] == 0 marks a segment the stream continues after (NULL: every
 * segment final).  A non-final segment must hold whole frames of block_size
 * samples and a whole number of 64-byte MD5 blocks (always true at 4096). */
int flacgpu_plan_create_segments(flacgpu_ctx *ctx, uint32_t n_streams, const uint64_t *stream_offsets,
                                 const uint64_t *stream_samples, uint32_t bytes_per_sample,
                                 const uint64_t *first_frame_numbers, const uint8_t *final_segment,
                                 flacgpu_plan **out);
/* Move every frame number of the plan on by `frames`, queued on hip_stream: the
 * next window of the same streams at the same device offsets (a ring buffer the
 * caller refills).  Frame numbers stay u36. */
int flacgpu_plan_advance(flacgpu_plan *plan, uint64_t frames, void *hip_stream);

/* Per-stream MD5 chaining state carried from one call to the next (device
 * memory, 32 bytes per stream; initialise with flacgpu_md5_state_init and copy
 * to the device). */
typedef struct {
    uint32_t h[4];      /* MD5 chaining value */
    uint64_t bytes;     /* message bytes absorbed */
    uint32_t finished;  /* 1 once the final segment has been padded: h is then the digest, and
                           later calls leave the state unchanged (a final segment passed again
                           reports the same digest); re-initialise it to start a new stream */
    uint32_t reserved;
} flacgpu_md5_state;
void flacgpu_md5_state_init(flacgpu_md5_state *states, size_t n);

/* Encode every frame of the plan from device PCM d_pcm into the contiguous
 * device buffer d_out (capacity out_cap).  Per frame: d_frame_bytes[f] (u32)
 * and d_frame_offsets[f] (u64 byte offset of frame f in d_out; stream s's
 * bitstream is the contiguous range starting at its first frame's offset).
 * d_total (u64) receives the total byte count.  If d_md5 is non-NULL, the MD5
 * of every stream's raw PCM bytes is computed on the GPU into d_md5[16*s].
 * Nothing is synchronised; all work is queued on hip_stream (NULL = the
 * context's own stream). */
int flacgpu_encode_plan_device(flacgpu_ctx *ctx, const flacgpu_plan *plan, const void *d_pcm, uint8_t *d_out,
                               uint64_t out_cap, uint32_t *d_frame_bytes, uint64_t *d_frame_offsets,
                               uint64_t *d_total, uint8_t *d_md5, void *hip_stream);

/* As flacgpu_encode_plan_device, but the MD5 of the streams is queued on
 * md5_stream (after the PCM is ready on hip_stream) and NOT joined back into
 * hip_stream: the encode of the next batch can start while this batch's MD5
 * chains finish (the MD5 is per-stream sequential and latency-bound, the
 * encode is throughput-bound, so consecutive batches overlap).  The caller
 * synchronises md5_stream before reading d_md5 or reusing d_pcm.
 * md5_stream == NULL behaves exactly like flacgpu_encode_plan_device. */
int flacgpu_encode_plan_device_md5_async(flacgpu_ctx *ctx, const flacgpu_plan *plan, const void *d_pcm,
                                         uint8_t *d_out, uint64_t out_cap, uint32_t *d_frame_bytes,
                                         uint64_t *d_frame_offsets, uint64_t *d_total, uint8_t *d_md5,
                                         void *hip_stream, void *md5_stream);

/* flacgpu_encode_plan_device with carried MD5 state: if d_md5_state is non-NULL,
 * each stream's state is read, advanced by its segment and written back (the
 * MD5 of a stream spanning many calls); segments marked final are padded and
 * their digest written to d_md5[16 s] (if non-NULL).  With d_md5_state NULL every
 * segment must be final (fresh state, digest to d_md5).  md5_stream as in
 * flacgpu_encode_plan_device_md5_async (NULL: joined into hip_stream). */
int flacgpu_encode_plan_device_ex(flacgpu_ctx *ctx, const flacgpu_plan *plan, const void *d_pcm, uint8_t *d_out,
                                  uint64_t out_cap, uint32_t *d_frame_bytes, uint64_t *d_frame_offsets,
                                  uint64_t *d_total, flacgpu_md5_state *d_md5_state, uint8_t *d_md5,
                                  void *hip_stream, void *md5_stream);

/* The host engine of the same MD5 (md5.zig:3-31 over the bytes wav_reader.zig:66
 * feeds it; finalised as Encoder.finalizeStreamInfoMd5, encoder.zig:168-170).
 * flacgpu_md5_many advances n independent chains on the library's host hashing
 * pool: chain i absorbs lens[i] bytes at data[i] from states[i] (host memory,
 * the layout and `finished` rules of the device path above, so a stream's state
 * may pass between the engines from one call to the next); final[i] != 0 (final
 * NULL: every chain) pads the chain and writes its digest to digests[16 i] (if
 * non-NULL).  states NULL: fresh chains, all final.  A chain that continues
 * after the call must absorb whole 64-byte blocks.  Needs no GPU; blocks. */
int flacgpu_md5_many(uint32_t n, const void *const *data, const uint64_t *lens, const uint8_t *final,
                     flacgpu_md5_state *states, uint8_t *digests);
/* flacgpu_md5_many over every segment of `plan`, read from h_pcm, a host copy
 * of the device PCM buffer (same offsets), with the plan's final flags.  Run it
 * on a host thread beside flacgpu_encode_plan_device_ex called with
 * d_md5_state = d_md5 = NULL: few long streams then hash at host-core speed
 * instead of one GPU lane each. */
int flacgpu_md5_plan_host(const flacgpu_plan *plan, const void *h_pcm, flacgpu_md5_state *states, uint8_t *digests);
/* The faster MD5 engine for this plan's segments: FLACGPU_MD5_HOST below the
 * stream-count crossover (a few long chains), FLACGPU_MD5_DEVICE above it:
 * flacgpu_md5_engine_for(plan's stream count, longest segment, total bytes). */
int flacgpu_plan_md5_engine(const flacgpu_plan *plan);

/* The rates the engine choice is priced with (no reference
 * counterpart: the reference hashes on its one thread).  host_chain[i]: bytes/s
 * per pool worker when every worker holds host_chains[i] chains (1, 2, 3, 4 for the
 * scalar interleave; 1, 4, 8, 16 where the host has AVX-512), MEASURED on this
 * machine by running the pool the first time they are needed
 * (flacgpu_md5_get_rates); host_workers: the pool's size (0: no pool, host_chain
 * is one chain on the caller); device_lane / device_chip: bytes/s of one stream's
 * GPU lane beside the encode and of all lanes together (MI355X measurements). */
typedef struct {
    double host_chain[4];
    uint32_t host_chains[4]; /* chains per worker of each host_chain entry (0s: 1, 2, 3, 4) */
    double device_lane;
    double device_chip;
    int32_t host_workers;
    int32_t measured; /* 1: host_chain measured in this process; 2: set by the caller; 3: measured while
                         other chains were hashing on the pool (possibly low: set_rates(NULL) re-measures) */
} flacgpu_md5_rates;
/* The current rates (measures the host ones on first use, ~2 ms).  Needs no GPU. */
int flacgpu_md5_get_rates(flacgpu_md5_rates *out);
/* Replace the rates (NULL: measure again); e.g. a caller's own measurement. */
int flacgpu_md5_set_rates(const flacgpu_md5_rates *rates);
/* The engine the rates predict faster for n_streams chains of at most max_len
 * bytes, total_len bytes in all: host time = total / (pool throughput at
 * ceil(n / workers) chains per worker, interpolated between the measured points
 * and flat past the last: time-sliced), device time =
 * max(max_len / device_lane, total / device_chip).  Needs no GPU. */
int flacgpu_md5_engine_for(uint32_t n_streams, uint64_t max_len, uint64_t total_len);

/* Synchronise hip_stream (NULL: the context's stream) and report the device-side
 * error word of the kernels queued so far (FLACGPU_ERR_OUTPUT_TOO_SMALL when a
 * frame would not fit out_cap, FLACGPU_ERR_INTERNAL on a violated invariant);
 * clears it.  The device-resident entry points are asynchronous: this is how
 * their caller learns of a failure. */
int flacgpu_sync_check(flacgpu_ctx *ctx, void *hip_stream);

/* ---- File level (host code around the GPU frame path) --------------------- */

/* The context's configuration (what flacgpu_open was given). */
int flacgpu_get_config(const flacgpu_ctx *ctx, flacgpu_config *out);

/* WavReader.init / getFmt (wav_reader.zig:116-170) and the flacStreaminfo checks
 * (wav_reader.zig:92-108) on an in-memory WAV file: the PCM data chunk starts at
 * data_offset; samples = data_len / (channels * (bits/8)) as in wav_reader.zig:169. */
typedef struct {
    uint32_t sample_rate;
    uint16_t channels;
    uint16_t bits_per_sample;   /* valid bits (EXTENSIBLE) or the fmt bit depth */
    uint16_t bytes_per_sample;  /* block_align / channels */
    uint16_t pad;
    uint64_t samples;           /* interchannel samples */
    uint64_t data_offset;
    uint64_t data_bytes;
} flacgpu_wav_info;
int flacgpu_wav_parse(const void *wav, size_t len, flacgpu_wav_info *info);

/* StreamInfo (metadata.zig:18-68). */
typedef struct {
    uint8_t md5[16];
    uint64_t interchannel_samples;
    uint32_t min_frame_size;    /* u24; starts at 0xFFFFFF */
    uint32_t max_frame_size;    /* u24; starts at 0 */
    uint32_t sample_rate;
    uint16_t min_block_size;
    uint16_t max_block_size;
    uint8_t channels;
    uint8_t bit_depth;
    uint8_t pad[6];
} flacgpu_streaminfo;
void flacgpu_streaminfo_init(flacgpu_streaminfo *si, uint32_t sample_rate, uint32_t channels, uint32_t bit_depth,
                             uint64_t interchannel_samples, uint32_t block_size);
/* StreamInfo.updateFrameSize (metadata.zig:35-40), with its else-if. */
void flacgpu_streaminfo_update_frame_size(flacgpu_streaminfo *si, uint32_t frame_size);
/* StreamInfo.updateFrameSize replayed over n_frames device-resident frame sizes in frame
 * order (metadata.zig:35-40, the caller's loop at wav2flac.zig:94): d_minmax (device, u32[2])
 * holds {min_frame_size, max_frame_size} on entry (0xFFFFFF, 0 for a new stream, or the
 * state after earlier windows) and on exit, with the reference's else-if quirk: a frame that
 * raises the running max never lowers the min.  One workgroup, queued on hip_stream; the
 * bitstream of a sharded encode never leaves HBM for its STREAMINFO. */
int flacgpu_streaminfo_replay_device(flacgpu_ctx *ctx, const uint32_t *d_frame_bytes, uint64_t n_frames,
                                     uint32_t *d_minmax, void *hip_stream);
/* StreamInfo.bytes (metadata.zig:42-68). */
void flacgpu_streaminfo_bytes(const flacgpu_streaminfo *si, uint8_t out[34]);
/* Encoder.writeHeader (encoder.zig:192-206): "fLaC" + STREAMINFO block; returns 42. */
size_t flacgpu_header_bytes(const flacgpu_streaminfo *si, int last_metadata, uint8_t out[42]);
/* Encoder.writeVorbisComment (encoder.zig:211-226): vendor "toastori FLAC 0.0.0", no tags; returns 31. */
size_t flacgpu_vorbis_comment_bytes(int last_metadata, uint8_t out[31]);

/* wav2flac (wav2flac.zig:10-97) for PCM in memory: the 73-byte header (STREAMINFO not
 * last, VORBIS_COMMENT last) + every frame, STREAMINFO carrying the frame-size
 * min/max (from the GPU's per-frame sizes, replayed in frame order) and the MD5 of
 * the PCM bytes (the context's MD5 engine; the host engine hashes on a thread
 * that runs beside the GPU encode). */
int flacgpu_encode_file(flacgpu_ctx *ctx, const void *pcm, uint32_t bytes_per_sample, uint64_t n_samples,
                        uint8_t *out, size_t out_cap, size_t *out_len);
/* flacgpu_encode_file for n_files PCM buffers at once on one context: out[i]
 * (capacity out_cap[i]) receives exactly the bytes flacgpu_encode_file writes for
 * file i, out_len[i] their count (all 0 on an error).  Every file's frames go
 * through one pipelined upload / encode / download schedule that runs on from
 * file to file, and every file's MD5 is hashed on the host pool in one batch
 * beside it: the many-files-per-GPU form of wav2flac.zig:10-97. */
int flacgpu_encode_files(flacgpu_ctx *ctx, uint32_t n_files, const void *const *pcm, uint32_t bytes_per_sample,
                         const uint64_t *n_samples, uint8_t *const *out, const size_t *out_cap, size_t *out_len);
/* The whole conversion of an in-memory WAV file on HIP device `device`
 * (Config.default for the WAV's channels and bit depth). */
int flacgpu_wav_to_flac(int device, const void *wav, size_t wav_len, uint8_t *out, size_t out_cap, size_t *out_len);

/* A decode-only context (no reference counterpart: the reference has no decoder).  flacgpu_open's
 * block_size limit, 4096, is the encoder's; RFC 9639's streamable subset allows frames of up to
 * 16384 samples, and encoders other than this one write them (4608 is a table code).  A context
 * opened here decodes frames of `channels` x `bits_per_sample` of up to max_block samples:
 * 1..FLACGPU_DECODER_MAX_BLOCK, and at most FLACGPU_DECODER_MAX_BLOCK_32 at 32 bits per sample, whose
 * 64-bit sample planes of larger frames do not fit a compute unit's LDS; anything else, and a bad
 * channel count, depth or rate, is FLACGPU_ERR_INVALID_CONFIG.  It allocates no encode buffers and is
 * closed by flacgpu_close.  Every entry point of the "Decode and verify" section below but
 * flacgpu_verify_plan_device works on it, and so do flacgpu_sync_check, flacgpu_get_config (block_size
 * = max_block, the encode options zero), the timing calls and the streaming MD5 (host engine).  Every entry point that
 * encodes, and flacgpu_plan_create* (so nothing that needs a plan can be reached), returns
 * FLACGPU_ERR_INVALID_CONFIG.  max_frames_per_call as in flacgpu_open. */
#define FLACGPU_DECODER_MAX_BLOCK 16384
#define FLACGPU_DECODER_MAX_BLOCK_32 8192
int flacgpu_open_decoder(int device, uint32_t sample_rate, uint8_t channels, uint8_t bits_per_sample,
                         uint32_t max_block, uint32_t max_frames_per_call, flacgpu_ctx **out);

/* ---- Decode and verify (no reference counterpart: the reference's readme lists a decoder as
 *      queued).  Frames are decoded where the encode entry points leave them; DESIGN.md
 *      "Decode and verify". ------------------------------------------------------------------ */
/* Per-frame status.  1..7 are minus the codes of the CPU verifier decoder (oracle/flac_decode.c),
 * checked in its order; the first failure wins. */
enum { FLACGPU_DEC_OK = 0, FLACGPU_DEC_SYNC = 1, FLACGPU_DEC_HEADER = 2, FLACGPU_DEC_CRC8 = 3,
       FLACGPU_DEC_SUBFRAME = 4, FLACGPU_DEC_CRC16 = 5, FLACGPU_DEC_TRUNCATED = 6, FLACGPU_DEC_RANGE = 7,
       FLACGPU_DEC_MISMATCH = 8 };
typedef struct {                             /* 32 bytes */
    uint32_t status, block_size;
    uint64_t number;                         /* coded frame number */
    uint32_t sample_rate;
    uint32_t first_bad;                      /* MISMATCH: first differing interleaved sample of the frame;
                                                0xFFFFFFFF: frame number / block size not the expected one */
    uint8_t channel_assign, bits, pad[6];
} flacgpu_decode_result;

/* Decode n_frames (<= max_frames_per_call) device-resident frames of the context's channel count
 * and bit depth: frame f is the d_frame_bytes[f] bytes at d_frames + d_frame_offsets[f] (the
 * layout of flacgpu_encode_plan_device).  Its PCM region starts d_pcm_offsets[f] bytes into
 * d_pcm_out / d_pcm_expect; d_pcm_offsets NULL: the frames are consecutive blocks of one stream
 * (offsets from a scan of the parsed block sizes).  d_pcm_out (NULL: none, capacity pcm_cap
 * bytes) receives interleaved little-endian PCM of bits/8 bytes per sample; a frame whose region
 * would pass pcm_cap gets RANGE.  d_pcm_expect (NULL: none) is compared with the decoded samples:
 * a difference gives MISMATCH.  A frame with a non-zero status writes no PCM.  d_results[f] and
 * *d_bad_count (frames with a non-zero status) are device memory.  Asynchronous on hip_stream.
 * The decode scratch of a context is allocated by its first decode call.  Blocks larger than
 * the context's block_size (flacgpu_open_decoder: max_block) are RANGE. */
int flacgpu_decode_frames_device(flacgpu_ctx *ctx, const uint8_t *d_frames, const uint64_t *d_frame_offsets,
                                 const uint32_t *d_frame_bytes, uint64_t n_frames, const uint64_t *d_pcm_offsets,
                                 uint8_t *d_pcm_out, uint64_t pcm_cap, const uint8_t *d_pcm_expect,
                                 flacgpu_decode_result *d_results, uint32_t *d_bad_count, void *hip_stream);
/* The --verify of flacgpu_encode_plan_device: decode every frame of the plan from d_out and compare
 * it with the PCM it was encoded from (d_pcm).  The expected PCM offset, frame number and sample
 * count of every frame come from the plan's frame table; another number or size gives MISMATCH
 * with first_bad = 0xFFFFFFFF.  The plan must hold at most max_frames_per_call frames. */
int flacgpu_verify_plan_device(flacgpu_ctx *ctx, const flacgpu_plan *plan, const void *d_pcm, const uint8_t *d_out,
                               const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                               flacgpu_decode_result *d_results, uint32_t *d_bad_count, void *hip_stream);
/* Host buffers, synchronous, in chunks of max_frames_per_call: the concatenated frames of one
 * stream to pcm_out (the PCM of the frames with status 0, each at the place its predecessors'
 * block sizes give it); *n_samples = interchannel samples.  Returns FLACGPU_OK with the
 * per-frame statuses in results[]; the call's own errors use the codes above. */
int flacgpu_decode_frames(flacgpu_ctx *ctx, const uint8_t *frames, const uint32_t *frame_bytes, uint64_t n_frames,
                          uint8_t *pcm_out, size_t pcm_cap, uint64_t *n_samples, flacgpu_decode_result *results);
/* Frame index of a FLAC file in memory (host only, no GPU): "fLaC", the metadata blocks
 * (STREAMINFO to *streaminfo, the others skipped by length), then the frame boundaries: a frame
 * ends where a CRC-16 over it is good and the next frame header (sync code, good CRC-8) or the
 * end of the data follows.  streaminfo NULL: flac points at a bare run of frames.  frame_bytes[]
 * (capacity cap) gets the sizes, *n_frames their count (also when cap is too small:
 * FLACGPU_ERR_OUTPUT_TOO_SMALL), *first_frame_offset (may be NULL) the first frame's offset. */
int flacgpu_flac_index(const void *flac, size_t len, flacgpu_streaminfo *streaminfo, size_t *first_frame_offset,
                       uint32_t *frame_bytes, size_t cap, size_t *n_frames);
/* The same index of a bare run of frames resident in device memory (any alignment, len <= 2^32 - 1),
 * found on the device: d_frame_offsets[] (relative to d_data) and d_frame_bytes[] (capacity cap
 * each) are what flacgpu_decode_frames_device takes.  *d_result (device memory): INDEX_OK with the
 * frame count and the same sizes flacgpu_flac_index(..., streaminfo = NULL) finds on these bytes;
 * INDEX_INVALID (0 frames) where that call returns FLACGPU_ERR_INVALID_INPUT; INDEX_TOO_SMALL
 * with the true count where it exceeds cap.  Only an OK result writes the two arrays, and only
 * their first n_frames entries.  stream_bits / stream_rate stand for the "from STREAMINFO"
 * header codes (16 and 0 in flacgpu_flac_index without a streaminfo).  Asynchronous on
 * hip_stream, no host synchronisation (but when the context's index scratch, sized from len and
 * cap, has to grow); independent of max_frames_per_call. */
enum { FLACGPU_INDEX_OK = 0, FLACGPU_INDEX_INVALID = 1, FLACGPU_INDEX_TOO_SMALL = 2 };
typedef struct { uint64_t n_frames; uint32_t status; uint32_t reserved; } flacgpu_index_result; /* device memory */
int flacgpu_flac_index_device(flacgpu_ctx *ctx, const uint8_t *d_data, uint64_t len,
                              uint32_t stream_bits, uint32_t stream_rate,
                              uint64_t *d_frame_offsets, uint32_t *d_frame_bytes, uint64_t cap,
                              flacgpu_index_result *d_result, void *hip_stream);
/* Decode and MD5 (the host engine) of a whole file whose channel count and bit depth are the
 * context's: the frames are uploaded once, indexed on the device (flacgpu_flac_index_device) and
 * decoded from there in chunks of max_frames_per_call, each chunk's PCM hashed on the host while
 * the next decodes; a stream the device index refuses goes through flacgpu_flac_index and
 * flacgpu_decode_frames.  *md5_ok (may be NULL) = the PCM's MD5 and sample count are
 * STREAMINFO's.  A damaged frame makes the call fail with FLACGPU_ERR_INVALID_INPUT. */
int flacgpu_decode_file(flacgpu_ctx *ctx, const void *flac, size_t len, uint8_t *pcm_out, size_t pcm_cap,
                        uint64_t *n_samples, int *md5_ok);
/* flacgpu_flac_index_device over n_streams (<= 65535, more: FLACGPU_ERR_INVALID_INPUT) bare runs of
 * frames of one device buffer in one call: stream s is the stream_lens[s] (<= 2^32 - 1) bytes at
 * d_data + stream_offsets[s], any alignment, with its own stream_bits[s] / stream_rates[s] (NULL:
 * 16 / 0 for all).  It owns entries [table_first[s], + table_caps[s]) of d_frame_offsets[] and
 * d_frame_bytes[] and d_results[s]; these are exactly what the single call leaves for that stream
 * alone (a zero-length stream: OK, 0 frames), but the offsets are relative to d_data, so a slice
 * feeds flacgpu_decode_frames_device with d_frames = d_data.  One stream's verdict touches no
 * other stream's slice or result.  The five stream arrays are host memory.  The number of kernel
 * launches does not depend on n_streams; the whole call is one timed launch of FLACGPU_K_INDEX.
 * Asynchronous on hip_stream: one table of n_streams entries is copied to the device, and the
 * host waits only when the context's index scratch (sized from the lengths and caps) has to grow. */
int flacgpu_flac_index_streams_device(flacgpu_ctx *ctx, const uint8_t *d_data, uint32_t n_streams,
                                      const uint64_t *stream_offsets, const uint64_t *stream_lens,
                                      const uint32_t *stream_bits, const uint32_t *stream_rates,
                                      const uint64_t *table_first, const uint64_t *table_caps,
                                      uint64_t *d_frame_offsets, uint32_t *d_frame_bytes,
                                      flacgpu_index_result *d_results, void *hip_stream);
/* Index (the call above, into a table the context owns) and decode n_streams device-resident
 * streams of the context's channel count and bit depth: stream s's PCM goes to the pcm_caps[s]
 * bytes at d_pcm_out + pcm_offsets[s] (host arrays), each frame at the place its predecessors'
 * block sizes give it.  All frames of all streams, in stream order, are cut into chunks of
 * max_frames_per_call that run on from one stream into the next.  A frame whose region would pass
 * its stream's capacity gets RANGE and writes nothing; a stream whose index is not OK decodes
 * nothing.  d_results[s] (device memory) sums the stream up.  d_md5 (device, 16 * n_streams bytes,
 * or NULL): the MD5 of every stream's decoded PCM by one batched device launch, 16 zero bytes for
 * a stream with a bad index or a bad frame; it needs every pcm_offsets[s] to be a multiple of 4.
 * The call waits for hip_stream ONCE, after the index, to read the frame counts; everything after
 * that is only queued. */
typedef struct {            /* 32 bytes, device memory */
    uint64_t n_frames, n_samples;      /* interchannel samples of the frames with status 0 */
    uint32_t index_status;             /* FLACGPU_INDEX_* */
    uint32_t bad_frames;               /* frames with a non-zero status */
    uint32_t first_bad_frame;          /* 0xFFFFFFFF: none */
    uint32_t first_bad_status;         /* FLACGPU_DEC_* of that frame */
} flacgpu_stream_result;
int flacgpu_decode_streams_device(flacgpu_ctx *ctx, const uint8_t *d_data, uint32_t n_streams,
                                  const uint64_t *stream_offsets, const uint64_t *stream_lens,
                                  const uint32_t *stream_bits, const uint32_t *stream_rates,
                                  uint8_t *d_pcm_out, const uint64_t *pcm_offsets, const uint64_t *pcm_caps,
                                  flacgpu_stream_result *d_results, uint8_t *d_md5, void *hip_stream);
/* flacgpu_decode_file for n_files (<= 65535) files in one call: status[i], n_samples[i], md5_ok[i]
 * (md5_ok may be NULL) and the bytes at pcm_out[i] (capacity pcm_cap[i]) are what
 * flacgpu_decode_file gives for file i alone on this context; one bad file (metadata, channel
 * count or bit depth, a damaged frame, a capacity too small) does not fail the others, and the
 * return value is for the call's own errors only.  All files' frames are uploaded into one device
 * buffer and go through flacgpu_decode_streams_device; the MD5s are hashed in one batch by the
 * engine flacgpu_md5_engine_for picks (the device kernel, or flacgpu_md5_many on the host pool).
 * A file the batch does not decode cleanly goes through flacgpu_decode_file afterwards.  The
 * whole batch is resident at once: a device allocation that fails returns
 * FLACGPU_ERR_OUT_OF_MEMORY; splitting an oversized batch into groups of files is the caller's. */
int flacgpu_decode_files(flacgpu_ctx *ctx, uint32_t n_files, const void *const *flac, const size_t *len,
                         uint8_t *const *pcm_out, const size_t *pcm_cap, uint64_t *n_samples, int *md5_ok,
                         int *status);
/* The sample positions of n_streams (<= 65535) streams that flacgpu_flac_index_streams_device has
 * indexed (same d_data, table_first, table_caps, stream_bits, stream_rates; the two tables and
 * d_index_results as that call left them): d_frame_first_sample[table_first[s] + i] = the
 * interchannel samples before frame i of stream s, d_stream_samples[s] = the stream's total (both
 * device memory; the first is laid out like the frame tables).  A frame's block size is what its
 * header states, read from at most 16 bytes at its offset with no regard to the context's channel
 * count, depth or block size; positions are the exclusive sum of the block sizes, never the coded
 * frame or sample number.  A stream whose index result is not OK gets total 0 and none of its
 * entries written.  The table is the caller's to keep: a batch that stays resident is indexed and
 * scanned once and serves any number of flacgpu_decode_windows_device calls.  Asynchronous on
 * hip_stream, no host synchronisation (but when the context's scratch has to grow): the frame
 * counts are read on the device, the grids are sized from table_caps; independent of
 * max_frames_per_call.  Timed as FLACGPU_K_SCAN. */
int flacgpu_flac_positions_streams_device(flacgpu_ctx *ctx, const uint8_t *d_data, uint32_t n_streams,
                                          const uint64_t *table_first, const uint64_t *table_caps,
                                          const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                          const flacgpu_index_result *d_index_results,
                                          const uint32_t *stream_bits, const uint32_t *stream_rates,
                                          uint64_t *d_frame_first_sample, uint64_t *d_stream_samples, void *hip_stream);
/* Decode n_windows (<= 65535, more: FLACGPU_ERR_INVALID_INPUT) sample windows of indexed streams
 * without decoding the rest: window w is samples [window_start[w], + window_count[w]) of stream
 * window_stream[w] (< n_streams, else FLACGPU_ERR_INVALID_INPUT), clipped to the stream's total; a
 * window that starts at or past the end or has count 0 is OK with 0 samples and 0 frames.  Its
 * bytes go to d_pcm_out + pcm_offsets[w] (any alignment) and are exactly those the whole decode
 * of the stream puts at [start * per, (start + n_samples) * per), per = channels * bytes per
 * sample.  Windows may share a stream and overlap.  Only the frames that hold a window's samples
 * (found by binary search of the positions) are parsed past their header and reconstructed, whole,
 * into scratch the context owns, in chunks of max_frames_per_call that run on from one window
 * into the next; one copy pass then delivers each window's bytes.  So a frame this context cannot
 * decode harms no window that does not cover it.  d_results[w] (device memory): BAD_INDEX where
 * the stream's index result is not OK, BAD_FRAME where a covering frame has a non-zero decode
 * status (first_bad_frame counted in the stream), TOO_SMALL where n_samples * per > pcm_caps[w];
 * each of the three delivers 0 samples and writes nothing, and nothing is ever written outside
 * [pcm_offsets[w], + n_samples * per).  The window and pcm arrays and table_first are host memory.
 * The call waits for hip_stream ONCE, to read the covers; everything after that is only queued.
 * The cover is timed as FLACGPU_K_SCAN, parse and reconstruct as in every decode, the copy is not. */
enum { FLACGPU_WINDOW_OK = 0, FLACGPU_WINDOW_BAD_INDEX = 1, FLACGPU_WINDOW_BAD_FRAME = 2, FLACGPU_WINDOW_TOO_SMALL = 3 };
typedef struct {                 /* 32 bytes, device memory */
    uint64_t n_samples;          /* interchannel samples delivered */
    uint64_t first_frame;        /* first covering frame, counted in its stream */
    uint32_t n_frames;           /* covering frames decoded */
    uint32_t status;             /* FLACGPU_WINDOW_* */
    uint32_t first_bad_frame;    /* BAD_FRAME: counted in its stream; else 0xFFFFFFFF */
    uint32_t first_bad_status;   /* FLACGPU_DEC_* of that frame */
} flacgpu_window_result;
int flacgpu_decode_windows_device(flacgpu_ctx *ctx, const uint8_t *d_data,
                                  uint32_t n_streams, const uint64_t *table_first,
                                  const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                  const flacgpu_index_result *d_index_results,
                                  const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                  uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                  const uint64_t *window_count,
                                  uint8_t *d_pcm_out, const uint64_t *pcm_offsets, const uint64_t *pcm_caps,
                                  flacgpu_window_result *d_results, void *hip_stream);
/* The same windows delivered as tensor elements instead of PCM bytes.  A source sample is the
 * bits / 8 bytes the decode writes (signed, little-endian, 8-bit included), sign-extended to
 * int32 x; its element is
 *   FLACGPU_SAMPLE_I32   x, unscaled
 *   FLACGPU_SAMPLE_F32   (float)x * 2^-(bits-1): the conversion rounds to nearest-even (inexact only
 *                        for 32-bit samples with |x| >= 2^24), the scale is exact; in [-1, 1]
 *   FLACGPU_SAMPLE_F16   that value rounded to nearest-even, subnormal results kept
 *   FLACGPU_SAMPLE_BF16  that value rounded to nearest-even
 * With C channels, n samples delivered after clipping and count = window_count[w], sample t of
 * channel c is element t * C + c from d_out + out_offsets[w] * element size (interleaved), or
 * c * count + t with FLACGPU_DELIVER_PLANAR: the plane stride is the stated count, whatever n turns
 * out to be.  With FLACGPU_DELIVER_PAD the elements of t in [n, count) are written as zero in every
 * channel -- also where n is 0 -- so every OK window fills exactly C * count elements; without it
 * they are not touched.  out_offsets and out_caps are in ELEMENTS.  TOO_SMALL where C * count
 * (PLANAR or PAD) or else C * n exceeds out_caps[w], decided before anything is decoded and with
 * no product formed, so count = 2^64 - 1 under PLANAR or PAD is TOO_SMALL.  n_samples of a result
 * counts decoded samples; padding is never counted.  A window that is not OK writes nothing, PAD or
 * not.  An unknown sample_format, unknown flag bits, d_out not aligned to the element size, or
 * out_offsets[w] + out_caps[w] passing 64 bits: FLACGPU_ERR_INVALID_INPUT before any device work.
 * Everything else -- the one wait, the chunks, BAD_INDEX and BAD_FRAME, windows that share streams
 * and overlap, what is timed -- is as in flacgpu_decode_windows_device. */
enum { FLACGPU_SAMPLE_I32 = 0, FLACGPU_SAMPLE_F32 = 1, FLACGPU_SAMPLE_F16 = 2, FLACGPU_SAMPLE_BF16 = 3 };
enum { FLACGPU_DELIVER_PLANAR = 1, FLACGPU_DELIVER_PAD = 2 };
int flacgpu_decode_windows_device_as(flacgpu_ctx *ctx, const uint8_t *d_data,
                                     uint32_t n_streams, const uint64_t *table_first,
                                     const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                     const flacgpu_index_result *d_index_results,
                                     const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                     uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                     const uint64_t *window_count,
                                     uint32_t sample_format, uint32_t flags,
                                     void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                     flacgpu_window_result *d_results, void *hip_stream);
/* The same delivery with a channel count other than the source's.  A window has K = out_channels
 * (1 to 8) channels; channel_masks (HOST memory, K entries) names the source channels of each: bit
 * c of channel_masks[k] is source channel c of the context's C.  With m the number of bits set,
 * sample t of output channel k is
 *   m = 0        zero in every format (bit pattern 0)
 *   m = 1        that source sample's element, bit for bit what flacgpu_decode_windows_device_as
 *                delivers
 *   m = 2, 4, 8  the exact mean: with s the exact integer sum of the m sign-extended source samples
 *                (|s| <= 8 * 2^31), FLACGPU_SAMPLE_F32 is (float)s * 2^-(bits - 1 + log2 m) -- the
 *                conversion rounds to nearest-even (inexact only for |s| >= 2^24), the scale is
 *                exact; in [-1, 1] -- and F16 and BF16 are that value narrowed as above
 * A mix is valid when no mask has a bit at or above C, every m is 0, 1, 2, 4 or 8, and for
 * FLACGPU_SAMPLE_I32 every m is at most 1 (selection, duplication, permutation and silence: a
 * mean has no integer value to deliver).  Layout, padding and capacity are those of
 * flacgpu_decode_windows_device_as with K in place of C: element t * K + k, or k * count + t with
 * FLACGPU_DELIVER_PLANAR; out_offsets and out_caps in ELEMENTS; TOO_SMALL where K * count (PLANAR
 * or PAD) or else K * n exceeds out_caps[w].  An invalid mix, out_channels outside 1..8, a NULL
 * channel_masks and every argument error of flacgpu_decode_windows_device_as:
 * FLACGPU_ERR_INVALID_INPUT before any device work.  Everything else -- the one wait, the chunks,
 * BAD_INDEX and BAD_FRAME, windows that share streams and overlap, what is timed -- is as in
 * flacgpu_decode_windows_device. */
int flacgpu_decode_windows_device_mix(flacgpu_ctx *ctx, const uint8_t *d_data,
                                      uint32_t n_streams, const uint64_t *table_first,
                                      const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                      const flacgpu_index_result *d_index_results,
                                      const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                      uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                      const uint64_t *window_count,
                                      uint32_t sample_format, uint32_t flags,
                                      uint32_t out_channels, const uint8_t *channel_masks,
                                      void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                      flacgpu_window_result *d_results, void *hip_stream);
/* The same delivery at another sample rate: a stream of rate src_rate is delivered at dst_rate by a
 * polyphase windowed-sinc FIR that runs in the delivery pass, over the same decoded covering frames.
 * With g = gcd(src_rate, dst_rate), L = dst_rate / g and M = src_rate / g, a ratio is valid when the
 * rates differ, 1 <= L, M <= 1024 and M <= 12 * L.  The filter: Hw = 24 where L >= M, else
 * ceil(24 * M / L); T = 2 * Hw taps (<= 576); for phase p < L and tap k < T, d = (k - Hw + 1) - p / L,
 * c = 0.95 * min(1, L / M), h64(p, k) = c * sinc(c * d) * I0(9 * sqrt(max(0, 1 - (d / Hw)^2))) / I0(9),
 * every phase divided by its own sum (DC gain 1), all in double (I0 by its power series), then
 * h[p][k] = (float)h64(p, k).  flacgpu_resample_filter (host only, no device) gives *up = L,
 * *down = M, *taps = T (each may be NULL) and the table h[p][k], row-major, L * T floats, in coeffs;
 * *n = L * T, FLACGPU_ERR_OUTPUT_TOO_SMALL (with *n set) where cap is less, FLACGPU_ERR_INVALID_INPUT
 * for an invalid ratio. */
int flacgpu_resample_filter(uint32_t src_rate, uint32_t dst_rate, uint32_t *up, uint32_t *down, uint32_t *taps,
                            float *coeffs, size_t cap, size_t *n);
/* The sample rule.  A stream of `total` source samples has out_total = ceil(total * L / M) output
 * samples; output sample j sits at source position j * M / L: i0 = j * M div L, p = j * M mod L.
 * With x[i] the FLACGPU_SAMPLE_F32 element of a source sample (+0.0f for i < 0 or i >= total: the
 * extension is zero), y = +0.0f, then for k = 0 .. T - 1 in this order
 * y = fmaf(h[p][k], x[i0 - Hw + 1 + k], y): one accumulator, one correctly rounded fused
 * multiply-add a tap.  flacgpu_resample_f32_host (host only) is this rule over one channel of F32
 * elements x[0 .. total), total <= 2^40: output samples [start, start + count) clipped to out_total
 * go to y (room for min(count, out_total - start) floats), *n of them.  It is a statement of the
 * rule for callers and tests, bit for bit what the device delivers; it is NOT a decode path: there
 * is no CPU fallback, a FLAC stream is decoded and resampled on the device only. */
int flacgpu_resample_f32_host(const float *x, uint64_t total, uint32_t src_rate, uint32_t dst_rate, uint64_t start,
                              uint64_t count, float *y, uint64_t *n);
/* flacgpu_decode_windows_device_mix through that filter.  The context's streams have rate src_rate;
 * window_start / window_count, out_offsets / out_caps and the results' n_samples are in OUTPUT samples
 * and elements at dst_rate: window w is output samples [start, start + count) clipped to out_total of
 * its stream, n of them delivered.  x[i] of output channel k is the F32 element the mix rule gives
 * (one source channel, the exact mean of 2, 4 or 8, zero for an empty mask); channel_masks NULL is
 * the identity of the context's C channels (out_channels is then ignored).  The element is y
 * (FLACGPU_SAMPLE_F32) or y narrowed as above (F16, BF16; |y| can pass 1 and stays below 4);
 * FLACGPU_SAMPLE_I32 is not offered.  The covering frames are those of the source samples
 * [max(0, start * M div L - Hw + 1), min(total, (start + n - 1) * M div L + Hw + 1)): first_frame and
 * n_frames of a result are theirs, and BAD_FRAME where any of them is bad, one that only the
 * filter's reach touches included.  Layout, FLACGPU_DELIVER_PAD (zeros for [n, count)) and TOO_SMALL
 * are those of _mix with the output count and n; a window that is not OK writes nothing.  An invalid
 * ratio, equal rates, FLACGPU_SAMPLE_I32 and every argument error of _mix (a NULL channel_masks
 * excepted): FLACGPU_ERR_INVALID_INPUT before any device work.  The coefficient table lives in
 * device memory the context owns, one per ratio, built on the host and uploaded by the first call
 * that needs it -- that call waits for hip_stream once more -- and freed by flacgpu_close.  The one
 * wait for the covers, the 65535-window limit, the chunks and the stream semantics are those of
 * flacgpu_decode_windows_device; the FIR kernel is not timed. */
int flacgpu_decode_windows_device_resample(flacgpu_ctx *ctx, const uint8_t *d_data,
                                           uint32_t n_streams, const uint64_t *table_first,
                                           const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                           const flacgpu_index_result *d_index_results,
                                           const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                           uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                           const uint64_t *window_count,
                                           uint32_t sample_format, uint32_t flags,
                                           uint32_t out_channels, const uint8_t *channel_masks,
                                           uint32_t src_rate, uint32_t dst_rate,
                                           void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                           flacgpu_window_result *d_results, void *hip_stream);
/* The same delivery as short-time power spectra, bare or folded onto the rows of a filter bank (mel
 * bands, for one).  N = n_fft is even, 16 <= N <= 2048; H = hop, 1 <= H <= N; B = N / 2 + 1 bins;
 * R = n_rows, 0 <= R <= 256, R = 0 meaning no filter bank: the rows are the B bins.  The table, in
 * double, rounded once to float: w[n] = 0.5 - 0.5 cos(2 pi n / N) (the periodic Hann window),
 * c[b][n] = (float)(w[n] cos(2 pi ((b n) mod N) / N)), s[b][n] = (float)(-w[n] sin(2 pi ((b n) mod N) / N)),
 * b n reduced in integers.  flacgpu_features_table (host only, no device) gives it as [2][B][N], the
 * cos plane then the sin plane; *n = 2 B N, FLACGPU_ERR_OUTPUT_TOO_SMALL (with *n set) where cap is
 * less, FLACGPU_ERR_INVALID_INPUT for an invalid n_fft. */
typedef struct { uint32_t n_fft, hop, n_rows; } flacgpu_features;
int flacgpu_features_table(uint32_t n_fft, float *table, size_t cap, size_t *n);
/* The rule.  x is one output channel of the delivery as FLACGPU_SAMPLE_F32 elements at the delivered
 * rate -- what flacgpu_decode_windows_device_mix delivers, or _resample where the rates differ --
 * `total` samples, +0.0f outside [0, total).  Frame t of a window that starts at sample `start` is
 * centred at q = start + t H and reads xf[n] = x[q - N / 2 + n].  re_b = +0.0f, then for n = 0 .. N - 1
 * in this order re_b = fmaf(c[b][n], xf[n], re_b); im_b the same chain with s;
 * P_b = fmaf(im_b, im_b, re_b * re_b), the product rounded to float first.  Row r is P_r (R = 0), or
 * with the caller's F[R][B] (float32, finite, host memory) m_r = +0.0f, then for b = 0 .. B - 1 in
 * this order m_r = fmaf(F[r][b], P_b, m_r).  The elements are linear power: no logarithm is applied
 * (two libraries' logf do not agree bit for bit).  Every frame t < frames is computed by this rule:
 * a frame that reaches past either end of the stream reads zeros there, one wholly outside is +0.0f
 * in every row; there is no other padding.  *n counts the frames whose centre lies inside the
 * stream: 0 where start >= total, else min(frames, ceil((total - start) / H)).
 * flacgpu_features_f32_host (host only) is this rule over one channel x[0 .. total), total <= 2^40,
 * (frames - 1) H + N < 2^31: y is [rows][frames].  It passes over zero entries of F, which changes
 * no bit (P is finite, so fmaf(0, P, m) = m).  It is a statement of the rule for callers and tests,
 * bit for bit what the device delivers; it is NOT a decode path. */
int flacgpu_features_f32_host(const float *x, uint64_t total, const flacgpu_features *ft, const float *filters,
                              uint64_t start, uint64_t frames, float *y, uint64_t *n);
/* The call.  window_start is in samples at the delivered rate, window_frames[w] the frame count;
 * src_rate = dst_rate = 0 is no rate change, otherwise the ratio rules of _resample hold;
 * channel_masks NULL is the identity of the context's C channels (K = C), else K = out_channels.
 * Row r, frame t of channel k is element (k rows + r) frames + t from d_out + out_offsets[w] *
 * element size; an OK window fills exactly K rows frames elements.  sample_format is
 * FLACGPU_SAMPLE_F32, or F16 / BF16: the F32 value narrowed as every other element is (linear power
 * can pass 65504: F16 then rounds to infinity; BF16 keeps the range).  n_samples of a result is the
 * rule's n (frames); first_frame and n_frames are those of the covering frames of the samples
 * [start - N / 2, start + (frames - 1) H + N / 2) inside the stream -- through the resampler's own
 * reach where the rates differ -- and BAD_INDEX and BAD_FRAME are as in _resample over them.
 * TOO_SMALL where K rows frames exceeds out_caps[w] (no product overflows), decided before anything
 * is decoded.  A window that is not OK writes nothing, and nothing is ever written outside a
 * window's elements.  FLACGPU_ERR_INVALID_INPUT before any device work: an invalid *ft, a NULL
 * filters with R > 0, a non-finite entry of filters, FLACGPU_SAMPLE_I32 or an unknown format, an
 * invalid ratio, a span (frames - 1) H + N of 2^31 or more, and every argument error of _mix (a
 * NULL channel_masks excepted).  The call runs in two stages: the window delivery itself leaves
 * every window's span as F32 in scratch the context owns (freed by flacgpu_close), then one kernel
 * computes the frames on the f32-input matrix instructions, whose accumulation is the chain above
 * bit for bit.  The STFT table (one per n_fft, kept) and the filter bank (found again by its
 * content; the context keeps the last 16) live in device memory the context owns, uploaded by the
 * first call that needs them -- that call waits for hip_stream once more for each.  The one wait for
 * the covers, the 65535-window limit, the chunks and the stream semantics are those of
 * flacgpu_decode_windows_device; the feature kernel is not timed. */
int flacgpu_decode_windows_device_features(flacgpu_ctx *ctx, const uint8_t *d_data,
                                           uint32_t n_streams, const uint64_t *table_first,
                                           const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                           const flacgpu_index_result *d_index_results,
                                           const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                           uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                           const uint64_t *window_frames,
                                           uint32_t sample_format,
                                           uint32_t out_channels, const uint8_t *channel_masks,
                                           uint32_t src_rate, uint32_t dst_rate,
                                           const flacgpu_features *ft, const float *filters,
                                           void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                           flacgpu_window_result *d_results, void *hip_stream);
/* The channel mix by a weight matrix.  A source sample has the context's C channels; x_c is the
 * FLACGPU_SAMPLE_F32 element of channel c exactly as flacgpu_decode_windows_device_as delivers it.  W
 * is a row-major K x C float matrix (HOST memory).  Output channel k is y = +0.0f, then for
 * c = 0 .. C - 1 in this order y = fmaf(W[k][c], x_c, y): one accumulator, one correctly rounded
 * fused multiply-add a source channel, as in the resampler and the features.  FLACGPU_SAMPLE_F32 is
 * y; F16 and BF16 are y rounded to nearest-even as every other element is (|y| can reach 2^35: F16
 * is infinity from 65520 on, BF16 keeps the range); FLACGPU_SAMPLE_I32 is not offered.  A matrix is
 * valid when C and K are 1 to 8, the format is F32, F16 or BF16 and every weight is 0 (of either
 * sign) or has 2^-32 <= |w| <= 2^32 -- NaN, infinities and subnormals are refused.  The bounds are
 * derived: |x_c| is 0 or lies in [2^-31, 1], so every product is 0 or a normal number, a multiple
 * of 2^-86 and at most 2^32; no fused multiply-add underflows or overflows (|y| <= 2^35); an exact
 * cancellation gives +0.0f, so no accumulator is ever -0.0f or subnormal; and passing over zero
 * weights, and over channels whose x_c is 0, changes no bit (the library does not read a channel
 * whose weight is 0).  A mean of three is {1/3, 1/3, 1/3}, mid/side {0.5, 0.5}, {0.5, -0.5}.
 * flacgpu_mix_weights_valid (host only): 1 where `weights` (out_channels x channels) is valid for
 * sample_format, else 0.  flacgpu_mix_weights_f32_host (host only): the rule over n samples of
 * `channels` channels, samples[n][channels] sign-extended samples of `bits` (8, 16, 24, 32) bits,
 * y[n][out_channels]; FLACGPU_ERR_INVALID_INPUT for an invalid matrix, depth or a sample outside the
 * depth, n <= 2^40.  It is a statement of the rule for callers and tests, bit for bit what the
 * device delivers; it is NOT a decode path. */
int flacgpu_mix_weights_valid(uint32_t channels, uint32_t out_channels, const float *weights, uint32_t sample_format);
int flacgpu_mix_weights_f32_host(const int32_t *samples, uint64_t n, uint32_t channels, uint32_t bits,
                                 uint32_t out_channels, const float *weights, float *y);
/* Every delivery above through one call that takes the delivery as a struct: the signature that
 * further kinds of delivery extend by fields, not by arguments.  With channel_weights NULL the call
 * IS the existing one the struct describes -- features != NULL: _features (window_count holds the
 * frame counts, flags must be 0); else src_rate or dst_rate != 0: _resample; else channel_masks !=
 * NULL: _mix; else _as -- with the same checks, bytes and results.  With channel_weights each of
 * those four deliveries has K = out_channels channels made by the weighted rule above in place of
 * the mask rule: the elements of _as / _mix; the planes x[i] the filter of _resample runs over;
 * the channels the frames of _features are taken from (through the resampler first where the rates
 * differ).  Layout, padding, capacity, statuses and results are those of the call it stands for
 * with K channels.  FLACGPU_ERR_INVALID_INPUT before any device work: a NULL `how`, a size other
 * than sizeof(flacgpu_window_delivery), both channel_masks and channel_weights, a matrix that
 * flacgpu_mix_weights_valid refuses for the context's C (FLACGPU_SAMPLE_I32 with weights included),
 * flags with features, and every argument error of the call it stands for.  The matrix lives in
 * device memory the context owns, found again by its content (the context keeps the last 16),
 * uploaded by the first call that needs it -- that call waits for hip_stream once more -- and freed
 * by flacgpu_close. */
typedef struct {
    uint32_t size;                  /* sizeof(flacgpu_window_delivery) */
    uint32_t sample_format, flags;  /* as flacgpu_decode_windows_device_as */
    uint32_t out_channels;          /* K, with masks or weights */
    const uint8_t *channel_masks;   /* host, K entries, or NULL */
    const float *channel_weights;   /* host, K * C floats row-major, or NULL; not both */
    uint32_t src_rate, dst_rate;    /* 0, 0: no rate change; else the rules of _resample */
    const flacgpu_features *features; /* NULL: samples; else the rules of _features */
    const float *filters;
} flacgpu_window_delivery;
int flacgpu_decode_windows_device_to(flacgpu_ctx *ctx, const uint8_t *d_data,
                                     uint32_t n_streams, const uint64_t *table_first,
                                     const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                     const flacgpu_index_result *d_index_results,
                                     const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                     uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                     const uint64_t *window_count,
                                     const flacgpu_window_delivery *how,
                                     void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                     flacgpu_window_result *d_results, void *hip_stream);
/* The same delivery convolved with a FIR filter of the window's choice: band-limiting, a microphone
 * or device response, pre-emphasis, a tilt, a short room response.  The rule.  x is one output
 * channel of the delivery as FLACGPU_SAMPLE_F32 elements at the delivered rate -- what _as, _mix or
 * the weighted mix of _to delivers, or _resample where the rates differ -- `total` samples, +0.0f
 * outside [0, total).  A filter has T taps h[0 .. T), 1 <= T <= 4096, all finite, and a delay d,
 * 0 <= d < T.  Element t of a window that starts at sample `start` is y = +0.0f, then for
 * k = 0 .. T - 1 in this order y = fmaf(h[k], x[start + t + d - k], y): one accumulator, one correctly
 * rounded fused multiply-add a tap, subnormals kept; a y that is zero is delivered as +0.0f.  Nothing
 * reassociates, splits, shortens or skips a step.  (The device adds steps of a zero tap times a
 * finite sample before and after the T: they change no accumulator but -0.0f, which only the
 * underflow of a negative product or sum to zero produces and the last clause removes on both
 * sides.)  d re-centres a linear-phase filter (d = (T - 1) / 2) or a response's direct path, so
 * that labels stay aligned; {1.0f} with d = 0 delivers the unfiltered crop bit for bit, which is how
 * one call mixes filtered and unfiltered crops.  The count is clipped to the stream as in _as:
 * n_samples is the part of [start, start + count) inside the stream at the delivered rate; elements
 * t < n follow the rule and read the stream's own samples before and after the window, zeros only
 * past the file's ends; with FLACGPU_DELIVER_PAD the rest of the window is +0.0f, without it the
 * rest is not written.  FLACGPU_SAMPLE_F32 is y; F16 and BF16 are y rounded to nearest-even as the
 * weighted mix's are (F16 is infinity from 65520 on); FLACGPU_SAMPLE_I32 is not offered.
 * flacgpu_fir_f32_host (host only) is this rule over one channel x[0 .. total), total <= 2^40,
 * count + n_taps - 1 < 2^31: y[t] for t < *n, +0.0f for the rest of the `count`.  It is a statement
 * of the rule for callers and tests, bit for bit what the device delivers; it is NOT a decode path.
 * The call.  `how` selects format, flags, masks or weights and rates exactly as
 * flacgpu_decode_windows_device_to does (K output channels); how->features must be NULL.  d_taps is
 * DEVICE memory the caller owns, taps_len floats, 4-byte aligned: a response bank is built once,
 * and the library neither copies nor inspects it.  Its taps must be finite: with a tap that is not,
 * the values are unspecified, but every write stays inside the window's elements.  filters[n_filters]
 * and window_filter[n_windows] are HOST arrays: window w goes through filters[window_filter[w]],
 * whose row r is the `taps` floats from d_taps + offset + r * taps; rows = 1: every output channel
 * uses row 0; rows = K: channel k uses row k (binaural or array responses after a mono-to-K mix).
 * FLACGPU_ERR_INVALID_INPUT before any device work: a NULL or misaligned d_taps or a NULL filters
 * where n_filters > 0, taps outside 1 .. 4096, delay >= taps, rows neither 1 nor K, reserved != 0,
 * offset + rows * taps > taps_len, window_filter[w] >= n_filters, count + taps - 1 >= 2^31,
 * FLACGPU_SAMPLE_I32 or an unknown format, how->features != NULL, and every argument error of the
 * call `how` describes.  Layout, TOO_SMALL (decided from n and the count as in _as, with K channels,
 * but on the device, after the span has been decoded),
 * BAD_INDEX and BAD_FRAME are as in _as; a window that is not OK writes nothing.  first_frame and
 * n_frames of a result are those of the covering frames of the samples
 * [start + d - (T - 1), start + count + d) inside the stream -- through the resampler's own reach
 * where the rates differ -- and BAD_FRAME is over them.  The call runs in two stages as _features
 * does: the window delivery itself leaves every window's span as F32 in scratch the context owns,
 * then one kernel runs the chains on the f32-input matrix instructions, whose accumulation is the
 * chain above bit for bit.  The one wait for the covers, the 65535-window limit, the chunks and the
 * stream semantics are those of flacgpu_decode_windows_device; the filter kernel is not timed. */
typedef struct { uint64_t offset; uint32_t taps, delay, rows, reserved; } flacgpu_fir;
int flacgpu_fir_f32_host(const float *x, uint64_t total, const float *taps, uint32_t n_taps, uint32_t delay,
                         uint64_t start, uint64_t count, float *y, uint64_t *n);
int flacgpu_decode_windows_device_fir(flacgpu_ctx *ctx, const uint8_t *d_data,
                                      uint32_t n_streams, const uint64_t *table_first,
                                      const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                      const flacgpu_index_result *d_index_results,
                                      const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                      uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                      const uint64_t *window_count,
                                      const flacgpu_window_delivery *how,
                                      const float *d_taps, uint64_t taps_len, uint32_t n_filters, const flacgpu_fir *filters,
                                      const uint32_t *window_filter,
                                      void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                      flacgpu_window_result *d_results, void *hip_stream);
/* The levels of sample windows: nothing is delivered but three numbers a block and channel.  A
 * stream's samples are the sign-extended integers x[t][c] of its depth.  The window [start, start +
 * count), clipped to n samples as in flacgpu_decode_windows_device, is cut by `hop` into ceil(n / hop)
 * blocks: block j holds the window's samples [j * hop, min((j + 1) * hop, n)), positions relative to
 * the window's start, the last block perhaps short.  Of every block and channel:
 *   peak    max |x| as uint32 (at 32 bits |-2^31| = 2^31 fits);
 *   sum     the sum of x as int64, exact (|sum| < 2^62 for hop < 2^31);
 *   energy  the sum of x^2 as an exact unsigned 128-bit integer (below 2^93), delivered as the double
 *           nearest to it, ties to even: the ONE rounding of the rule.  Below 2^64 it is the
 *           conversion of the integer; above, the integer is shifted right by s = its bit length - 64
 *           with every bit shifted out ORed into bit 0 (a sticky bit, 11 bits below the rounding
 *           position), converted to double (round to nearest-even) and scaled by 2^s (exact).
 *           Python's float(int) rounds the same way.
 * Record out_offsets[w] + j * C + c of each of d_peak, d_sum and d_energy (device memory, aligned to
 * their element) is block j, channel c of window w; out_offsets and out_caps count records.  Status
 * FLACGPU_WINDOW_TOO_SMALL where C * ceil(n / hop) > out_caps[w], decided before anything is decoded,
 * and nothing is written; a window with n = 0 is OK and writes nothing; n_samples of a result counts
 * the samples measured.  Everything else -- the tables, BAD_INDEX and BAD_FRAME (which write
 * nothing), windows that share streams and overlap, the one wait for hip_stream, the chunks of
 * max_frames_per_call, what is timed -- is as in flacgpu_decode_windows_device.  The accumulators are
 * integers and partial results combine exactly, so the bits do not depend on how the work is cut.
 * FLACGPU_ERR_INVALID_INPUT before any device work: hop == 0 or hop >= 2^31, a NULL output array,
 * one not aligned to its element size, out_offsets[w] + out_caps[w] passing 64 bits, and every
 * argument error of flacgpu_decode_windows_device.
 * flacgpu_levels_host (host only): the rule over n interleaved samples[n][channels] (any int32 is a
 * sample), ceil(n / hop) * channels records to each array; FLACGPU_ERR_INVALID_INPUT for hop == 0 or
 * >= 2^31, channels == 0, n > 2^40, or a NULL array with n > 0.  A statement of the rule for callers
 * and tests, bit for bit what the device writes; it is NOT a decode path. */
int flacgpu_levels_windows_device(flacgpu_ctx *ctx, const uint8_t *d_data,
                                  uint32_t n_streams, const uint64_t *table_first,
                                  const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                  const flacgpu_index_result *d_index_results,
                                  const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                  uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                  const uint64_t *window_count,
                                  uint32_t hop, uint32_t *d_peak, int64_t *d_sum, double *d_energy,
                                  const uint64_t *out_offsets, const uint64_t *out_caps,
                                  flacgpu_window_result *d_results, void *hip_stream);
int flacgpu_levels_host(const int32_t *samples, uint64_t n, uint32_t channels, uint32_t hop, uint32_t *peak,
                        int64_t *sum, double *energy);
/* Windows of whole files in host memory: window w is samples [window_start[w], + window_count[w])
 * of file window_file[w] (< n_files), delivered to pcm_out[w] (capacity pcm_cap[w]) with
 * n_samples[w].  Metadata is parsed on the host as in flacgpu_decode_files; the good files' frames
 * are uploaded into one device buffer, indexed and scanned there, and only the windows' bytes and
 * results come back.  status[w]: 0; the code flacgpu_decode_file gives for a file with bad
 * metadata, another channel count or depth; FLACGPU_ERR_INVALID_INPUT where the device index
 * refuses the file (there is no second try through the host index) or a covering frame is
 * damaged; FLACGPU_ERR_OUTPUT_TOO_SMALL.  No MD5: a window has none.  The return value is for the
 * call's own errors only. */
int flacgpu_decode_files_windows(flacgpu_ctx *ctx, uint32_t n_files, const void *const *flac, const size_t *len,
                                 uint32_t n_windows, const uint32_t *window_file, const uint64_t *window_start,
                                 const uint64_t *window_count, uint8_t *const *pcm_out, const size_t *pcm_cap,
                                 uint64_t *n_samples, int *status);

/* ---- Elements to PCM: the inverse of the delivery --------------------------- */
/* The rule.  An element of one of the four FLACGPU_SAMPLE_* formats becomes a sample of `bits` bits
 * (8, 16, 24, 32).  A float format: the element widened to f32 (exact), v = x * 2^(bits-1) (a power
 * of two: exact, or an overflow to +-inf), r = v rounded to an integer to nearest-even, clamped to
 * [-2^(bits-1), 2^(bits-1) - 1]; NaN gives 0 and -0.0 gives 0.  The clamp compares r with +-2^(bits-1)
 * as floats before the integer conversion (the upper limit is no f32 at 32 bits), so no conversion
 * sees a value out of range.  FLACGPU_SAMPLE_I32: the value, clamped to the same range.  An element
 * the clamp changed, or a NaN, is CLIPPED: 1.0 is, since a delivery only produces [-1, 1).  It is the
 * inverse of flacgpu_decode_windows_device_as wherever that conversion is exact: a sample delivered
 * as F32 (8, 16, 24 bits), as F16 or BF16 (8 bits) or as I32 (every depth) comes back as itself.
 * There is no dither and no noise shaping.
 * The PCM of a stream of T samples of C channels is T * C interleaved samples of bits / 8 bytes,
 * signed little-endian (8-bit included), at a 4-byte-aligned byte offset: what flacgpu_plan_create
 * takes.  The stream's last 32-bit word is written whole, its pad bytes zero; nothing past the
 * stream's length rounded up to 4 is touched.
 * flacgpu_pcm_from_elements_device: n_streams (at most 65535) streams in one launch, asynchronous on
 * hip_stream, on an encode context (flacgpu_open), whose channels and depth they have.  d_src is a
 * HOST array of device addresses, stream s's elements at any element alignment: channel c's sample
 * t at element c * plane_stride[s] + t with FLACGPU_DELIVER_PLANAR (plane_stride[s] >= samples[s];
 * plane_stride NULL: samples[s]), else at t * C + c.  Its PCM goes to d_pcm + pcm_offsets[s], the
 * offsets ascending, and d_clipped[s] (device, u64) is set to its count of clipped elements.
 * FLACGPU_ERR_INVALID_INPUT before any device work: a NULL pointer (ctx, an entry of d_src), a
 * decode-only context, an offset that is no multiple of 4, a stream that passes pcm_cap or runs into
 * the next one's offset, a format outside the four, a flag other than FLACGPU_DELIVER_PLANAR, a
 * plane stride below samples[s], more than 65535 streams.  The stream table lives in device memory
 * the context owns; the call waits for hip_stream only where that table has to grow.  Not timed. */
int flacgpu_pcm_from_elements_device(flacgpu_ctx *ctx, uint32_t n_streams, const void *const *d_src,
                                     const uint64_t *samples, const uint64_t *plane_stride,
                                     uint32_t sample_format, uint32_t flags, uint8_t *d_pcm,
                                     const uint64_t *pcm_offsets, uint64_t pcm_cap, uint64_t *d_clipped,
                                     void *hip_stream);
/* The same rule and the same PCM writer on the host, for one stream of `samples` samples of
 * `channels` channels in host memory, into pcm_out (4-byte aligned, capacity cap bytes: the PCM
 * length rounded up to 4, else FLACGPU_ERR_OUTPUT_TOO_SMALL); *clipped its count.  Needs no GPU.
 * FLACGPU_ERR_INVALID_INPUT: a NULL or unaligned pointer, channels outside 1..8, bits not 8, 16, 24
 * or 32, a bad format or flag, a plane stride below `samples`.  It is a statement of the rule for
 * callers and tests, bit for bit what the device writes; it is NOT a conversion path. */
int flacgpu_pcm_from_elements_host(const void *src, uint64_t samples, uint64_t plane_stride, uint32_t channels,
                                   uint32_t bits, uint32_t sample_format, uint32_t flags, uint8_t *pcm_out,
                                   size_t cap, uint64_t *clipped);

/* ---- Instrumentation ---------------------------------------------------- */
/* Kernel ids for flacgpu_kernel_time: frame analysis (4096-sample frames /
 * short frames), frame-size scan, frame packing (all frames), stream MD5. */
enum { FLACGPU_K_ANALYZE = 0, FLACGPU_K_ANALYZE_TAIL = 1, FLACGPU_K_SCAN = 2, FLACGPU_K_PACK = 3, FLACGPU_K_MD5 = 4,
       FLACGPU_K_DEC_PARSE = 5, FLACGPU_K_DEC_RECON = 6, /* the decoder's parse and reconstruct kernels */
       FLACGPU_K_INDEX = 7,                              /* the device frame index: all its stages as one launch */
       FLACGPU_K_COUNT = 8 };
/* When enabled, every launch of kernel k is bracketed by HIP events on the
 * stream it runs on; flacgpu_kernel_time returns the number of timed launches
 * and their summed device milliseconds since the last reset. */
int flacgpu_set_timing(flacgpu_ctx *ctx, int enable);
int flacgpu_kernel_time(flacgpu_ctx *ctx, int kernel, uint64_t *launches, double *total_ms);
int flacgpu_reset_timing(flacgpu_ctx *ctx);

/* Decision records (for parity tests): when enabled, each encode call also
 * stores one flacgpu_frame_record per frame, readable with
 * flacgpu_get_records after a synchronous call (flacgpu_encode_files: the
 * records of every file, file after file, in frame order). */
typedef struct {
    uint8_t type;       /* 0 CONSTANT, 1 VERBATIM, 2 FIXED, 3 LPC */
    uint8_t waste;
    uint8_t bits;       /* channel bit depth before waste removal */
    uint8_t order;
    uint8_t part_order;
    uint8_t method;     /* 0 FOUR, 1 FIVE */
    uint8_t written;    /* 1 if this candidate is in the bitstream */
    uint8_t pad;
    uint32_t pad2;
    uint64_t estimate;
    int64_t constant;
    uint8_t params[256];
    uint8_t lpc_precision;  /* LPC only */
    int8_t lpc_shift;
    uint8_t pad3[6];
    int32_t lpc_coefs[32];
} flacgpu_subframe_record;

typedef struct {
    uint32_t channel_code;
    uint32_t n_cand;
    uint32_t frame_bytes;
    uint32_t pad;
    flacgpu_subframe_record cand[8];
} flacgpu_frame_record;

int flacgpu_set_records(flacgpu_ctx *ctx, int enable);

/* Encode schedule (no reference counterpart: how the device runs the writeFrame loop).
 * ranges > 1: each call's full frames are encoded in that many frame ranges, the analysis of
 * range i+1 beside the scan + pack of range i on a second HIP stream, the two persistent grids
 * capped at ana_per_cu / pack_per_cu workgroups per CU (0 = no cap); calls with fewer than
 * ranges * min_frames full frames use fewer ranges.  ranges <= 1: one analysis, scan and pack
 * launch per call.  Output bytes are the same either way.  The overlapped schedule measured
 * slower than the serial one: ranges > 1 is FLACGPU_ERR_INVALID_CONFIG unless the library is a
 * diagnostic build (flacgpu_build_flags() & FLACGPU_BUILD_DIAG). */
int flacgpu_set_overlap(flacgpu_ctx *ctx, uint32_t ranges, uint32_t ana_per_cu, uint32_t pack_per_cu,
                        uint32_t min_frames);
int flacgpu_get_records(flacgpu_ctx *ctx, flacgpu_frame_record *out, uint64_t max_frames, uint64_t *n_frames);

#ifdef __cplusplus
}
#endif
#endif
