// fg_api.cpp -- the C ABI of libflacgpu.so (include/flacgpu.h): device
// memory planning, frame tables, launches and host <-> device movement for
// the gfx950 kernels (fg_device.hpp, fg_misc.hip).  No CPU encoding path exists: every
// encode goes through the HIP kernels, and a missing/unsupported device is an
// error (FLACGPU_ERR_DEVICE), never a fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/flacgpu.h"
#include "fg_common.hpp"
#include "fg_ctx.hpp"
#include "fg_internal.hpp"
#include "fg_layout.hpp"
#include "fg_md5_host.hpp"
#include "fg_quantize.hpp"

namespace fg {
hipError_t launch_stage(int stage, const EncodeArgs &a, bool full, uint32_t threads, uint32_t lds, hipStream_t st);
hipError_t launch_make_jobs(FrameJob *jobs, uint64_t n_samples, uint32_t block, uint32_t stride, uint64_t first,
                            uint32_t n_frames, hipStream_t st);
hipError_t launch_frame_totals(const EncodeArgs &a, hipStream_t st);
hipError_t launch_md5_streams(const uint8_t *base, const uint64_t *offs, const uint64_t *lens, const uint8_t *fin,
                              uint32_t n, Md5State *states, uint8_t *digests, hipStream_t st, int kernel, int prio);
hipError_t launch_advance_jobs(FrameJob *jobs, uint64_t n, uint64_t delta, hipStream_t st);
hipError_t launch_md5_blocks(uint32_t *state, const uint32_t *blocks, uint64_t n_blocks, hipStream_t st);
uint32_t md5_workgroups(uint32_t n, int kernel);
hipError_t launch_streaminfo_replay(const uint32_t *sizes, uint64_t n, uint32_t *minmax, hipStream_t st);
}  // namespace fg

using namespace fg;

static_assert(sizeof(SubRec) == sizeof(flacgpu_subframe_record), "record layout");
static_assert(sizeof(FrameRec) == sizeof(flacgpu_frame_record), "record layout");
static_assert(sizeof(Md5State) == sizeof(flacgpu_md5_state), "md5 state layout");

namespace {

constexpr uint32_t kCrcPoly = 0x8005u;

uint32_t crc_mulmod_host(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x10000u | kCrcPoly;
        if ((a >> i) & 1u) r ^= b;
    }
    return r & 0xFFFFu;
}
// z^e mod P
uint32_t crc_zpow(uint64_t e) {
    uint32_t result = 1, base = 2;  // z
    while (e) {
        if (e & 1) result = crc_mulmod_host(result, base);
        base = crc_mulmod_host(base, base);
        e >>= 1;
    }
    return result;
}

// z^e mod Q, Q = z^15 + z + 1 (a factor of P): the shift constants of the table-free CRC fold
// (fg_device.hpp crc_lane_q)
uint32_t q_zpow(uint64_t e) {
    const uint32_t r = crc_zpow(e);
    return (r & 0x8000u) ? r ^ 0x8003u : r;
}

// CRC-16 shift constants of the table-free fold (mod Q, fg_device.hpp crc_lane_q) for a pack
// kernel of T threads: thread t folds 2H words, followed by 2H (T - 1 - t) words and the CRC's
// z^16.  Row H - 1 for H = 1..hmax, and one spare entry so that a kernel not in use still has a table.
std::vector<uint16_t> crc_fold_shifts(uint32_t T, uint32_t hmax) {
    std::vector<uint16_t> pw((size_t)hmax * T + 1);
    for (uint32_t h = 1; h <= hmax; h++)
        for (uint32_t t = 0; t < T; t++) pw[(size_t)(h - 1) * T + t] = (uint16_t)q_zpow(16ull + 64ull * h * (T - 1u - t));
    return pw;
}

// The one reader of the knobs' environment variables (fg_geom.hpp: kKnobNames, knob_set)
Knobs knobs_from_env() {
    Knobs k;
    for (const char *name : kKnobNames)
        if (const char *e = std::getenv(name)) knob_set(k, name, e);
    return k;
}

}  // namespace

// device MD5 engine: whole blocks move through one bounded device buffer
constexpr uint64_t kMd5ChunkBlocks = (64ull << 20) / 64;
// overlapped encode: at most this many frame ranges per call (one ticket set of 4 u32 each)
constexpr uint32_t kOvlMaxChunks = 64;

Event fg::get_event(flacgpu_ctx *c) {
    Event ev;
    if (c->event_pool.empty()) {
        ev.create();
    } else {
        ev = std::move(c->event_pool.back());
        c->event_pool.pop_back();
    }
    return ev;
}

namespace {

void resolve_timing(flacgpu_ctx *c) {
    for (auto &t : c->pending) {
        hipEventSynchronize(t.stop.get());
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t.start.get(), t.stop.get()) == hipSuccess) {
            c->launches[t.kernel]++;
            c->ms[t.kernel] += ms;
        }
        c->event_pool.push_back(std::move(t.start));
        c->event_pool.push_back(std::move(t.stop));
    }
    c->pending.clear();
}

int validate(const flacgpu_config *cfg) {
    if (!cfg) return FLACGPU_ERR_INVALID_INPUT;
    if (cfg->channels < 1 || cfg->channels > 8) return FLACGPU_ERR_INVALID_CONFIG;
    const uint32_t b = cfg->bits_per_sample;
    if (b != 8 && b != 16 && b != 24 && b != 32) return FLACGPU_ERR_INVALID_CONFIG;  // frame_writer.zig:221-233
    if (cfg->block_size < 1 || cfg->block_size > kBlock) return FLACGPU_ERR_INVALID_CONFIG;
    if (cfg->max_rice_part_order > kMaxPartOrder) return FLACGPU_ERR_INVALID_CONFIG;  // rice.zig:13 buffers
    if (cfg->max_rice_param < 1 || cfg->max_rice_param > 30) return FLACGPU_ERR_INVALID_CONFIG;
    if (cfg->sample_rate >= (1u << 20)) return FLACGPU_ERR_INVALID_CONFIG;  // u20 (wav_reader.zig:98)
    // prediction: 0 = fixed only (the reference); 1..12 = LPC search up to that order
    // (build-defined extension; the FLAC subset limit)
    if (cfg->prediction > kLpcMax) return FLACGPU_ERR_INVALID_CONFIG;
    return FLACGPU_OK;
}

// What flacgpu_open and flacgpu_open_decoder share: the device checks, then a context with its
// shared part filled and its own stream.
int open_shared(int device, const StreamFormat &fmt, uint32_t max_frames_per_call, std::unique_ptr<flacgpu_ctx> &c) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return FLACGPU_ERR_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FLACGPU_ERR_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FLACGPU_ERR_DEVICE;  // code objects are gfx950-only
    HIPCHK(hipSetDevice(device));
    c.reset(new (std::nothrow) flacgpu_ctx());
    if (!c) return FLACGPU_ERR_OUT_OF_MEMORY;
    c->device = device;
    c->fmt = fmt;
    c->max_frames = max_frames_per_call ? max_frames_per_call : 32768u;
    c->k = knobs_from_env();
    if (c->stream.create() != hipSuccess) return FLACGPU_ERR_DEVICE;
    return flacgpu_md5_init(c.get());
}

// a device copy of a host table (none of an empty one)
template <class T>
hipError_t upload(DevBuf<T> &d, const std::vector<T> &h) {
    if (h.empty()) return hipSuccess;
    const hipError_t e = d.grow(h.size());
    return e != hipSuccess ? e : hipMemcpy(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// n zeroed elements
template <class T>
hipError_t zeroed(DevBuf<T> &d, uint64_t n) {
    const hipError_t e = d.grow(n);
    return e != hipSuccess ? e : hipMemset(d.get(), 0, n * sizeof(T));
}

uint64_t frames_for(uint64_t n_samples, uint32_t bs) { return (n_samples + bs - 1) / bs; }

// Queue the encode of n_full full frames (jobs[0..n_full)) and n_tail short ones
// (jobs[n_full..)): analysis (descriptors + exact sizes), scan (byte offsets),
// pack (frames written at their offsets in d_out).  full_slots: the slot of each full job
// (NULL: slot == job index); full jobs are in increasing slot order.
//
// Overlapped schedule (ovl_chunks > 1 and enough full frames): the tail frames are analysed
// first, then the full frames in K ranges: the analysis of range i+1 runs on `st` while the scan
// of range i's slot span (carried base: the bytes before it) and its pack run on the `ovl` stream, each
// persistent grid capped per CU so that an analysis grid and a pack grid share every CU (the
// analysis is VALU/issue bound, the pack LDS/latency bound).  Each range has its own set of
// frame-queue tickets.  Output bytes are identical to the serial schedule.
int encode_core(flacgpu_ctx *c, const uint8_t *d_pcm, const FrameJob *d_jobs, uint64_t n_full, uint64_t n_tail,
                uint8_t *d_desc, uint32_t *d_fbytes, uint8_t *d_out, uint64_t out_cap, uint64_t *d_offsets,
                uint64_t *d_total, hipStream_t st, const uint32_t *full_slots = nullptr) {
    const uint64_t n_frames = n_full + n_tail;
    if (n_frames == 0) {
        HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint64_t), st));
        return FLACGPU_OK;
    }
    if (n_frames > 0xFFFFFFFFull) return FLACGPU_ERR_INVALID_INPUT;
    EncState &e = *c->enc;
    EncodeArgs a{};
    a.pcm = d_pcm;
    a.channels = e.g.C;
    a.bits = e.g.bits;
    a.bytes_per_sample = e.g.B;
    a.sample_rate = e.cfg.sample_rate;
    a.stereo = e.g.stereo;
    a.max_part_order = e.cfg.max_rice_part_order;
    a.max_param = e.cfg.max_rice_param;
    a.lpc_order = e.cfg.prediction;
    a.block_size = e.cfg.block_size;
    a.desc = d_desc;
    a.desc_stride = e.g.desc_stride;
    a.image_bytes = e.g.image_bytes;
    a.stage_dbuf = e.g.stage_dbuf ? 1u : 0u;
    a.pack_dbuf = e.g.pack_dbuf ? 1u : 0u;
    a.enc_prio = c->k.enc_prio;
    a.ana1_variant = e.g.ana1_variant;
    a.frame_bytes = d_fbytes;
    a.offsets = d_offsets;
    a.out = d_out;
    a.out_cap = out_cap;
    a.err = e.d_err.get();
    a.work_ctr = e.d_ctr.get();
    a.crc_pow = e.d_crc_pow.get();
    a.crc_pow4 = e.d_crc_pow4.get();
    a.crc_hmax4 = e.g.crc_hmax4;
    a.crc_join = e.d_crc_join.get();
    a.crc_hmax = e.g.crc_hmax;
    a.records = e.records_on ? e.d_records.get() : nullptr;
    a.stamps = e.d_stamps.get();
    a.crc_x8 = e.d_crc_x8.get();

    // full-frame analysis of jobs[j0, j0 + n) with ticket set `set`
    auto analyze_full = [&](uint64_t j0, uint64_t n, uint32_t set, uint32_t per_cu, hipStream_t s) -> int {
        Timed t(c, FLACGPU_K_ANALYZE, s);
        EncodeArgs h = a;
        h.jobs = d_jobs + j0;
        h.n_jobs = (uint32_t)n;
        h.work_ctr = e.d_ctr.get() + kCtrSet * set;
        h.grid_reserve = e.grid_reserve;
        h.grid_per_cu = per_cu;
        if (e.g.ana_split) {
            h.channels = e.g.C / 2u;
            h.ch_split = 1;
            h.xcd_queue = c->k.xcd_queue ? ((c->k.split_jit & 1u) ? 3u : 1u) : 0u;
            HIPCHK(launch_stage(0, h, true, e.g.nt_split, e.g.lds_split, s));
            HIPCHK(launch_frame_totals(h, s));
        } else if (e.g.ana1) {
            HIPCHK(launch_stage(3, h, true, 64u, (uint32_t)Ana1Layout::total, s));
        } else {
            HIPCHK(launch_stage(0, h, true, e.g.nt, e.g.lds, s));
        }
        return FLACGPU_OK;
    };
    auto pack_full = [&](uint64_t j0, uint64_t n, uint32_t set, uint32_t per_cu, hipStream_t s) -> int {
        Timed t(c, FLACGPU_K_PACK, s);
        EncodeArgs h = a;
        h.jobs = d_jobs + j0;
        h.n_jobs = (uint32_t)n;
        h.work_ctr = e.d_ctr.get() + kCtrSet * set;
        h.grid_reserve = c->k.md5_reserve == 2 ? e.grid_reserve : 0u;
        h.grid_per_cu = per_cu;
        if (e.g.pack_split) {
            h.channels = e.g.C / 2u;
            h.ch_split = 1;
            h.image_bytes = e.g.image_split;
            h.crc_pow4 = e.d_crc_pows.get();
            h.crc_hmax4 = e.g.crc_hmaxs;
            h.xcd_queue = c->k.pack_xcdq ? ((c->k.split_jit & 2u) ? 3u : 1u) : 0u;
            HIPCHK(launch_stage(1, h, true, e.g.nt_psplit, e.g.lds_psplit, s));
        } else if (e.g.nt_pack4) {
            HIPCHK(launch_stage(1, h, true, e.g.nt_pack4, e.g.lds_pack4, s));
        } else {
            HIPCHK(launch_stage(1, h, true, e.g.nt_pack, e.g.lds_pack, s));
        }
        return FLACGPU_OK;
    };
    auto analyze_tail = [&](hipStream_t s) -> int {
        Timed t(c, FLACGPU_K_ANALYZE_TAIL, s);
        EncodeArgs h = a;
        h.jobs = d_jobs + n_full;
        h.n_jobs = (uint32_t)n_tail;
        HIPCHK(launch_stage(0, h, false, e.g.nt, e.g.lds_tail, s));
        return FLACGPU_OK;
    };
    auto pack_tail = [&](hipStream_t s) -> int {
        Timed t(c, FLACGPU_K_PACK, s);
        EncodeArgs h = a;
        h.jobs = d_jobs + n_full;
        h.n_jobs = (uint32_t)n_tail;
        HIPCHK(launch_stage(1, h, false, e.g.nt_pack, e.g.lds_pack, s));
        return FLACGPU_OK;
    };
    // the multi-workgroup scan's per-block sums: a grow-only context buffer
    const uint32_t nb = (uint32_t)((n_frames + 4095u) / 4096u);
    HIPCHK(c->d_scan_part.grow(nb));

    if (e.g.fused && n_full) {
        // fused: the tail frames' analysis first (it publishes their sizes), then analysis + pack of
        // the full frames in one kernel whose frames find their offsets by look-back, then the scan
        // (offsets of every frame, the total) and the tail frames' pack
        HIPCHK(e.d_status.grow(n_frames));
        HIPCHK(hipMemsetAsync(e.d_status.get(), 0, (size_t)n_frames * 8u, st));
        HIPCHK(hipMemsetAsync(e.d_ctr.get(), 0, 4, st));  // the fused kernel's frame queue (ticket 0)
        a.status = e.d_status.get();
        int rc;
        if (n_tail && (rc = analyze_tail(st))) return rc;
        {
            Timed t(c, FLACGPU_K_ANALYZE, st);
            EncodeArgs h = a;
            h.jobs = d_jobs;
            h.n_jobs = (uint32_t)n_full;
            h.stage_dbuf = 0;
            h.crc_pow4 = e.d_crc_powf.get();
            h.crc_hmax4 = e.g.crc_hmaxf;
            h.grid_reserve = e.grid_reserve;
            HIPCHK(launch_stage(2, h, true, 256u, e.g.lds_fused, st));
        }
        a.status = nullptr;
        {
            Timed t(c, FLACGPU_K_SCAN, st);
            HIPCHK(launch_scan(d_fbytes, d_offsets, d_total, (uint32_t)n_frames, c->d_scan_part.get(), st));
        }
        if (n_tail && (rc = pack_tail(st))) return rc;
        return FLACGPU_OK;
    }

    uint32_t K = e.ovl_chunks;
    if (K > kOvlMaxChunks) K = kOvlMaxChunks;
    while (K > 1 && n_full / K < e.ovl_min_frames) K--;
    if (K > 1) {
        int rc;
        if (n_tail && (rc = analyze_tail(st))) return rc;
        auto slot_of = [&](uint64_t j) -> uint64_t { return full_slots ? full_slots[j] : j; };
        auto j_begin = [&](uint32_t i) -> uint64_t { return n_full * i / K; };
        std::vector<Event> evs;
        auto release = [&]() {
            for (Event &ev : evs) c->event_pool.push_back(std::move(ev));
        };
        for (uint32_t i = 0; i < K; i++) {
            const uint64_t j0 = j_begin(i), j1 = j_begin(i + 1);
            if ((rc = analyze_full(j0, j1 - j0, i, e.ovl_ana, st))) return release(), rc;
            evs.push_back(get_event(c));
            const hipEvent_t ev = evs.back().get();
            if (!ev) return release(), FLACGPU_ERR_DEVICE;
            if (hipEventRecord(ev, st) != hipSuccess || hipStreamWaitEvent(e.ovl.get(), ev, 0) != hipSuccess)
                return release(), FLACGPU_ERR_DEVICE;
            // the slot span of range i: from its first full job (0 for the first range) to the next
            // range's first full job (n_frames for the last); tail slots inside it were analysed first
            const uint64_t s0 = i == 0 ? 0 : slot_of(j0), s1 = i + 1 == K ? n_frames : slot_of(j1);
            {
                Timed t(c, FLACGPU_K_SCAN, e.ovl.get());
                if (i == 0 && hipMemsetAsync(e.d_cum.get(), 0, sizeof(uint64_t), e.ovl.get()) != hipSuccess)
                    return release(), FLACGPU_ERR_DEVICE;
                const hipError_t se = launch_scan(d_fbytes + s0, d_offsets + s0, i + 1 == K ? d_total : e.d_cum.get() + i + 1,
                                                 (uint32_t)(s1 - s0), c->d_scan_part.get(), e.ovl.get(), e.d_cum.get() + i);
                if (se != hipSuccess) return release(), hip_err(se);
            }
            if ((rc = pack_full(j0, j1 - j0, i, e.ovl_pack, e.ovl.get()))) return release(), rc;
        }
        if (n_tail && (rc = pack_tail(e.ovl.get()))) return release(), rc;
        // st continues after the last pack
        evs.push_back(get_event(c));
        const hipEvent_t done = evs.back().get();
        if (!done) return release(), FLACGPU_ERR_DEVICE;
        if (hipEventRecord(done, e.ovl.get()) != hipSuccess || hipStreamWaitEvent(st, done, 0) != hipSuccess)
            return release(), FLACGPU_ERR_DEVICE;
        release();  // the waits are enqueued: the events can be recorded again
        return FLACGPU_OK;
    }

    int rc;
    if (n_full && (rc = analyze_full(0, n_full, 0, 0, st))) return rc;
    if (n_tail && (rc = analyze_tail(st))) return rc;
    {
        Timed t(c, FLACGPU_K_SCAN, st);
        HIPCHK(launch_scan(d_fbytes, d_offsets, d_total, (uint32_t)n_frames, c->d_scan_part.get(), st));
    }
    if (n_full && (rc = pack_full(0, n_full, 0, 0, st))) return rc;
    if (n_tail && (rc = pack_tail(st))) return rc;
    return FLACGPU_OK;
}

// The device error word, read back, as a return code (bit 0 invariant, bit 1 output too small); a
// set word is cleared for the next call.
int device_error_code(flacgpu_ctx *c, uint32_t err) {
    if (!err) return FLACGPU_OK;
    hipMemset(c->enc->d_err.get(), 0, 4);
    return (err & 2u) && !(err & 1u) ? FLACGPU_ERR_OUTPUT_TOO_SMALL : FLACGPU_ERR_INTERNAL;
}

int check_device_error(flacgpu_ctx *c) {
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, c->enc->d_err.get(), 4, hipMemcpyDeviceToHost));
    return device_error_code(c, err);
}

// Wait on the host for everything queued on st so far, through the context's event i (blocking
// sync: the thread sleeps).
hipError_t wait_host(flacgpu_ctx *c, hipStream_t st, int i) {
    const hipEvent_t ev = c->enc->hw[i].get();
    const hipError_t e = hipEventRecord(ev, st);
    return e != hipSuccess ? e : hipEventSynchronize(ev);
}

// check_device_error after a blocking wait on st (the pipelined path's end)
int check_device_error_on(flacgpu_ctx *c, hipStream_t st) {
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, c->enc->d_err.get(), 4, hipMemcpyDeviceToHost, st));
    HIPCHK(wait_host(c, st, 3));
    return device_error_code(c, err);
}

int fetch_records(flacgpu_ctx *c, uint64_t n_frames, hipStream_t st) {
    EncState &e = *c->enc;
    if (!e.records_on) return FLACGPU_OK;
    const size_t base = e.h_records.size();
    e.h_records.resize(base + n_frames);
    HIPCHK(hipMemcpyAsync(e.h_records.data() + base, e.d_records.get(), n_frames * sizeof(FrameRec),
                          hipMemcpyDeviceToHost, st));
    return FLACGPU_OK;
}

}  // namespace

// One chunk of at most max_frames frames (fg_internal.hpp): upload, encode, wait; the
// frames stay in the context's device output until ctx_download_chunk.
int fg::ctx_encode_chunk(flacgpu_ctx *c, const uint8_t *src, uint64_t ns, uint64_t first_number, uint64_t *total,
                         uint32_t *frame_bytes) {
    EncState &e = *c->enc;
    const hipStream_t st = c->stream.get();
    const uint32_t bs = e.cfg.block_size;
    const uint64_t nf = frames_for(ns, bs);
    if (nf > c->max_frames || !total) return FLACGPU_ERR_INVALID_INPUT;
    *total = 0;
    if (nf == 0) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(e.d_pcm.get(), src, ns * e.g.C * e.g.B, hipMemcpyHostToDevice, st));
    HIPCHK(launch_make_jobs(e.d_jobs.get(), ns, bs, (uint32_t)((uint64_t)bs * e.g.C * e.g.B), first_number, (uint32_t)nf, st));
    // frames with n == 4096 take the lane-owned-partition kernel, the rest the general one
    const uint64_t n_full = (bs == (uint32_t)kBlock) ? ns / kBlock : 0;
    int rc = encode_core(c, e.d_pcm.get(), e.d_jobs.get(), n_full, nf - n_full, e.d_desc.get(), e.d_fbytes.get(),
                         e.d_out.get(), e.d_out.cap(), e.d_offsets.get(), e.d_total.get(), st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(total, e.d_total.get(), 8, hipMemcpyDeviceToHost, st));
    if (frame_bytes) HIPCHK(hipMemcpyAsync(frame_bytes, e.d_fbytes.get(), nf * 4, hipMemcpyDeviceToHost, st));
    if ((rc = fetch_records(c, nf, st))) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return check_device_error(c);
}

int fg::ctx_download_chunk(flacgpu_ctx *c, uint8_t *out, uint64_t total) {
    if (!total) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(out, c->enc->d_out.get(), total, hipMemcpyDeviceToHost));
    return FLACGPU_OK;
}

uint32_t fg::ctx_max_frames(const flacgpu_ctx *c) { return c->max_frames; }
bool fg::ctx_decode_only(const flacgpu_ctx *c) { return !c->enc; }
bool fg::ctx_plain(const flacgpu_ctx *c) {
    const EncState &e = *c->enc;
    return !e.records_on && !c->timing && e.ovl_chunks <= 1 && !e.g.fused;
}
fg::CtxDevice fg::ctx_device(const flacgpu_ctx *c) {
    const EncState &e = *c->enc;
    return {c->device,      (void *)c->stream.get(), e.d_out.get(),           e.d_fbytes.get(), e.d_total.get(),
            e.d_out.cap(),  c->fmt.channels,         c->fmt.bytes_per_sample, c->fmt.max_block};
}
void fg::ctx_finish(flacgpu_ctx *c) { resolve_timing(c); }

extern "C" {

flacgpu_config flacgpu_config_default(uint32_t channels, uint32_t bits_per_sample, uint32_t sample_rate) {
    flacgpu_config c{};
    c.sample_rate = sample_rate;
    c.block_size = 4096;
    c.channels = (uint8_t)channels;
    c.bits_per_sample = (uint8_t)bits_per_sample;
    c.stereo_decorrelation = 1;
    c.max_rice_part_order = 8;
    c.max_rice_param = 30;
    c.prediction = 0;
    return c;
}

const char *flacgpu_strerror(int code) {
    switch (code) {
        case FLACGPU_OK: return "ok";
        case FLACGPU_ERR_INVALID_CONFIG: return "invalid config";
        case FLACGPU_ERR_INVALID_INPUT: return "invalid input";
        case FLACGPU_ERR_OUT_OF_MEMORY: return "out of memory";
        case FLACGPU_ERR_OUTPUT_TOO_SMALL: return "output buffer too small";
        case FLACGPU_ERR_DEVICE: return "HIP device error (no usable gfx950 device?)";
        case FLACGPU_ERR_INTERNAL: return "device-side invariant violated";
        default: return "unknown error";
    }
}

int flacgpu_abi_version(void) { return FLACGPU_ABI_VERSION; }

uint32_t flacgpu_build_flags(void) {
    uint32_t f = 0;
#if FG_DIAG
    f |= FLACGPU_BUILD_DIAG;
#endif
#ifdef FG_STAMPS
    f |= FLACGPU_BUILD_STAMPS;
#endif
    return f;
}

int flacgpu_get_config(const flacgpu_ctx *c, flacgpu_config *out) {
    if (!c || !out) return FLACGPU_ERR_INVALID_INPUT;
    // a decode-only context: its stream, block_size = max_block, the encode options zero
    const flacgpu_config dec{c->fmt.sample_rate, (uint16_t)c->fmt.max_block, (uint8_t)c->fmt.channels, (uint8_t)c->fmt.bits};
    *out = c->enc ? c->enc->cfg : dec;
    return FLACGPU_OK;
}

size_t flacgpu_reference_max_frame_bytes(const flacgpu_config *cfg) {
    if (!cfg) return 0;
    // maxFrameBytes(block_size, bit_depth, channels, compute_waste_bits=true) (encoder.zig:55-60,583-595)
    const size_t bps = cfg->channels == 2 ? cfg->bits_per_sample + 1u : cfg->bits_per_sample;
    return 14u + 8u * cfg->channels + (size_t)cfg->block_size * ((bps + 7) / 8) * (cfg->channels + 1u) + 2u;
}

size_t flacgpu_frame_bound_bytes(const flacgpu_config *cfg) {
    if (!cfg) return 0;
    const bool stereo = cfg->channels == 2 && cfg->stereo_decorrelation;
    return frame_bound_bytes(kBlock, cfg->channels, cfg->bits_per_sample, stereo);
}

int flacgpu_open(int device, const flacgpu_config *cfg, uint32_t max_frames_per_call, flacgpu_ctx **out) {
    if (!out) return FLACGPU_ERR_INVALID_INPUT;
    *out = nullptr;
    int rc = validate(cfg);
    if (rc) return rc;
    std::unique_ptr<flacgpu_ctx> c;
    const StreamFormat fmt{cfg->channels, cfg->bits_per_sample, cfg->bits_per_sample / 8u, cfg->sample_rate, cfg->block_size};
    if ((rc = open_shared(device, fmt, max_frames_per_call, c))) return rc;
    c->enc.reset(new (std::nothrow) EncState());
    if (!c->enc) return FLACGPU_ERR_OUT_OF_MEMORY;
    EncState &e = *c->enc;
    e.cfg = *cfg;
    if ((rc = enc_geometry(e.cfg, c->k, e.g))) return rc;  // a kernel's LDS does not fit
    const EncGeom &g = e.g;
    c->md5_kernel = g.md5_kernel;
    e.ovl_chunks = c->k.ovl_chunks;
    e.ovl_ana = c->k.ovl_ana;
    e.ovl_pack = c->k.ovl_pack;
    e.ovl_min_frames = c->k.ovl_min_frames;

    for (Stream *s : {&e.aux, &e.dl, &e.up, &e.ovl})
        if (s->create() != hipSuccess) return FLACGPU_ERR_DEVICE;
    const unsigned quiet = hipEventDisableTiming;
    const struct {
        Event *ev;
        size_t n;
        unsigned flags;
    } events[] = {{e.up_done, kPipeSets, quiet}, {e.set_done, kPipeSets, quiet}, {e.dl_done, kPipeSets, quiet},
                  {&e.fork, 1, quiet},           {&e.join, 1, quiet},
                  {e.hw, 4, c->k.spin_sync ? quiet : quiet | hipEventBlockingSync}};
    for (const auto &a : events)
        for (size_t i = 0; i < a.n; i++)
            if (a.ev[i].create(a.flags) != hipSuccess) return FLACGPU_ERR_DEVICE;

    // the CRC fold's shifts for each pack kernel's thread count (an unused one: hmax = 0)
    std::vector<uint16_t> pj(g.crc_hmax), x8(24);
    for (uint32_t h = 1; h <= g.crc_hmax; h++) pj[h - 1] = (uint16_t)q_zpow(32ull * h);
    for (uint32_t i = 0; i < 24; i++) x8[i] = (uint16_t)crc_zpow(8ull << i);
    if (g.crc_hmaxf) HIPCHK(upload(e.d_crc_powf, crc_fold_shifts(256u, g.crc_hmaxf)));
    HIPCHK(upload(e.d_crc_pows, crc_fold_shifts(g.nt_psplit, g.crc_hmaxs)));
    HIPCHK(upload(e.d_crc_x8, x8));
    HIPCHK(upload(e.d_crc_pow, crc_fold_shifts(g.nt_pack, g.crc_hmax)));
    HIPCHK(upload(e.d_crc_pow4, crc_fold_shifts(g.nt_pack4, g.crc_hmax4)));
    HIPCHK(upload(e.d_crc_join, pj));

    const uint64_t F = c->max_frames;
    HIPCHK(zeroed(e.d_err, 4));
    HIPCHK(zeroed(e.d_ctr, kCtrSet * kOvlMaxChunks));
    HIPCHK(e.d_cum.grow(kOvlMaxChunks + 1u));
    HIPCHK(e.d_jobs.grow(F));
    HIPCHK(e.d_desc.grow(F * (uint64_t)g.desc_stride));
    HIPCHK(e.d_fbytes.grow(F));
    HIPCHK(e.d_offsets.grow(F));
    HIPCHK(e.d_total.grow(kPipeSets + 1u));
    HIPCHK(e.d_pcm.grow(F * (uint64_t)kBlock * g.C * g.B + 64));
    HIPCHK(e.d_out.grow(F * (uint64_t)g.image_bytes));
    HIPCHK(e.d_md5_state.grow(4));
    HIPCHK(zeroed(e.d_stamps, 32));
    *out = c.release();
    return FLACGPU_OK;
}

// A context that only decodes: the shared part and nothing else -- the decoder allocates its
// scratch on first use (fg_dec_host.cpp), sized by max_block.  The limits are dec_geometry's: what
// k_dec_recon's planes hold.
int flacgpu_open_decoder(int device, uint32_t sample_rate, uint8_t channels, uint8_t bits_per_sample, uint32_t max_block,
                         uint32_t max_frames_per_call, flacgpu_ctx **out) {
    if (!out) return FLACGPU_ERR_INVALID_INPUT;
    *out = nullptr;
    if (sample_rate >= (1u << 20)) return FLACGPU_ERR_INVALID_CONFIG;  // u20, as flacgpu_open
    if (!dec_geometry(channels, bits_per_sample, max_block).ok) return FLACGPU_ERR_INVALID_CONFIG;
    std::unique_ptr<flacgpu_ctx> c;
    const StreamFormat fmt{channels, bits_per_sample, bits_per_sample / 8u, sample_rate, max_block};
    const int rc = open_shared(device, fmt, max_frames_per_call, c);
    if (rc) return rc;
    // the batched MD5 of decoded streams: the kernel enc_geometry picks for this depth
    c->md5_kernel = c->k.md5_kernel_set ? c->k.md5_kernel : (fmt.bytes_per_sample == 4u ? 2 : 1);
    *out = c.release();
    return FLACGPU_OK;
}

// Deleting the context releases everything it owns, in the order its members state (fg_ctx.hpp).
void flacgpu_close(flacgpu_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream.get());
    resolve_timing(c);
    delete c;
}

// Host buffers in, host buffers out, with both PCIe directions and the encode overlapped: the
// context's device buffers split into kPipeSets (3) chunk sets; chunk i+1 uploads on `up` while
// chunk i encodes on the context's stream and the frames of chunks i-1, i-2 download on `dl`, issued by one
// worker thread (pageable copies block the issuing thread, so the download needs a thread of its own).
// Output bytes and frame sizes are identical to the sequential loop; only the schedule differs.
// The input is a list of segments (files, flacgpu_encode_files): chunks never span two, and the
// pipeline runs on from one segment into the next instead of draining at each file's end.
struct PipeSeg {
    const uint8_t *src;
    uint64_t n_samples, first_frame_number;
    uint8_t *out;
    size_t out_cap, written;
    uint32_t *frame_bytes;  // may be NULL
};

// encode_pipelined could not start its download thread: nothing was queued, encode sequentially
constexpr int kNoWorker = -1000;

static int encode_pipelined(flacgpu_ctx *c, PipeSeg *segs, size_t nseg) {
    EncState &e = *c->enc;
    const hipStream_t st = c->stream.get();
    const uint32_t bs = e.cfg.block_size;
    const uint64_t stride = (uint64_t)bs * e.g.C * e.g.B;
    // chunks of at most 2048 frames (32 MiB of 16-bit stereo) so that long inputs keep both
    // PCIe directions busy; the thirds of the context's buffers hold one chunk each
    const uint32_t NS = c->k.pipe_sets;
    const uint64_t part = c->max_frames / NS;  // frames of one chunk set
    const uint64_t F = std::min<uint64_t>(part, 2048u);
    const uint64_t pcm_half = part * kBlock * e.g.C * e.g.B;  // 16-B multiple
    const uint64_t out_half = part * e.g.image_bytes;
    const uint64_t fb_half = part;
    const Event *done = e.set_done;  // a chunk set's encode finished
    struct Dl {
        int set;
        PipeSeg *sg;
        uint64_t frame0, nf;
    };
    // the download worker: one thread for the whole call, fed chunk by chunk
    std::mutex m;
    std::condition_variable cv;
    std::deque<Dl> q;
    uint64_t n_done = 0;  // downloads issued (in chunk order; dl_done[set] marks their completion)
    bool closing = false;
    int wrc = FLACGPU_OK;  // the first download error
    // One host wait per chunk: the download stream waits for the chunk's encode on the GPU, the
    // worker reads the chunk's byte count (it places the next chunk of the segment), then issues
    // the copies and records dl_done[set], on which the next encode into that set waits GPU-side.
    // (Round 4 slept on three blocking-sync events per chunk -- encode done, count, copies done --
    // and the 64-file batch moved 33 GB/s of PCM against 56 GB/s of chunked H2D beside D2H.)
    auto download = [&](const Dl &d) -> int {
        PipeSeg *sg = d.sg;
        uint64_t total = 0;
        if (hipSetDevice(c->device) != hipSuccess || hipStreamWaitEvent(e.dl.get(), done[d.set].get(), 0) != hipSuccess ||
            hipMemcpyAsync(&total, e.d_total.get() + d.set, 8, hipMemcpyDeviceToHost, e.dl.get()) != hipSuccess ||
            wait_host(c, e.dl.get(), 2) != hipSuccess)
            return FLACGPU_ERR_DEVICE;
        if (sg->written + total > sg->out_cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
        if ((sg->frame_bytes && hipMemcpyAsync(sg->frame_bytes + d.frame0, e.d_fbytes.get() + d.set * fb_half, d.nf * 4,
                                               hipMemcpyDeviceToHost, e.dl.get()) != hipSuccess) ||
            hipMemcpyAsync(sg->out + sg->written, e.d_out.get() + d.set * out_half, total, hipMemcpyDeviceToHost, e.dl.get()) !=
                hipSuccess ||
            hipEventRecord(e.dl_done[d.set].get(), e.dl.get()) != hipSuccess)
            return FLACGPU_ERR_DEVICE;
        sg->written += total;
        return FLACGPU_OK;
    };
    auto work = [&]() {
        for (;;) {
            Dl d;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return closing || !q.empty(); });
                if (q.empty()) return;
                d = q.front();
                q.pop_front();
            }
            const int r = wrc == FLACGPU_OK ? download(d) : FLACGPU_OK;  // after an error: drain only
            {
                std::lock_guard<std::mutex> lk(m);
                if (r != FLACGPU_OK && wrc == FLACGPU_OK) wrc = r;
                n_done++;
            }
            cv.notify_all();
        }
    };
    std::thread worker;
    try {
        worker = std::thread(work);
    } catch (const std::system_error &) {
        return kNoWorker;  // the caller encodes chunk by chunk on this thread instead
    }
    // wait (host) until at least `k` downloads have been issued; the first download error
    auto wait_done = [&](uint64_t k) -> int {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return n_done >= k || wrc != FLACGPU_OK; });
        return wrc;
    };
    int rc = FLACGPU_OK;
    uint64_t chunk = 0;  // chunks issued so far
    for (size_t si = 0; si < nseg && rc == FLACGPU_OK; si++) {
        PipeSeg *sg = &segs[si];
        sg->written = 0;
        const uint64_t total_frames = frames_for(sg->n_samples, bs);
        for (uint64_t frame0 = 0; frame0 < total_frames && rc == FLACGPU_OK; chunk++) {
            const int set = (int)(chunk % NS);
            const uint64_t nf = std::min<uint64_t>(F, total_frames - frame0);
            const uint64_t s0 = frame0 * bs;
            const uint64_t ns = std::min<uint64_t>(nf * bs, sg->n_samples - s0);
            uint8_t *dp = e.d_pcm.get() + set * pcm_half;
            // upload: the PCM part was last read by chunk i-3's encode (its `done` event, a GPU-side
            // wait); it runs beside chunk i-1's encode and the downloads of chunks i-2, i-3
            if ((chunk >= NS && hipStreamWaitEvent(e.up.get(), done[set].get(), 0) != hipSuccess) ||
                hipMemcpyAsync(dp, sg->src + s0 * e.g.C * e.g.B, ns * e.g.C * e.g.B, hipMemcpyHostToDevice, e.up.get()) !=
                    hipSuccess ||
                hipEventRecord(e.up_done[set].get(), e.up.get()) != hipSuccess) {
                rc = FLACGPU_ERR_DEVICE;
                break;
            }
            // the encode writes the output part chunk i-3's download reads: that download first
            // (issued by the worker: then the encode stream waits for its copies on the GPU)
            if (chunk >= NS && (rc = wait_done(chunk - NS + 1))) break;
            if ((chunk >= NS && hipStreamWaitEvent(st, e.dl_done[set].get(), 0) != hipSuccess) ||
                hipStreamWaitEvent(st, e.up_done[set].get(), 0) != hipSuccess ||
                launch_make_jobs(e.d_jobs.get(), ns, bs, (uint32_t)stride, sg->first_frame_number + frame0, (uint32_t)nf,
                                 st) != hipSuccess) {
                rc = FLACGPU_ERR_DEVICE;
                break;
            }
            const uint64_t n_full = (bs == (uint32_t)kBlock) ? ns / kBlock : 0;
            if ((rc = encode_core(c, dp, e.d_jobs.get(), n_full, nf - n_full, e.d_desc.get(), e.d_fbytes.get() + set * fb_half,
                                  e.d_out.get() + set * out_half, out_half, e.d_offsets.get(), e.d_total.get() + set, st)))
                break;
            if (hipEventRecord(done[set].get(), st) != hipSuccess) {
                rc = FLACGPU_ERR_DEVICE;
                break;
            }
            {
                std::lock_guard<std::mutex> lk(m);
                q.push_back(Dl{set, sg, frame0, nf});
            }
            cv.notify_all();
            frame0 += nf;
        }
    }
    {
        std::lock_guard<std::mutex> lk(m);
        closing = true;
    }
    cv.notify_all();
    worker.join();
    if (rc == FLACGPU_OK) rc = wrc;
    const hipError_t se = hipStreamSynchronize(e.dl.get());  // the last chunks' copies
    if (rc == FLACGPU_OK && se != hipSuccess) rc = FLACGPU_ERR_DEVICE;
    if (rc) {
        hipStreamSynchronize(e.up.get());
        hipStreamSynchronize(st);
        return rc;
    }
    return check_device_error_on(c, st);
}

}  // extern "C"

int fg::ctx_encode_segments(flacgpu_ctx *c, uint32_t n, const uint8_t *const *src, const uint64_t *n_samples,
                            uint8_t *const *out, const size_t *out_cap, size_t *out_len, uint32_t *const *frame_bytes) {
    EncState &e = *c->enc;
    HIPCHK(hipSetDevice(c->device));
    // contexts the pipeline cannot serve (one frame per call, decision records on), or no thread
    // for its downloads: each file through flacgpu_encode_frames, which is what
    // flacgpu_encode_file does for them
    auto one_by_one = [&]() -> int {
        for (uint32_t i = 0; i < n; i++) out_len[i] = 0;
        // with decision records on, the records of EVERY file are kept, file after file in frame
        // order (flacgpu_get_records), not only the last file's
        if (e.records_on) e.h_records.clear();
        e.records_keep = true;
        for (uint32_t i = 0; i < n; i++) {
            const int r = flacgpu_encode_frames(c, src[i], e.g.B, n_samples[i], 0, out[i], out_cap[i], &out_len[i],
                                                frame_bytes ? frame_bytes[i] : nullptr);
            if (r) {
                e.records_keep = false;
                for (uint32_t j = 0; j < n; j++) out_len[j] = 0;
                return r;
            }
        }
        e.records_keep = false;
        return FLACGPU_OK;
    };
    if (c->max_frames < c->k.pipe_sets || e.records_on) return one_by_one();
    std::vector<PipeSeg> segs;
    try {
        segs.resize(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t nf = frames_for(n_samples[i], e.cfg.block_size);
        if (nf && nf - 1 > (1ull << 36) - 1) return FLACGPU_ERR_INVALID_INPUT;  // u36 frame numbers
        segs[i] = PipeSeg{src[i], n_samples[i], 0, out[i], out_cap[i], 0, frame_bytes ? frame_bytes[i] : nullptr};
    }
    const int rc = encode_pipelined(c, segs.data(), n);
    if (rc == kNoWorker) return one_by_one();
    resolve_timing(c);
    for (uint32_t i = 0; i < n; i++) out_len[i] = rc ? 0 : segs[i].written;
    return rc;
}

extern "C" {

int flacgpu_encode_frames(flacgpu_ctx *c, const void *pcm, uint32_t bytes_per_sample, uint64_t n_samples,
                          uint64_t first_frame_number, uint8_t *out, size_t out_cap, size_t *out_len,
                          uint32_t *frame_bytes) {
    if (!c || (!pcm && n_samples) || !out_len) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);
    EncState &e = *c->enc;
    if (bytes_per_sample != e.g.B) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    *out_len = 0;
    const uint32_t bs = e.cfg.block_size;
    const uint64_t total_frames = frames_for(n_samples, bs);
    // frame numbers are u36 (frame_writer.zig:153, wav2flac.zig:75)
    if (total_frames && (first_frame_number >= (1ull << 36) || total_frames - 1 > (1ull << 36) - 1 - first_frame_number))
        return FLACGPU_ERR_INVALID_INPUT;
    const uint8_t *src = (const uint8_t *)pcm;
    uint64_t frame0 = 0;
    size_t written = 0;
    if (e.records_on && !e.records_keep) e.h_records.clear();
    if (!e.records_on && c->max_frames >= c->k.pipe_sets &&
        total_frames > std::min<uint64_t>(c->max_frames / c->k.pipe_sets, 2048u)) {
        PipeSeg seg{src, n_samples, first_frame_number, out, out_cap, 0, frame_bytes};
        const int rc = encode_pipelined(c, &seg, 1);
        if (rc != kNoWorker) {
            resolve_timing(c);
            if (rc == FLACGPU_OK) *out_len = seg.written;
            return rc;
        }
    }
    while (frame0 < total_frames) {
        const uint64_t nf = std::min<uint64_t>(c->max_frames, total_frames - frame0);
        const uint64_t s0 = frame0 * bs;
        const uint64_t ns = std::min<uint64_t>(nf * bs, n_samples - s0);
        uint64_t total = 0;
        int rc = fg::ctx_encode_chunk(c, src + s0 * e.g.C * e.g.B, ns, first_frame_number + frame0, &total,
                                      frame_bytes ? frame_bytes + frame0 : nullptr);
        if (rc) return rc;
        if (written + total > out_cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
        if ((rc = fg::ctx_download_chunk(c, out + written, total))) return rc;
        written += total;
        frame0 += nf;
    }
    resolve_timing(c);
    *out_len = written;
    return FLACGPU_OK;
}

int flacgpu_encode_frame_planar(flacgpu_ctx *c, const int32_t *const planes[8], uint32_t n, uint64_t frame_number,
                                uint8_t *out, size_t out_cap, uint32_t *frame_bytes) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);
    EncState &e = *c->enc;
    if (!planes || !out || n == 0 || n > e.cfg.block_size) return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t ch = 0; ch < e.g.C; ch++)
        if (!planes[ch]) return FLACGPU_ERR_INVALID_INPUT;
    // Encoder.samples[ch][0..n] -> the little-endian interleaved layout the kernels stage
    std::vector<uint8_t> pcm((size_t)n * e.g.C * e.g.B + 4);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t ch = 0; ch < e.g.C; ch++) {
            const uint32_t v = (uint32_t)planes[ch][i];
            uint8_t *d = &pcm[((size_t)i * e.g.C + ch) * e.g.B];
            for (uint32_t k = 0; k < e.g.B; k++) d[k] = (uint8_t)(v >> (8 * k));
        }
    size_t len = 0;
    uint32_t fb = 0;
    int rc = flacgpu_encode_frames(c, pcm.data(), e.g.B, n, frame_number, out, out_cap, &len, &fb);
    if (rc) return rc;
    if (frame_bytes) *frame_bytes = fb;
    return FLACGPU_OK;
}

// ---- streaming MD5 --------------------------------------------------------
int flacgpu_md5_set_engine(flacgpu_ctx *c, int engine) {
    if (!c || (engine != FLACGPU_MD5_HOST && engine != FLACGPU_MD5_DEVICE)) return FLACGPU_ERR_INVALID_INPUT;
    if (engine == FLACGPU_MD5_DEVICE) FG_ENCODER_ONLY(c);  // the device engine's state is an encode buffer
    c->md5_engine = engine;
    return flacgpu_md5_init(c);
}

int flacgpu_md5_get_engine(const flacgpu_ctx *c) { return c ? c->md5_engine : FLACGPU_ERR_INVALID_INPUT; }

int flacgpu_md5_init(flacgpu_ctx *c) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    c->host_md5.reset();
    if (c->md5_engine != FLACGPU_MD5_DEVICE) return FLACGPU_OK;
    EncState &e = *c->enc;
    e.md5_fill = 0;
    e.md5_len = 0;
    const uint32_t iv[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(e.d_md5_state.get(), iv, 16, hipMemcpyHostToDevice));
    return FLACGPU_OK;
}

// device engine: whole blocks through one bounded buffer (kMd5ChunkBlocks per launch)
static int md5_push_blocks(flacgpu_ctx *c, const uint8_t *p, uint64_t nblocks) {
    if (!nblocks) return FLACGPU_OK;
    EncState &e = *c->enc;
    HIPCHK(e.d_md5_blocks.grow(kMd5ChunkBlocks * 16u));  // the first call allocates
    for (uint64_t b = 0; b < nblocks; b += kMd5ChunkBlocks) {
        const uint64_t nb = std::min<uint64_t>(kMd5ChunkBlocks, nblocks - b);
        HIPCHK(hipMemcpyAsync(e.d_md5_blocks.get(), p + b * 64, nb * 64, hipMemcpyHostToDevice, c->stream.get()));
        {
            Timed t(c, FLACGPU_K_MD5, c->stream.get());
            HIPCHK(launch_md5_blocks(e.d_md5_state.get(), e.d_md5_blocks.get(), nb, c->stream.get()));
        }
        HIPCHK(hipStreamSynchronize(c->stream.get()));
    }
    return FLACGPU_OK;
}

int flacgpu_md5_update(flacgpu_ctx *c, const void *data, size_t len) {
    if (!c || (!data && len)) return FLACGPU_ERR_INVALID_INPUT;
    if (c->md5_engine != FLACGPU_MD5_DEVICE) {
        c->host_md5.update(data, len);
        return FLACGPU_OK;
    }
    EncState &e = *c->enc;
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *p = (const uint8_t *)data;
    e.md5_len += len;
    if (e.md5_fill) {
        const size_t take = std::min<size_t>(64 - e.md5_fill, len);
        std::memcpy(e.md5_buf + e.md5_fill, p, take);
        e.md5_fill += (uint32_t)take;
        p += take;
        len -= take;
        if (e.md5_fill == 64) {
            int rc = md5_push_blocks(c, e.md5_buf, 1);
            if (rc) return rc;
            e.md5_fill = 0;
        }
    }
    const uint64_t nb = len / 64;
    int rc = md5_push_blocks(c, p, nb);
    if (rc) return rc;
    p += nb * 64;
    len -= nb * 64;
    std::memcpy(e.md5_buf, p, len);
    e.md5_fill = (uint32_t)len;
    return FLACGPU_OK;
}

int flacgpu_md5_final(flacgpu_ctx *c, uint8_t digest[16]) {
    if (!c || !digest) return FLACGPU_ERR_INVALID_INPUT;
    if (c->md5_engine != FLACGPU_MD5_DEVICE) {
        c->host_md5.final(digest);
        return FLACGPU_OK;
    }
    EncState &e = *c->enc;
    HIPCHK(hipSetDevice(c->device));
    uint8_t tail[128] = {};
    std::memcpy(tail, e.md5_buf, e.md5_fill);
    tail[e.md5_fill] = 0x80;
    const uint32_t nb = e.md5_fill < 56 ? 1 : 2;
    const uint64_t bits = e.md5_len * 8;
    for (int i = 0; i < 8; i++) tail[nb * 64 - 8 + i] = (uint8_t)(bits >> (8 * i));
    int rc = md5_push_blocks(c, tail, nb);
    if (rc) return rc;
    uint32_t st[4];
    HIPCHK(hipMemcpy(st, e.d_md5_state.get(), 16, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) digest[4 * i + j] = (uint8_t)(st[i] >> (8 * j));
    resolve_timing(c);
    return flacgpu_md5_init(c);
}

void flacgpu_md5_state_init(flacgpu_md5_state *s, size_t n) {
    for (size_t i = 0; s && i < n; i++) {
        s[i].h[0] = 0x67452301u;
        s[i].h[1] = 0xefcdab89u;
        s[i].h[2] = 0x98badcfeu;
        s[i].h[3] = 0x10325476u;
        s[i].bytes = 0;
        s[i].finished = 0;
        s[i].reserved = 0;
    }
}

int flacgpu_md5_many(uint32_t n, const void *const *data, const uint64_t *lens, const uint8_t *final,
                     flacgpu_md5_state *states, uint8_t *digests) {
    if (n && (!data || !lens)) return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t i = 0; i < n; i++) {
        const bool fin = !final || final[i];
        // the state carries no partial block: a chain continues only after whole 64-byte blocks
        if (!fin && (!states || lens[i] % 64u)) return FLACGPU_ERR_INVALID_INPUT;
        if (lens[i] && !data[i]) return FLACGPU_ERR_INVALID_INPUT;
    }
    std::vector<fg::HostMd5> hs;
    std::vector<fg::HostMd5 *> hp;
    std::vector<const uint8_t *> ps;
    std::vector<size_t> ls;
    std::vector<uint32_t> idx;
    try {
        hs.resize(n);
        hp.reserve(n);
        ps.reserve(n);
        ls.reserve(n);
        idx.reserve(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t i = 0; i < n; i++) {
        const bool fin = !final || final[i];
        if (states && (states[i].finished & 1u)) {
            // a finished chain stays as it is; a final segment reports its digest again
            if (fin && digests)
                for (int w = 0; w < 4; w++)
                    for (int b = 0; b < 4; b++) digests[16 * i + 4 * w + b] = (uint8_t)(states[i].h[w] >> (8 * b));
            continue;
        }
        if (states) {
            std::memcpy(hs[i].h, states[i].h, 16);
            hs[i].bytes = states[i].bytes;
        }
        hp.push_back(&hs[i]);
        ps.push_back((const uint8_t *)data[i]);
        ls.push_back((size_t)lens[i]);
        idx.push_back(i);
    }
    fg::md5_pool_update_many(hp.data(), ps.data(), ls.data(), hp.size());
    for (uint32_t i : idx) {
        const bool fin = !final || final[i];
        const uint64_t bytes = hs[i].bytes;
        uint8_t dg[16];
        if (fin) {
            hs[i].final(dg);
            if (digests) std::memcpy(digests + 16 * (size_t)i, dg, 16);
        }
        if (states) {
            if (fin)
                for (int w = 0; w < 4; w++)
                    states[i].h[w] = (uint32_t)dg[4 * w] | (uint32_t)dg[4 * w + 1] << 8 | (uint32_t)dg[4 * w + 2] << 16 |
                                     (uint32_t)dg[4 * w + 3] << 24;
            else
                std::memcpy(states[i].h, hs[i].h, 16);
            states[i].bytes = bytes;
            states[i].finished = fin ? 1u : 0u;
            states[i].reserved = 0;
        }
    }
    return FLACGPU_OK;
}

int flacgpu_md5_plan_host(const flacgpu_plan *p, const void *h_pcm, flacgpu_md5_state *states, uint8_t *digests) {
    if (!p || (p->n_streams && !h_pcm)) return FLACGPU_ERR_INVALID_INPUT;
    std::vector<const void *> ptrs;
    try {
        ptrs.resize(p->n_streams);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t s = 0; s < p->n_streams; s++) ptrs[s] = (const uint8_t *)h_pcm + p->h_md5_offs[s];
    return flacgpu_md5_many(p->n_streams, ptrs.data(), p->h_md5_lens.data(),
                            p->h_md5_fin.empty() ? nullptr : p->h_md5_fin.data(), states, digests);
}

// The engine rates: device figures from bench.py's stream_curve on MI355X (DESIGN.md section 5.2:
// one lane per stream at ~72 MB/s beside the encode, at most ~600 GB/s over the chip -- 16384
// streams: 4.3 GB of MD5 in 7.1 ms); host figures measured on this machine the first time the
// choice is made (fg::md5_measure_rates: the fixed 0.95 GB/s-per-chain constants of round 4 were
// 1.6-3x off on the driver's box, where the picker then chose the slower engine).
static std::mutex g_rates_mu;
static flacgpu_md5_rates g_rates{};
static bool g_rates_set = false;

static flacgpu_md5_rates md5_rates() {
    std::lock_guard<std::mutex> lk(g_rates_mu);
    if (!g_rates_set) {
        flacgpu_md5_rates r{};
        const bool contended = fg::md5_measure_rates(r.host_chain, r.host_chains);
        r.device_lane = 72e6;
        r.device_chip = 600e9;
        r.host_workers = fg::md5_pool_workers();
        r.measured = contended ? 3 : 1;
        g_rates = r;
        g_rates_set = true;
    }
    return g_rates;
}

int flacgpu_md5_get_rates(flacgpu_md5_rates *out) {
    if (!out) return FLACGPU_ERR_INVALID_INPUT;
    *out = md5_rates();
    return FLACGPU_OK;
}

int flacgpu_md5_set_rates(const flacgpu_md5_rates *r) {
    // the whole struct is validated on a local copy first: a rejected call leaves the rates in use
    // (measured or set earlier) as they were
    flacgpu_md5_rates v{};
    if (r) {
        v = *r;
        for (double x : v.host_chain)
            if (!(x > 0)) return FLACGPU_ERR_INVALID_INPUT;
        if (!(v.device_lane > 0) || !(v.device_chip > 0) || v.host_workers < 0) return FLACGPU_ERR_INVALID_INPUT;
        if (!v.host_chains[0])
            for (uint32_t i = 0; i < 4; i++) v.host_chains[i] = i + 1u;
        for (uint32_t i = 1; i < 4; i++)
            if (v.host_chains[i] <= v.host_chains[i - 1]) return FLACGPU_ERR_INVALID_INPUT;
        v.measured = 2;
    }
    std::lock_guard<std::mutex> lk(g_rates_mu);
    if (r) g_rates = v;
    g_rates_set = r != nullptr;
    return FLACGPU_OK;
}

int flacgpu_md5_engine_for(uint32_t n_streams, uint64_t max_len, uint64_t total_len) {
    if (!n_streams || !total_len) return FLACGPU_MD5_DEVICE;
    const flacgpu_md5_rates r = md5_rates();
    const double n = n_streams;
    const double t_dev = std::max((double)max_len / r.device_lane, (double)total_len / r.device_chip);
    double t_host;
    if (r.host_workers <= 0) {
        t_host = (double)total_len / r.host_chain[0];  // no pool: the caller hashes chain after chain
    } else {
        // k chains per worker: the per-worker rate interpolated between the measured points, flat
        // past the last (more chains are time-sliced); with fewer chains than workers, one chain
        // each on n workers
        const double w = r.host_workers;
        const double k = std::ceil(n / w);
        double rw = r.host_chain[3];
        for (int i = 0; i < 4; i++) {
            const double pk = r.host_chains[i] ? r.host_chains[i] : i + 1.0;
            if (k <= pk) {
                if (i == 0) {
                    rw = r.host_chain[0];
                } else {
                    const double p0 = r.host_chains[i - 1] ? r.host_chains[i - 1] : i;
                    rw = r.host_chain[i - 1] + (r.host_chain[i] - r.host_chain[i - 1]) * (k - p0) / (pk - p0);
                }
                break;
            }
        }
        t_host = std::max((double)total_len / (rw * std::min(n, w)), (double)max_len / r.host_chain[0]);
    }
    return t_host < t_dev ? FLACGPU_MD5_HOST : FLACGPU_MD5_DEVICE;
}

int flacgpu_plan_md5_engine(const flacgpu_plan *p) {
    if (!p || !p->n_streams) return FLACGPU_MD5_DEVICE;
    return flacgpu_md5_engine_for(p->n_streams, p->md5_max_len, p->md5_total);
}

// ---- plans (device-resident batches of independent streams) --------------
int flacgpu_plan_create_segments(flacgpu_ctx *c, uint32_t n_streams, const uint64_t *offs, const uint64_t *samples,
                                 uint32_t bytes_per_sample, const uint64_t *first_frame_numbers,
                                 const uint8_t *final_segment, flacgpu_plan **out) {
    if (!c || !out) return FLACGPU_ERR_INVALID_INPUT;
    *out = nullptr;
    FG_ENCODER_ONLY(c);  // no plan exists on a decode-only context, so nothing that takes one runs on it
    EncState &e = *c->enc;
    if ((n_streams && (!offs || !samples)) || bytes_per_sample != e.g.B) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t bs = e.cfg.block_size;
    const uint64_t fbytes_in = (uint64_t)e.g.C * e.g.B;
    std::vector<FrameJob> full, tail;
    std::vector<uint64_t> lens(n_streams);
    uint64_t max_number = 0;
    // validate everything before any allocation
    for (uint32_t s = 0; s < n_streams; s++) {
        // stream starts: 4-byte aligned (the kernels' dword / 16-byte vector loads)
        if (offs[s] & 3u) return FLACGPU_ERR_INVALID_INPUT;
        const uint64_t nf = frames_for(samples[s], bs);
        const uint64_t f0 = first_frame_numbers ? first_frame_numbers[s] : 0;
        if (nf && (f0 >= (1ull << 36) || nf - 1 > (1ull << 36) - 1 - f0)) return FLACGPU_ERR_INVALID_INPUT;  // u36
        if (nf) max_number = std::max(max_number, f0 + nf - 1);
        // a segment that the stream continues after: whole frames and whole MD5 blocks
        if (final_segment && !final_segment[s] && (samples[s] % bs || (samples[s] * fbytes_in) % 64))
            return FLACGPU_ERR_INVALID_INPUT;
    }
    std::unique_ptr<flacgpu_plan> p(new (std::nothrow) flacgpu_plan());
    if (!p) return FLACGPU_ERR_OUT_OF_MEMORY;
    p->ctx = c;
    p->n_streams = n_streams;
    p->B = bytes_per_sample;
    p->max_number = max_number;
    uint64_t slot = 0;
    try {
        p->first_frame.resize(n_streams);
        for (uint32_t s = 0; s < n_streams; s++) {
            p->first_frame[s] = slot;
            lens[s] = samples[s] * fbytes_in;
            p->md5_max_len = std::max(p->md5_max_len, lens[s]);
            p->md5_total += lens[s];
            const uint64_t nf = frames_for(samples[s], bs);
            const uint64_t f0 = first_frame_numbers ? first_frame_numbers[s] : 0;
            for (uint64_t f = 0; f < nf; f++, slot++) {
                FrameJob j;
                j.pcm_off = offs[s] + f * bs * fbytes_in;
                j.number = f0 + f;
                j.n = (uint32_t)std::min<uint64_t>(bs, samples[s] - f * bs);
                j.slot = (uint32_t)slot;
                (j.n == (uint32_t)kBlock ? full : tail).push_back(j);
                if (j.n == (uint32_t)kBlock) p->full_slots.push_back(j.slot);
            }
        }
        full.insert(full.end(), tail.begin(), tail.end());
        p->h_md5_offs.assign(offs, offs + n_streams);
        p->h_md5_lens = lens;
        if (final_segment) p->h_md5_fin.assign(final_segment, final_segment + n_streams);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    p->n_frames = slot;
    p->n_full = full.size() - tail.size();
    p->n_tail = tail.size();
    p->out_bound = slot * (uint64_t)e.g.image_bytes;
    if (slot > 0xFFFFFFFFull) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(upload(p->d_jobs, full));
    if (n_streams) {
        HIPCHK(p->d_md5_offs.grow(n_streams));
        HIPCHK(hipMemcpy(p->d_md5_offs.get(), offs, n_streams * 8, hipMemcpyHostToDevice));
        HIPCHK(upload(p->d_md5_lens, lens));
        if (final_segment) {
            HIPCHK(p->d_md5_fin.grow(n_streams));
            HIPCHK(hipMemcpy(p->d_md5_fin.get(), final_segment, n_streams, hipMemcpyHostToDevice));
        }
    }
    if (slot > c->max_frames) HIPCHK(p->d_desc.grow(slot * (uint64_t)e.g.desc_stride));
    *out = p.release();
    return FLACGPU_OK;
}

int flacgpu_plan_create(flacgpu_ctx *c, uint32_t n_streams, const uint64_t *offs, const uint64_t *samples,
                        uint32_t bytes_per_sample, flacgpu_plan **out) {
    return flacgpu_plan_create_segments(c, n_streams, offs, samples, bytes_per_sample, nullptr, nullptr, out);
}

void flacgpu_plan_destroy(flacgpu_plan *p) { delete p; }

uint64_t flacgpu_plan_frames(const flacgpu_plan *p) { return p ? p->n_frames : 0; }
uint64_t flacgpu_plan_out_bound(const flacgpu_plan *p) { return p ? p->out_bound : 0; }
uint64_t flacgpu_plan_stream_first_frame(const flacgpu_plan *p, uint32_t s) {
    return (p && s < p->n_streams) ? p->first_frame[s] : 0;
}

int flacgpu_plan_advance(flacgpu_plan *p, uint64_t frames, void *hip_stream) {
    if (!p) return FLACGPU_ERR_INVALID_INPUT;
    if (!frames || !p->n_frames) return FLACGPU_OK;
    if (frames > (1ull << 36) - 1 - p->max_number) return FLACGPU_ERR_INVALID_INPUT;  // u36 frame numbers
    flacgpu_ctx *c = p->ctx;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, hip_stream);
    HIPCHK(launch_advance_jobs(p->d_jobs.get(), p->n_frames, frames, st));
    p->max_number += frames;
    return FLACGPU_OK;
}

int flacgpu_encode_plan_device_ex(flacgpu_ctx *c, const flacgpu_plan *p, const void *d_pcm, uint8_t *d_out,
                                  uint64_t out_cap, uint32_t *d_frame_bytes, uint64_t *d_frame_offsets,
                                  uint64_t *d_total, flacgpu_md5_state *d_md5_state, uint8_t *d_md5, void *hip_stream,
                                  void *md5_stream) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);
    EncState &e = *c->enc;
    if (!p || p->ctx != c || !d_pcm || !d_out || !d_frame_bytes || !d_frame_offsets || !d_total)
        return FLACGPU_ERR_INVALID_INPUT;
    // a stream that continues past this segment has no digest yet: its state must be carried
    if (p->d_md5_fin.get() && d_md5 && !d_md5_state) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, hip_stream);
    if (e.records_on && p->n_frames > c->max_frames) return FLACGPU_ERR_INVALID_INPUT;
    uint8_t *desc = p->d_desc.get() ? p->d_desc.get() : e.d_desc.get();
    // MD5 of every stream on a second stream, overlapping the encode kernels (joined back into
    // st unless the caller owns the MD5 stream)
    const bool join = md5_stream == nullptr;
    hipStream_t ms = join ? e.aux.get() : pick_stream(c, md5_stream);
    const bool md5 = (d_md5 || d_md5_state) && p->n_streams;
    if (md5) {
        Event pooled = join ? Event() : get_event(c);
        const hipEvent_t fork = join ? e.fork.get() : pooled.get();
        if (!fork) return FLACGPU_ERR_DEVICE;
        HIPCHK(hipEventRecord(fork, st));
        HIPCHK(hipStreamWaitEvent(ms, fork, 0));
        if (!join) c->event_pool.push_back(std::move(pooled));  // recycled: the wait is already enqueued
        {
            Timed t(c, FLACGPU_K_MD5, ms);
            HIPCHK(launch_md5_streams((const uint8_t *)d_pcm, p->d_md5_offs.get(), p->d_md5_lens.get(), p->d_md5_fin.get(),
                                      p->n_streams, (Md5State *)d_md5_state, d_md5, ms, c->md5_kernel, c->k.md5_prio));
        }
        if (join) HIPCHK(hipEventRecord(e.join.get(), ms));
    }
    // the MD5 workgroups were queued first: the encode kernels' persistent grids leave their slots
    // auto: only for long chains (>= 4096 blocks per stream per call, e.g. c4's 4 x 96-KiB frames).  A
    // persistent grid cannot grow back, so the reserved slots idle once the MD5 is done; a shorter
    // chain started late (after the analysis) still ends before the pack
    const bool reserve = c->k.md5_reserve > 0 || (c->k.md5_reserve < 0 && p->md5_max_len >= (256u << 10));
    e.grid_reserve = (md5 && reserve) ? md5_workgroups(p->n_streams, c->md5_kernel) : 0u;
    int rc = encode_core(c, (const uint8_t *)d_pcm, p->d_jobs.get(), p->n_full, p->n_tail, desc, d_frame_bytes, d_out,
                         out_cap, d_frame_offsets, d_total, st, p->full_slots.data());
    e.grid_reserve = 0;
    if (rc) return rc;
    if (join && md5) HIPCHK(hipStreamWaitEvent(st, e.join.get(), 0));
    return FLACGPU_OK;
}

int flacgpu_encode_plan_device_md5_async(flacgpu_ctx *c, const flacgpu_plan *p, const void *d_pcm, uint8_t *d_out,
                                         uint64_t out_cap, uint32_t *d_frame_bytes, uint64_t *d_frame_offsets,
                                         uint64_t *d_total, uint8_t *d_md5, void *hip_stream, void *md5_stream) {
    return flacgpu_encode_plan_device_ex(c, p, d_pcm, d_out, out_cap, d_frame_bytes, d_frame_offsets, d_total, nullptr,
                                         d_md5, hip_stream, md5_stream);
}

int flacgpu_encode_plan_device(flacgpu_ctx *c, const flacgpu_plan *p, const void *d_pcm, uint8_t *d_out,
                               uint64_t out_cap, uint32_t *d_frame_bytes, uint64_t *d_frame_offsets, uint64_t *d_total,
                               uint8_t *d_md5, void *hip_stream) {
    return flacgpu_encode_plan_device_ex(c, p, d_pcm, d_out, out_cap, d_frame_bytes, d_frame_offsets, d_total, nullptr,
                                         d_md5, hip_stream, nullptr);
}

int flacgpu_streaminfo_replay_device(flacgpu_ctx *c, const uint32_t *d_frame_bytes, uint64_t n_frames,
                                     uint32_t *d_minmax, void *hip_stream) {
    if (!c || !d_minmax || (n_frames && !d_frame_bytes)) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, hip_stream);
    HIPCHK(launch_streaminfo_replay(d_frame_bytes, n_frames, d_minmax, st));
    return FLACGPU_OK;
}

// ---- tensor elements to the encoder's PCM (fg_quantize.hpp) -------------------
namespace {

// a stream's PCM bytes rounded up to whole words, or false where T * C * B passes 2^62
bool quant_span(uint64_t samples, uint32_t C, uint32_t B, uint64_t &span) {
    if (samples > (1ull << 62) / ((uint64_t)C * B)) return false;
    span = quantize::pcm_words(samples * C, B) * 4u;
    return true;
}

}  // namespace

int flacgpu_pcm_from_elements_device(flacgpu_ctx *c, uint32_t n_streams, const void *const *d_src, const uint64_t *samples,
                                     const uint64_t *plane_stride, uint32_t sample_format, uint32_t flags, uint8_t *d_pcm,
                                     const uint64_t *pcm_offsets, uint64_t pcm_cap, uint64_t *d_clipped, void *hip_stream) {
    if (!c || !c->enc) return FLACGPU_ERR_INVALID_INPUT;  // a decode-only context has no PCM to encode
    if (n_streams > quantize::kMaxStreams || sample_format >= quantize::SAMPLE_FORMATS || (flags & ~(uint32_t)FLACGPU_DELIVER_PLANAR))
        return FLACGPU_ERR_INVALID_INPUT;
    if (!n_streams) return FLACGPU_OK;
    if (!d_src || !samples || !d_pcm || !pcm_offsets || !d_clipped) return FLACGPU_ERR_INVALID_INPUT;
    EncState &e = *c->enc;
    const uint32_t C = e.g.C, B = e.g.B;
    const bool planar = (flags & FLACGPU_DELIVER_PLANAR) != 0;
    std::vector<quantize::Stream> tab;
    try {
        tab.resize(n_streams);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    uint64_t max_units = 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        uint64_t span;
        const uint64_t stride = plane_stride ? plane_stride[s] : samples[s];
        if (!d_src[s] || (pcm_offsets[s] & 3u) || !quant_span(samples[s], C, B, span)) return FLACGPU_ERR_INVALID_INPUT;
        if (planar && stride < samples[s]) return FLACGPU_ERR_INVALID_INPUT;
        if (pcm_offsets[s] > pcm_cap || span > pcm_cap - pcm_offsets[s]) return FLACGPU_ERR_INVALID_INPUT;
        if (s + 1u < n_streams && (pcm_offsets[s + 1u] < pcm_offsets[s] || span > pcm_offsets[s + 1u] - pcm_offsets[s]))
            return FLACGPU_ERR_INVALID_INPUT;  // a stream runs into the next one
        tab[s] = {d_src[s], samples[s], stride, pcm_offsets[s]};
        max_units = std::max(max_units, quantize::units(samples[s] * C));
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, hip_stream);
    const uint64_t bytes = (uint64_t)n_streams * sizeof(quantize::Stream);
    HIPCHK(e.d_quant.grow(bytes, &st));  // an earlier call on this stream may still read the old table
    HIPCHK(hipMemcpyAsync(e.d_quant.get(), tab.data(), bytes, hipMemcpyHostToDevice, st));
    HIPCHK(launch_elements_pcm((const quantize::Stream *)e.d_quant.get(), n_streams, max_units, d_pcm, d_clipped, C, B,
                               sample_format, planar, st));
    return FLACGPU_OK;
}

int flacgpu_pcm_from_elements_host(const void *src, uint64_t samples, uint64_t plane_stride, uint32_t channels, uint32_t bits,
                                   uint32_t sample_format, uint32_t flags, uint8_t *pcm_out, size_t cap, uint64_t *clipped) {
    if (!src || !pcm_out || !clipped || ((uintptr_t)pcm_out & 3u)) return FLACGPU_ERR_INVALID_INPUT;
    if (channels < 1u || channels > 8u || (bits != 8u && bits != 16u && bits != 24u && bits != 32u)) return FLACGPU_ERR_INVALID_INPUT;
    if (sample_format >= quantize::SAMPLE_FORMATS || (flags & ~(uint32_t)FLACGPU_DELIVER_PLANAR)) return FLACGPU_ERR_INVALID_INPUT;
    const bool planar = (flags & FLACGPU_DELIVER_PLANAR) != 0;
    const uint32_t B = bits / 8u;
    uint64_t span;
    if ((planar && plane_stride < samples) || !quant_span(samples, channels, B, span)) return FLACGPU_ERR_INVALID_INPUT;
    *clipped = 0;
    if (span > cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
    const quantize::Stream st{src, samples, plane_stride, 0};
    const uint64_t n = samples * channels, nu = quantize::units(n);
    uint64_t count = 0;
    for (uint64_t u = 0; u < nu; u++)
        count += quantize::convert_unit<uint64_t>(st, (uint32_t *)pcm_out, u, n, channels, B, sample_format, planar);
    *clipped = count;
    return FLACGPU_OK;
}

int flacgpu_sync_check(flacgpu_ctx *c, void *hip_stream) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(pick_stream(c, hip_stream)));
    if (!c->enc) return FLACGPU_OK;  // the error word is the encode kernels': decode statuses are per frame
    return check_device_error(c);
}

// ---- instrumentation ---------------------------------------------------------
int flacgpu_set_timing(flacgpu_ctx *c, int enable) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    c->timing = enable != 0;
    return FLACGPU_OK;
}

int flacgpu_kernel_time(flacgpu_ctx *c, int kernel, uint64_t *launches, double *total_ms) {
    if (!c || kernel < 0 || kernel >= FLACGPU_K_COUNT) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    resolve_timing(c);
    if (launches) *launches = c->launches[kernel];
    if (total_ms) *total_ms = c->ms[kernel];
    return FLACGPU_OK;
}

int flacgpu_reset_timing(flacgpu_ctx *c) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    resolve_timing(c);
    for (int k = 0; k < FLACGPU_K_COUNT; k++) {
        c->launches[k] = 0;
        c->ms[k] = 0;
    }
    return FLACGPU_OK;
}

int flacgpu_set_overlap(flacgpu_ctx *c, uint32_t ranges, uint32_t ana_per_cu, uint32_t pack_per_cu,
                        uint32_t min_frames) {
    if (!c || ranges > kOvlMaxChunks || min_frames == 0) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);
    EncState &e = *c->enc;
    // the overlapped schedule measured slower: diagnostic builds only
    if (!FG_DIAG && ranges > 1) return FLACGPU_ERR_INVALID_CONFIG;
    e.ovl_chunks = ranges;
    e.ovl_ana = ana_per_cu;
    e.ovl_pack = pack_per_cu;
    e.ovl_min_frames = min_frames;
    return FLACGPU_OK;
}

int flacgpu_set_records(flacgpu_ctx *c, int enable) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);
    EncState &e = *c->enc;
    HIPCHK(hipSetDevice(c->device));
    if (enable) HIPCHK(zeroed(e.d_records, c->max_frames));  // the first call allocates
    e.records_on = enable != 0;
    return FLACGPU_OK;
}

int flacgpu_get_records(flacgpu_ctx *c, flacgpu_frame_record *out, uint64_t max_frames, uint64_t *n_frames) {
    if (!c || !n_frames) return FLACGPU_ERR_INVALID_INPUT;
    const std::vector<FrameRec> none, &recs = c->enc ? c->enc->h_records : none;  // a decode-only context has none
    const uint64_t n = std::min<uint64_t>(max_frames, recs.size());
    if (out && n) std::memcpy(out, recs.data(), n * sizeof(FrameRec));
    *n_frames = recs.size();
    return FLACGPU_OK;
}

// Diagnostic build only (-DFG_STAMPS): per-phase shader-clock sums of the encode kernel.
int flacgpu_debug_stamps(flacgpu_ctx *c, uint64_t *out32, int reset) {
    if (!c || !out32) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);
    EncState &e = *c->enc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(out32, e.d_stamps.get(), 32 * 8, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(e.d_stamps.get(), 0, 32 * 8));
    return FLACGPU_OK;
}

}  // extern "C"
