// fg_dec_host.cpp -- the device-driving side of the decoder's C ABI: the frame decoder / verifier
// (fg_dec.hpp, fg_dec.hip) and the device frame index (fg_index.hpp, fg_index.hip) over device
// memory, the host-buffer decode, and the device side of the whole-file decode; and their
// many-streams forms: the index of n streams in one call, decode chunks that span streams
// (fg_streams.hpp, fg_dec_streams.hip), and the device side of flacgpu_decode_files; and the
// sample-window decode (fg_window.hpp, fg_window.hip): the positions of indexed streams, windows
// over resident tables -- as PCM bytes or as tensor elements (fg_deliver.hpp) -- and the device
// side of flacgpu_decode_files_windows; and the same windows stated and delivered at another
// sample rate (fg_resample.hpp, fg_resample.hip), and as short-time power spectra and filter-bank
// rows over that delivery (fg_features.hpp, fg_features.hip), and convolved with a per-window FIR
// filter (fg_fir.hpp, fg_fir.hip); and the same windows measured, not
// delivered: peak, sum and energy a block (fg_levels.hpp, fg_levels.hip).  The host-only side (metadata, the host index,
// flacgpu_decode_file / _files) is fg_dec_api.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/flacgpu.h"
#include "fg_ctx.hpp"
#include "fg_dec.hpp"
#include "fg_deliver.hpp"
#include "fg_features.hpp"
#include "fg_fir.hpp"
#include "fg_index.hpp"
#include "fg_internal.hpp"
#include "fg_levels.hpp"
#include "fg_resample.hpp"
#include "fg_streams.hpp"
#include "fg_window.hpp"

using namespace fg;

static_assert(sizeof(window::WindowResult) == sizeof(flacgpu_window_result), "window result layout");
static_assert(FLACGPU_WINDOW_BAD_INDEX == (int)window::WIN_BAD_INDEX && FLACGPU_WINDOW_BAD_FRAME == (int)window::WIN_BAD_FRAME &&
                  FLACGPU_WINDOW_TOO_SMALL == (int)window::WIN_TOO_SMALL,
              "window status codes");
static_assert(FLACGPU_SAMPLE_I32 == (int)deliver::SAMPLE_I32 && FLACGPU_SAMPLE_F32 == (int)deliver::SAMPLE_F32 &&
                  FLACGPU_SAMPLE_F16 == (int)deliver::SAMPLE_F16 && FLACGPU_SAMPLE_BF16 == (int)deliver::SAMPLE_BF16 &&
                  FLACGPU_DELIVER_PLANAR == (int)deliver::DELIVER_PLANAR && FLACGPU_DELIVER_PAD == (int)deliver::DELIVER_PAD,
              "sample formats and delivery flags");
static_assert(sizeof(dec::Result) == sizeof(flacgpu_decode_result), "decode result layout");
static_assert(sizeof(idx::IndexResult) == sizeof(flacgpu_index_result), "index result layout");
static_assert(sizeof(streams::StreamResult) == sizeof(flacgpu_stream_result), "stream result layout");
static_assert(FLACGPU_INDEX_INVALID == (int)idx::IDX_INVALID && FLACGPU_INDEX_TOO_SMALL == (int)idx::IDX_TOO_SMALL,
              "index status codes");
static_assert(sizeof(fir::Filter) == sizeof(flacgpu_fir), "filter layout");

namespace {

// All or nothing: c->dec is set only once its allocation is there, so a call that fails here
// leaves the context as it was and the next one tries again.
int dec_scratch(flacgpu_ctx *c) {
    if (c->dec) return FLACGPU_OK;
    std::unique_ptr<DecScratch> d(new (std::nothrow) DecScratch());
    if (!d) return FLACGPU_ERR_OUT_OF_MEMORY;
    HIPCHK(fit(d->buf, [&](uint8_t *base) {  // 8-byte members first
        Carve v{base};
        v.take(c->max_frames, d->samp_off, d->exp_off, d->exp_number, d->d_foff, d->d_results);
        v.take(1, d->total);
        v.take((uint64_t)c->max_frames * c->fmt.channels, d->subs);
        v.take(c->max_frames, d->blocks, d->body, d->exp_n, d->d_fbytes);
        v.take(16, d->ctl);
        return v.take(1, d->d_bad);
    }));
    c->dec = std::move(d);
    return FLACGPU_OK;
}

IdxScratch *idx_scratch(flacgpu_ctx *c) {
    if (!c->idx) c->idx.reset(new (std::nothrow) IdxScratch());
    return c->idx.get();
}

// a chunk that holds frames of several streams: its segments and the per-stream arrays (device)
struct ChunkStreams {
    const streams::Segment *segs;
    uint32_t n_segs;
    const uint64_t *pcm_base, *pcm_cap;
    uint64_t *carried;
    streams::StreamResult *res;
};

// parse, (scan / segment offsets,) reconstruct(, fold) of n frames, queued on st.  The PCM offsets:
// d_pcm_off per frame; or NULL and no `cs`: consecutive blocks of one stream; or `cs`: frames of
// several streams, offsets from the segments (the verify arrays' exp_off holds them).
int dec_core(flacgpu_ctx *c, const uint8_t *d_frames, const uint64_t *d_foff, const uint32_t *d_fbytes, uint32_t n,
             const uint64_t *d_pcm_off, uint8_t *d_out, uint64_t cap, const uint8_t *d_expect, bool verify,
             flacgpu_decode_result *d_results, uint32_t *d_bad, hipStream_t st, const ChunkStreams *cs = nullptr) {
    DecScratch *d = c->dec.get();
    if (cs) d_pcm_off = d->exp_off;
    dec::Args a{};
    a.frames = d_frames;
    a.frame_off = d_foff;
    a.frame_bytes = d_fbytes;
    a.n_frames = n;
    a.channels = c->fmt.channels;
    a.bits = c->fmt.bits;
    a.bps = c->fmt.bytes_per_sample;
    a.rate = c->fmt.sample_rate;
    a.block = c->fmt.max_block;
    a.subs = d->subs;
    a.blocks = d->blocks;
    a.body = d->body;
    a.pcm_off = d_pcm_off;
    a.samp_off = d->samp_off;
    a.out = d_out;
    a.cap = cap;
    a.expect = d_expect;
    a.exp_number = verify ? d->exp_number : nullptr;
    a.exp_n = verify ? d->exp_n : nullptr;
    a.results = (dec::Result *)d_results;
    a.bad = d_bad ? d_bad : d->d_bad;
    a.ticket = d->ctl;
    {
        Timed t(c, FLACGPU_K_DEC_PARSE, st);
        HIPCHK(launch_dec_parse(a, st));
    }
    if (cs) {
        Timed t(c, FLACGPU_K_SCAN, st);
        HIPCHK(launch_seg_offsets(cs->segs, cs->n_segs, d->blocks, cs->pcm_base, cs->pcm_cap, cs->carried, c->fmt.channels * a.bps,
                                  d->exp_off, st));
    } else if (!d_pcm_off) {
        // consecutive blocks of one stream: sample offsets from the scan of the parsed block sizes
        HIPCHK(c->d_scan_part.grow((n + 4095u) / 4096u, &st));
        Timed t(c, FLACGPU_K_SCAN, st);
        HIPCHK(launch_scan(d->blocks, d->samp_off, d->total, n, c->d_scan_part.get(), st));
    }
    {
        Timed t(c, FLACGPU_K_DEC_RECON, st);
        HIPCHK(launch_dec_recon(a, st));
    }
    if (cs) HIPCHK(launch_seg_fold(cs->segs, cs->n_segs, a.results, cs->res, st));
    return FLACGPU_OK;
}

// the eight stages over [d_data, d_data + len), len > 0, queued on st
int index_core(flacgpu_ctx *c, const uint8_t *d_data, uint64_t len, uint32_t stream_bits, uint32_t stream_rate,
               uint64_t *d_off, uint32_t *d_bytes, uint64_t cap, idx::IndexResult *d_res, hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    idx::IdxArgs g{};
    g.data = d_data;
    idx::stream_geometry(g, (uint64_t)(uintptr_t)d_data, len, cap);
    g.bits = stream_bits;
    g.rate = stream_rate;
    g.offs = d_off;
    g.bytes = d_bytes;
    g.res = d_res;
    auto carve = [&](uint8_t *base) {  // 8-byte members first
        Carve v{base};
        v.take(g.n_chunks, g.cmask, g.smask);
        v.take(g.n_groups, g.grp, g.gcnt);
        v.take(4, g.ctl);
        v.take(g.spos_cap, g.spos);
        return v.take(g.n_chunks, g.terms);
    };
    HIPCHK(fit(x->buf, carve, &st));  // an earlier index on this stream may still use the old one
    Timed t(c, FLACGPU_K_INDEX, st);
    HIPCHK(launch_index(g, st));
    return FLACGPU_OK;
}

// The eight stages, once, over n streams of one device buffer (0 < n <= kIdxMaxStreams, every
// length < 2^32): stream s owns entries [table_first[s], + table_caps[s]) of the two tables and
// d_res[s].  One table of n IdxArgs goes to the device; the host waits only where the scratch grows.
int index_streams_core(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n, const uint64_t *offs, const uint64_t *lens,
                       const uint32_t *bits, const uint32_t *rates, const uint64_t *table_first, const uint64_t *table_caps,
                       uint64_t *d_off, uint32_t *d_bytes, idx::IndexResult *d_res, hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    std::vector<idx::IdxArgs> tab;
    try {
        tab.assign(n, idx::IdxArgs{});
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    idx::IdxTotals tot;
    for (uint32_t s = 0; s < n; s++) {
        idx::IdxArgs &g = tab[s];
        g.data = d_data + offs[s];
        idx::stream_geometry(g, (uint64_t)(uintptr_t)g.data, lens[s], table_caps[s]);
        g.bits = bits ? bits[s] : 16u;
        g.rate = rates ? rates[s] : 0u;
        g.offs = d_off + table_first[s];
        g.bytes = d_bytes + table_first[s];
        g.res = d_res + s;
        g.base_off = offs[s];
        idx::totals_add(tot, g);
    }
    idx::IdxPool pool{};
    idx::IdxArgs *d_tab = nullptr;
    auto carve = [&](uint8_t *base) {  // 8-byte members first
        Carve v{base};
        v.take(tot.chunks, pool.cmask, pool.smask);
        v.take(n, d_tab);
        v.take(tot.groups, pool.grp, pool.gcnt);
        v.take(4u * (uint64_t)n, pool.ctl);
        v.take(tot.spos, pool.spos);
        return v.take(tot.chunks, pool.terms);
    };
    HIPCHK(fit(x->buf, carve, &st));  // an earlier index on this stream may still use the old one
    idx::IdxTotals at;
    for (uint32_t s = 0; s < n; s++) idx::carve_stream(tab[s], pool, at);
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), (uint64_t)n * sizeof(idx::IdxArgs), hipMemcpyHostToDevice, st));
    Timed t(c, FLACGPU_K_INDEX, st);
    HIPCHK(launch_index_streams(d_tab, n, tot.max_groups, tot.max_spos, st));
    return FLACGPU_OK;
}

// the table entries a stream of len bytes can need: a frame is at least 9 bytes
inline uint64_t table_cap_for(uint64_t len) { return len / 8u + 1u; }

bool streams_args_ok(uint32_t n, const uint64_t *lens) {
    if (n > idx::kIdxMaxStreams) return false;
    for (uint32_t s = 0; s < n; s++)
        if (lens[s] > 0xFFFFFFFFull) return false;
    return true;
}

// The frame tables of a many-streams decode, in the context's index scratch: stream s owns
// table_cap_for(lens[s]) entries from first[s].
struct StreamTables {
    std::vector<uint64_t> first, caps;
    uint64_t *f_off = nullptr;
    uint32_t *f_bytes = nullptr;
    idx::IndexResult *d_ires = nullptr;
};

// Index all streams into the context's table, wait for hip_stream once, and leave the index
// results in `ires`.
int streams_index(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n, const uint64_t *offs, const uint64_t *lens,
                  const uint32_t *bits, const uint32_t *rates, StreamTables &tb, std::vector<idx::IndexResult> &ires,
                  hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    uint64_t total = 0;
    try {
        tb.first.resize(n);
        tb.caps.resize(n);
        ires.resize(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t s = 0; s < n; s++) {
        tb.first[s] = total;
        tb.caps[s] = table_cap_for(lens[s]);
        total += tb.caps[s];
    }
    auto table = [&](uint8_t *base) {
        Carve v{base};
        v.take(total, tb.f_off);
        v.take(n, tb.d_ires);
        return v.take(total, tb.f_bytes);
    };
    HIPCHK(fit(x->table, table, &st));
    const int rc = index_streams_core(c, d_data, n, offs, lens, bits, rates, tb.first.data(), tb.caps.data(), tb.f_off,
                                      tb.f_bytes, tb.d_ires, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ires.data(), tb.d_ires, (uint64_t)n * sizeof(idx::IndexResult), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FLACGPU_OK;
}

// What a many-streams decode and a window decode share once every stream s < n -- a stream, or the
// covering frames of a window -- has its frame count.  prepare() cuts frames[] into segments and
// chunks of max_frames frames, carves the packed frame table, the meta rows, `carried`, whatever
// `extra` takes and the segments out of buf (grown, after a wait for st where it must), and uploads
// `host` -- rows of n values: row 0 the PCM bases, 1 the PCM caps, 2 the first table entries, the
// rest the caller's -- and the segments.  The caller's init kernel goes between the two steps.
// run() packs the frame tables and puts every chunk through parse, segment offsets, reconstruct
// and fold.  Both only queue.
struct ChunkRun {
    std::vector<streams::Segment> segs;
    std::vector<uint32_t> chunk_seg;
    uint32_t n = 0;
    uint64_t *p_off = nullptr, *meta = nullptr, *carried = nullptr;
    uint32_t *p_bytes = nullptr;
    streams::Segment *d_segs = nullptr;

    uint64_t *row(uint32_t r) const { return meta + (uint64_t)r * n; }

    template <class Extra>
    int prepare(flacgpu_ctx *c, const std::vector<uint64_t> &frames, const std::vector<uint64_t> &host,
                DevBuf<uint8_t> &buf, Extra extra, hipStream_t st) {
        n = (uint32_t)frames.size();
        try {
            streams::cut_segments(frames, c->max_frames, segs, chunk_seg);
        } catch (...) {
            return FLACGPU_ERR_OUT_OF_MEMORY;
        }
        const uint64_t n_packed = (uint64_t)(chunk_seg.empty() ? 0u : chunk_seg.size() - 1u) * c->max_frames;
        auto carve = [&](uint8_t *base) {
            Carve v{base};
            v.take(n_packed, p_off);
            v.take(host.size(), meta);  // one upload
            v.take(n, carried);
            extra(v);
            v.take(segs.size(), d_segs);
            return v.take(n_packed, p_bytes);
        };
        HIPCHK(fit(buf, carve, &st));
        HIPCHK(hipMemcpyAsync(meta, host.data(), host.size() * 8u, hipMemcpyHostToDevice, st));
        if (!segs.empty())
            HIPCHK(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(streams::Segment), hipMemcpyHostToDevice, st));
        return FLACGPU_OK;
    }

    // the frames of d_data by the tables f_off / f_bytes into d_out, of which `whole` bytes are the
    // capacity k_dec_recon checks: the end of the last region
    int run(flacgpu_ctx *c, const uint8_t *d_data, const uint64_t *f_off, const uint32_t *f_bytes, uint8_t *d_out,
            uint64_t whole, streams::StreamResult *res, hipStream_t st) const {
        HIPCHK(launch_streams_gather(d_segs, (uint32_t)segs.size(), row(2), f_off, f_bytes, p_off, p_bytes, st));
        for (uint32_t k = 0; k + 1u < chunk_seg.size(); k++) {
            const uint32_t s0 = chunk_seg[k], s1 = chunk_seg[k + 1u];
            const uint32_t nf = segs[s1 - 1u].first + segs[s1 - 1u].count;
            const ChunkStreams cs{d_segs + s0, s1 - s0, row(0), row(1), carried, res};
            const int rc = dec_core(c, d_data, p_off + (uint64_t)k * c->max_frames, p_bytes + (uint64_t)k * c->max_frames, nf,
                                    nullptr, d_out, whole, nullptr, false, (flacgpu_decode_result *)c->dec->d_results, nullptr,
                                    st, &cs);
            if (rc) return rc;
        }
        return FLACGPU_OK;
    }
};

// Everything after the index of a many-streams decode, only queued: the streams' results set up,
// the frame tables of the OK streams packed and every chunk decoded (ChunkRun), then (d_md5) one
// batched MD5 over the decoded regions.
int streams_decode(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n, const StreamTables &tb,
                   const std::vector<idx::IndexResult> &ires, uint8_t *d_pcm_out, const uint64_t *pcm_offsets,
                   const uint64_t *pcm_caps, streams::StreamResult *d_results, uint8_t *d_md5, hipStream_t st) {
    std::vector<uint64_t> frames, host;
    uint64_t whole = 0;
    try {
        frames.assign(n, 0);
        host.resize(3u * (uint64_t)n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t s = 0; s < n; s++) {
        if (ires[s].status == idx::IDX_OK && ires[s].n_frames <= tb.caps[s]) frames[s] = ires[s].n_frames;
        whole = std::max(whole, pcm_offsets[s] + pcm_caps[s]);
        host[s] = pcm_offsets[s];
        host[n + s] = pcm_caps[s];
        host[2u * (uint64_t)n + s] = tb.first[s];
    }
    ChunkRun run;
    uint64_t *md5_lens = nullptr;
    int rc = run.prepare(c, frames, host, c->idx->packed, [&](Carve &v) { v.take(n, md5_lens); }, st);
    if (rc) return rc;
    HIPCHK(launch_streams_init(tb.d_ires, d_results, run.carried, n, st));
    rc = run.run(c, d_data, tb.f_off, tb.f_bytes, d_pcm_out, whole, d_results, st);
    if (rc) return rc;
    if (d_md5) {
        HIPCHK(launch_streams_md5_lens(d_results, c->fmt.channels * c->fmt.bytes_per_sample, md5_lens, n, st));
        {
            Timed t(c, FLACGPU_K_MD5, st);
            HIPCHK(launch_md5_streams(d_pcm_out, run.row(0), md5_lens, nullptr, n, nullptr, d_md5, st, c->md5_kernel,
                                      c->k.md5_prio));
        }
        HIPCHK(launch_streams_md5_mask(d_results, d_md5, n, st));
    }
    return FLACGPU_OK;
}

// The sample positions of n indexed streams (0 < n <= kIdxMaxStreams), only queued: one table of
// n PosStream goes to the device; the grids are sized from the caps, the frame counts are read
// from d_res on the device.
int positions_core(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n, const uint64_t *table_first, const uint64_t *table_caps,
                   const uint64_t *d_off, const uint32_t *d_bytes, const idx::IndexResult *d_res, const uint32_t *bits,
                   const uint32_t *rates, uint64_t *d_pos, uint64_t *d_totals, hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    std::vector<window::PosStream> tab;
    try {
        tab.resize(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    uint64_t max_cap = 0;
    for (uint32_t s = 0; s < n; s++) {
        tab[s] = {table_first[s], table_caps[s], bits ? bits[s] : 16u, rates ? rates[s] : 0u};
        max_cap = std::max(max_cap, table_caps[s]);
    }
    HIPCHK(x->pos.grow((uint64_t)n * sizeof(window::PosStream), &st));  // an earlier call may still use the old one
    HIPCHK(hipMemcpyAsync(x->pos.get(), tab.data(), (uint64_t)n * sizeof(window::PosStream), hipMemcpyHostToDevice, st));
    Timed t(c, FLACGPU_K_SCAN, st);
    HIPCHK(launch_positions(d_data, (const window::PosStream *)x->pos.get(), n, max_cap, d_off, d_bytes, d_res, d_pos, d_totals, st));
    return FLACGPU_OK;
}

// A window call that resamples: its ratio, the ratio's table on the device and the streams' totals.
struct Resampling {
    resample::Ratio rt;
    const float *d_coeffs;
    const uint64_t *d_totals;
};

// The device table of a ratio: built on the host by flacgpu_resample_filter and uploaded by the
// first call of the context that needs it, which waits for st once more than the others; kept for
// the context's life.
int resample_table(flacgpu_ctx *c, const resample::Ratio &rt, uint32_t src_rate, uint32_t dst_rate, const float **d_coeffs,
                   hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    for (const ResampleTable &t : x->tables)
        if (t.L == rt.L && t.M == rt.M) {
            *d_coeffs = t.coeffs.get();
            return FLACGPU_OK;
        }
    std::vector<float> h;
    size_t n = 0;
    try {
        h.resize((size_t)rt.L * rt.T);
        x->tables.reserve(x->tables.size() + 1u);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    const int rc = flacgpu_resample_filter(src_rate, dst_rate, nullptr, nullptr, nullptr, h.data(), h.size(), &n);
    if (rc) return rc;
    DevBuf<float> d;
    HIPCHK(d.grow(n));
    HIPCHK(hipMemcpyAsync(d.get(), h.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // h goes out of scope
    *d_coeffs = d.get();
    x->tables.push_back({rt.L, rt.M, std::move(d)});
    return FLACGPU_OK;
}

// The device copy of a weight matrix W[K][C], found again by its content; a new one is uploaded by
// the first call that needs it, which waits for st once more than the others.  The context keeps
// the last kMaxMixWeights matrices: before the oldest is dropped st is waited for, since work queued
// on it may still read that matrix.  dec_scratch(c) has run.
int mix_weights(flacgpu_ctx *c, uint32_t K, uint32_t C, const float *W, const float **d_weights, hipStream_t st) {
    DecScratch *d = c->dec.get();
    const size_t n = (size_t)K * C;
    for (const MixWeights &m : d->mix_weights)
        if (m.rows == K && m.cols == C && std::memcmp(m.host.data(), W, n * sizeof(float)) == 0) {
            *d_weights = m.dev.get();
            return FLACGPU_OK;
        }
    MixWeights m;
    try {
        m.host.assign(W, W + n);
        d->mix_weights.reserve(d->mix_weights.size() + 1u);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    m.rows = K;
    m.cols = C;
    HIPCHK(m.dev.grow(n));
    HIPCHK(hipMemcpyAsync(m.dev.get(), m.host.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    if (d->mix_weights.size() >= kMaxMixWeights) d->mix_weights.erase(d->mix_weights.begin());  // st has just been waited for
    *d_weights = m.dev.get();
    d->mix_weights.push_back(std::move(m));
    return FLACGPU_OK;
}

// A window call that measures levels (fg_levels.hpp) in place of delivering: the hop and the three
// arrays of records.
struct Levels {
    uint32_t hop;
    uint32_t *d_peak;
    int64_t *d_sum;
    double *d_energy;
};

// The windows of a call between its two halves: as uploaded, and their cover records on both sides.
struct WindowsCall {
    uint32_t n = 0;
    window::WindowArg *d_args = nullptr;
    window::Cover *d_recs = nullptr;
    std::vector<window::Cover> recs;
};

// The first half of a window decode: the windows go to the device, k_window_cover finds their
// covering frames, and the host waits for st ONCE to read the records.  caps[w]: the bytes of
// window w's destination, or its elements where dv converts; TOO_SMALL is deliver::too_small's.
// With `rs` the windows are stated in output samples of its ratio and k_resample_cover covers the
// source samples their filter needs.  With `lv` caps[w] counts records of a block and channel and
// TOO_SMALL is levels::too_small's.
int windows_cover(flacgpu_ctx *c, const uint64_t *table_first, const idx::IndexResult *d_ires, const uint64_t *d_pos,
                  const uint64_t *d_totals, uint32_t n, const uint32_t *window_stream, const uint64_t *window_start,
                  const uint64_t *window_count, const uint64_t *caps, const deliver::Delivery &dv, WindowsCall &wc,
                  hipStream_t st, const Resampling *rs = nullptr, const Levels *lv = nullptr) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    std::vector<window::WindowArg> args;
    try {
        args.resize(n);
        wc.recs.resize(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t w = 0; w < n; w++)
        args[w] = {window_start[w], window_count[w], caps[w], table_first[window_stream[w]], window_stream[w], 0u};
    auto carve = [&](uint8_t *base) {
        Carve v{base};
        v.take(n, wc.d_args);
        return v.take(n, wc.d_recs);
    };
    HIPCHK(fit(x->win_in, carve, &st));  // an earlier call may still use the old one
    wc.n = n;
    HIPCHK(hipMemcpyAsync(wc.d_args, args.data(), (uint64_t)n * sizeof(window::WindowArg), hipMemcpyHostToDevice, st));
    {
        Timed t(c, FLACGPU_K_SCAN, st);
        const uint32_t unit = lv ? dv.channels : dv.format == deliver::SAMPLE_BYTES ? dv.channels * dv.sample_bytes : dv.out_channels;
        if (rs) HIPCHK(launch_resample_cover(wc.d_args, d_ires, d_pos, d_totals, rs->rt, unit, dv.flags, wc.d_recs, n, st));
        else HIPCHK(launch_window_cover(wc.d_args, d_ires, d_pos, d_totals, unit, dv.flags, lv ? lv->hop : 0u, wc.d_recs, n, st));
    }
    HIPCHK(hipMemcpyAsync(wc.recs.data(), wc.d_recs, (uint64_t)n * sizeof(window::Cover), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FLACGPU_OK;
}

// The second half, only queued.  Every window plays the role a stream plays in streams_decode: its
// covering frames are its frames, cut with all the others' into chunks of max_frames (ChunkRun);
// its PCM region is span * per bytes of the context's window scratch (bases 16-byte aligned); its
// result is a scratch StreamResult.  After the last chunk k_window_copy moves each clean window's
// bytes to d_pcm_out + out_offsets[w] -- or, where dv converts, k_window_elements (its mix
// instantiation where dv mixes: dv.out_channels channels a sample) writes its elements from element
// out_offsets[w] of d_pcm_out on -- and k_window_results writes d_results.  With `rs` a record's
// n_samples counts output samples, its cover is that of the filter's source range, and
// k_window_resample stands in place of k_window_elements.  With `lv` nothing is delivered:
// k_window_levels stands in place of k_window_copy and writes the records of every clean window's
// blocks from record out_offsets[w] of lv's arrays on; where a block is longer than a tile, window w
// has levels::partial_records(n, ...) Acc of the chunk loop's scratch for its parts' exact partial
// results, which k_levels_fold sums.
int windows_decode(flacgpu_ctx *c, const uint8_t *d_data, const uint64_t *table_first, const uint64_t *d_foff,
                   const uint32_t *d_fbytes, const WindowsCall &wc, const uint32_t *window_stream,
                   const uint64_t *window_count, const deliver::Delivery &dv, uint8_t *d_pcm_out, const uint64_t *out_offsets,
                   window::WindowResult *d_results, hipStream_t st, const Resampling *rs = nullptr, const Levels *lv = nullptr) {
    IdxScratch *x = c->idx.get();
    const uint32_t n = wc.n;
    const uint64_t per = (uint64_t)c->fmt.channels * c->fmt.bytes_per_sample;
    std::vector<uint64_t> frames, host;  // host: scratch base, scratch cap, table first, destination(, lv: first partial)
    const bool convert = dv.format != deliver::SAMPLE_BYTES;
    const levels::Plan pl = levels::plan(lv ? lv->hop : 1u, (uint32_t)per);
    uint64_t n_parts = 0, max_measured = 0;  // lv: the partial records of all windows; the most samples a window measures
    uint64_t whole = 0, max_bytes = 0;  // whole: the end of the last region
    uint64_t max_written = 0;           // convert: the most samples a window writes, its padding included
    try {
        frames.assign(n, 0);
        host.assign((lv ? 5u : 4u) * (uint64_t)n, 0);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    for (uint32_t w = 0; w < n; w++) {
        const window::Cover &r = wc.recs[w];
        const bool decode = r.status == window::WIN_OK && r.n_frames > 0;
        host[w] = whole;
        host[2u * (uint64_t)n + w] = table_first[window_stream[w]] + r.first_frame;
        host[3u * (uint64_t)n + w] = out_offsets[w];
        if (convert && r.status == window::WIN_OK)
            max_written = std::max(max_written, deliver::written_samples(r.n_samples, window_count[w], dv.flags));
        if (!decode) continue;
        if (r.span > (1ull << 40) || (!rs && r.n_samples > r.span)) return FLACGPU_ERR_INVALID_INPUT;  // no stream's positions
        frames[w] = r.n_frames;
        host[n + w] = r.span * per;
        whole += (r.span * per + 15u) & ~(uint64_t)15u;
        if (whole > (1ull << 47)) return FLACGPU_ERR_OUT_OF_MEMORY;
        max_bytes = std::max(max_bytes, r.n_samples * per);
        if (lv) {
            host[4u * (uint64_t)n + w] = n_parts;
            n_parts += levels::partial_records(r.n_samples, pl, c->fmt.channels);
            max_measured = std::max(max_measured, r.n_samples);
        }
    }
    HIPCHK(x->win_pcm.grow(whole + 16u, &st));
    ChunkRun run;
    streams::StreamResult *sres = nullptr;
    levels::Acc *d_parts = nullptr;
    int rc = run.prepare(c, frames, host, x->win, [&](Carve &v) {
        v.take(n, sres);
        if (lv) v.take(n_parts, d_parts);
    }, st);
    if (rc) return rc;
    HIPCHK(launch_window_init(wc.d_recs, sres, run.carried, n, st));
    rc = run.run(c, d_data, d_foff, d_fbytes, x->win_pcm.get(), whole, sres, st);
    if (rc) return rc;
    const uint64_t *d_base = run.row(0), *d_dst = run.row(3);
    if (lv)
        HIPCHK(launch_window_levels(wc.d_recs, sres, x->win_pcm.get(), d_base, d_dst, run.row(4), d_parts, lv->d_peak, lv->d_sum,
                                    lv->d_energy, lv->hop, c->fmt.channels, c->fmt.bytes_per_sample, n, max_measured, st));
    else if (rs)
        HIPCHK(launch_window_resample(wc.d_recs, sres, wc.d_args, rs->d_totals, x->win_pcm.get(), d_base, d_pcm_out, d_dst, dv, rs->rt,
                                      rs->d_coeffs, n, max_written, st));
    else if (convert)
        HIPCHK(launch_window_elements(wc.d_recs, sres, wc.d_args, x->win_pcm.get(), d_base, d_pcm_out, d_dst, dv, n, max_written, st));
    else
        HIPCHK(launch_window_copy(wc.d_recs, sres, x->win_pcm.get(), d_base, d_pcm_out, d_dst, (uint32_t)per, n, max_bytes, st));
    HIPCHK(launch_window_results(wc.d_recs, sres, d_results, n, st));
    return FLACGPU_OK;
}

// The files of a many-files call in one device buffer, the context's d_frames: file i at the
// 64-byte aligned offs[i], lens[i] bytes, uploaded on st.
int upload_files(flacgpu_ctx *c, uint32_t n, const uint8_t *const *p, const size_t *len, std::vector<uint64_t> &offs,
                 std::vector<uint64_t> &lens, hipStream_t st) {
    DecScratch *d = c->dec.get();
    try {
        offs.resize(n);
        lens.resize(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (len[i] > 0xFFFFFFFFull) return FLACGPU_ERR_INVALID_INPUT;
        offs[i] = total;
        lens[i] = len[i];
        total += (len[i] + 63u) & ~(uint64_t)63u;
    }
    HIPCHK(d->d_frames.grow(total + 16u, &st));
    for (uint32_t i = 0; i < n; i++)
        if (len[i]) HIPCHK(hipMemcpyAsync(d->d_frames.get() + offs[i], p[i], len[i], hipMemcpyHostToDevice, st));
    return FLACGPU_OK;
}

// One chunk of a host-buffer decode on the context's stream: the n <= max_frames consecutive
// frames of the table (d_foff, d_fbytes) into d_frames are decoded into the zeroed staging PCM (a
// damaged frame leaves zeros), their results copied to `results`, their PCM to pcm_out + *written;
// *written and *n_samples grow by the chunk's.  `overlap` runs on the host once the work is
// queued, before the wait for it.
template <class F>
int decode_chunk(flacgpu_ctx *c, const uint8_t *d_frames, const uint64_t *d_foff, const uint32_t *d_fbytes, uint32_t n,
                 uint8_t *pcm_out, uint64_t pcm_cap, uint64_t *written, uint64_t *n_samples, dec::Result *results,
                 F overlap) {
    DecScratch *d = c->dec.get();
    hipStream_t st = c->stream.get();
    // (a decode-only context's block_size is its max_block, up to 16384: 64-bit products)
    const uint64_t per = (uint64_t)c->fmt.channels * c->fmt.bytes_per_sample, need = (uint64_t)n * (uint64_t)c->fmt.max_block * per;
    HIPCHK(d->d_pcm.grow(need));  // the chunk before this one was waited for
    HIPCHK(hipMemsetAsync(d->d_pcm.get(), 0, need, st));
    const int rc = dec_core(c, d_frames, d_foff, d_fbytes, n, nullptr, d->d_pcm.get(), need, nullptr, false,
                            (flacgpu_decode_result *)d->d_results, nullptr, st);
    if (rc) return rc;
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(results, d->d_results, (uint64_t)n * sizeof(dec::Result), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, d->total, 8, hipMemcpyDeviceToHost, st));
    overlap();
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t out_bytes = total * per;
    if (out_bytes > need) return FLACGPU_ERR_INTERNAL;
    if (*written + out_bytes > pcm_cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
    if (out_bytes) HIPCHK(hipMemcpy(pcm_out + *written, d->d_pcm.get(), out_bytes, hipMemcpyDeviceToHost));
    *written += out_bytes;
    *n_samples += total;
    return FLACGPU_OK;
}

}  // namespace

extern "C" {

int flacgpu_decode_frames_device(flacgpu_ctx *c, const uint8_t *d_frames, const uint64_t *d_frame_offsets,
                                 const uint32_t *d_frame_bytes, uint64_t n_frames, const uint64_t *d_pcm_offsets,
                                 uint8_t *d_pcm_out, uint64_t pcm_cap, const uint8_t *d_pcm_expect,
                                 flacgpu_decode_result *d_results, uint32_t *d_bad_count, void *hip_stream) {
    if (!c || !d_frames || !d_frame_offsets || !d_frame_bytes || !d_results || !d_bad_count || n_frames > c->max_frames)
        return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    const int rc = dec_scratch(c);
    if (rc) return rc;
    hipStream_t st = pick_stream(c, hip_stream);
    if (n_frames == 0) {
        HIPCHK(hipMemsetAsync(d_bad_count, 0, 4, st));
        return FLACGPU_OK;
    }
    return dec_core(c, d_frames, d_frame_offsets, d_frame_bytes, (uint32_t)n_frames, d_pcm_offsets, d_pcm_out, pcm_cap,
                    d_pcm_expect, false, d_results, d_bad_count, st);
}

int flacgpu_verify_plan_device(flacgpu_ctx *c, const flacgpu_plan *p, const void *d_pcm, const uint8_t *d_out,
                               const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                               flacgpu_decode_result *d_results, uint32_t *d_bad_count, void *hip_stream) {
    if (!c) return FLACGPU_ERR_INVALID_INPUT;
    FG_ENCODER_ONLY(c);  // a plan is an encoder context's
    if (!p || p->ctx != c || !d_pcm || !d_out || !d_frame_offsets || !d_frame_bytes || !d_results || !d_bad_count ||
        p->n_frames > c->max_frames)
        return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    const int rc = dec_scratch(c);
    if (rc) return rc;
    hipStream_t st = pick_stream(c, hip_stream);
    if (p->n_frames == 0) {
        HIPCHK(hipMemsetAsync(d_bad_count, 0, 4, st));
        return FLACGPU_OK;
    }
    DecScratch *d = c->dec.get();
    // the plan's frame table (full jobs, then tail jobs) by output slot
    HIPCHK(launch_dec_expect(p->d_jobs.get(), p->n_frames, d->exp_off, d->exp_number, d->exp_n, st));
    return dec_core(c, d_out, d_frame_offsets, d_frame_bytes, (uint32_t)p->n_frames, d->exp_off, nullptr, 0,
                    (const uint8_t *)d_pcm, true, d_results, d_bad_count, st);
}

int flacgpu_flac_index_device(flacgpu_ctx *c, const uint8_t *d_data, uint64_t len, uint32_t stream_bits,
                              uint32_t stream_rate, uint64_t *d_frame_offsets, uint32_t *d_frame_bytes, uint64_t cap,
                              flacgpu_index_result *d_result, void *hip_stream) {
    if (!c || !d_data || !d_frame_offsets || !d_frame_bytes || !d_result || len > 0xFFFFFFFFull)
        return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = pick_stream(c, hip_stream);
    if (len == 0) {  // no frames: OK, 0
        HIPCHK(hipMemsetAsync(d_result, 0, sizeof(flacgpu_index_result), st));
        return FLACGPU_OK;
    }
    return index_core(c, d_data, len, stream_bits, stream_rate, d_frame_offsets, d_frame_bytes, cap,
                      (idx::IndexResult *)d_result, st);
}

int flacgpu_flac_index_streams_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams,
                                      const uint64_t *stream_offsets, const uint64_t *stream_lens,
                                      const uint32_t *stream_bits, const uint32_t *stream_rates,
                                      const uint64_t *table_first, const uint64_t *table_caps, uint64_t *d_frame_offsets,
                                      uint32_t *d_frame_bytes, flacgpu_index_result *d_results, void *hip_stream) {
    if (!c || !d_data || !stream_offsets || !stream_lens || !table_first || !table_caps || !d_frame_offsets ||
        !d_frame_bytes || !d_results || !streams_args_ok(n_streams, stream_lens))
        return FLACGPU_ERR_INVALID_INPUT;
    if (n_streams == 0) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    return index_streams_core(c, d_data, n_streams, stream_offsets, stream_lens, stream_bits, stream_rates, table_first,
                              table_caps, d_frame_offsets, d_frame_bytes, (idx::IndexResult *)d_results,
                              pick_stream(c, hip_stream));
}

int flacgpu_decode_streams_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *stream_offsets,
                                  const uint64_t *stream_lens, const uint32_t *stream_bits, const uint32_t *stream_rates,
                                  uint8_t *d_pcm_out, const uint64_t *pcm_offsets, const uint64_t *pcm_caps,
                                  flacgpu_stream_result *d_results, uint8_t *d_md5, void *hip_stream) {
    if (!c || !d_data || !stream_offsets || !stream_lens || !d_pcm_out || !pcm_offsets || !pcm_caps || !d_results ||
        !streams_args_ok(n_streams, stream_lens))
        return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t s = 0; s < n_streams; s++) {
        if (pcm_offsets[s] + pcm_caps[s] < pcm_offsets[s]) return FLACGPU_ERR_INVALID_INPUT;
        if (d_md5 && (pcm_offsets[s] & 3u)) return FLACGPU_ERR_INVALID_INPUT;  // the MD5 kernel loads words
    }
    if (n_streams == 0) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    hipStream_t st = pick_stream(c, hip_stream);
    StreamTables tb;
    std::vector<idx::IndexResult> ires;
    rc = streams_index(c, d_data, n_streams, stream_offsets, stream_lens, stream_bits, stream_rates, tb, ires, st);
    if (rc) return rc;
    return streams_decode(c, d_data, n_streams, tb, ires, d_pcm_out, pcm_offsets, pcm_caps, (streams::StreamResult *)d_results,
                          d_md5, st);
}

int flacgpu_flac_positions_streams_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams,
                                          const uint64_t *table_first, const uint64_t *table_caps,
                                          const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                          const flacgpu_index_result *d_index_results, const uint32_t *stream_bits,
                                          const uint32_t *stream_rates, uint64_t *d_frame_first_sample,
                                          uint64_t *d_stream_samples, void *hip_stream) {
    if (!c || !d_data || !table_first || !table_caps || !d_frame_offsets || !d_frame_bytes || !d_index_results ||
        !d_frame_first_sample || !d_stream_samples || n_streams > idx::kIdxMaxStreams)
        return FLACGPU_ERR_INVALID_INPUT;
    if (n_streams == 0) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    return positions_core(c, d_data, n_streams, table_first, table_caps, d_frame_offsets, d_frame_bytes,
                          (const idx::IndexResult *)d_index_results, stream_bits, stream_rates, d_frame_first_sample,
                          d_stream_samples, pick_stream(c, hip_stream));
}

namespace {

// flacgpu_decode_windows_device (format SAMPLE_BYTES, no flags: offsets and caps in bytes),
// flacgpu_decode_windows_device_as (offsets and caps in elements) and
// flacgpu_decode_windows_device_mix (`masks`: its out_channels channel masks, else NULL) behind
// their own checks; with src_rate != 0 flacgpu_decode_windows_device_resample: windows, offsets and
// caps in output samples and elements at dst_rate.  `weights` (host, out_channels x C, never with
// masks): the weighted mix of flacgpu_decode_windows_device_to in place of the masks.
int windows_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                   const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes, const flacgpu_index_result *d_index_results,
                   const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples, uint32_t n_windows,
                   const uint32_t *window_stream, const uint64_t *window_start, const uint64_t *window_count,
                   uint32_t sample_format, uint32_t flags, uint32_t out_channels, const uint8_t *masks, void *d_out,
                   const uint64_t *offsets, const uint64_t *caps, flacgpu_window_result *d_results, void *hip_stream,
                   uint32_t src_rate = 0, uint32_t dst_rate = 0, const float *weights = nullptr, const Levels *lv = nullptr) {
    if (!c || !d_data || !table_first || !d_frame_offsets || !d_frame_bytes || !d_index_results || !d_frame_first_sample ||
        !d_stream_samples || n_windows > 65535u)
        return FLACGPU_ERR_INVALID_INPUT;
    if (n_windows && (!window_stream || !window_start || !window_count || (!d_out && !lv) || !offsets || !caps || !d_results))
        return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t w = 0; w < n_windows; w++)
        if (window_stream[w] >= n_streams || offsets[w] + caps[w] < offsets[w]) return FLACGPU_ERR_INVALID_INPUT;
    deliver::Delivery dv = deliver::identity_delivery(sample_format, flags, c->fmt.channels, c->fmt.bytes_per_sample);
    if (masks) {
        if (!deliver::mix_valid(c->fmt.channels, out_channels, masks, sample_format)) return FLACGPU_ERR_INVALID_INPUT;
        dv.mix = deliver::MIX_MASKS;
        dv.out_channels = out_channels;
        for (uint32_t k = 0; k < deliver::kMixMaxChannels; k++) dv.masks[k] = k < out_channels ? masks[k] : (uint8_t)0;
    } else if (weights) {
        if (!deliver::mixw_valid(c->fmt.channels, out_channels, weights, sample_format)) return FLACGPU_ERR_INVALID_INPUT;
        dv.mix = deliver::MIX_WEIGHTS;
        dv.out_channels = out_channels;
        for (uint32_t k = 0; k < deliver::kMixMaxChannels; k++) dv.masks[k] = 0;
    }
    Resampling rs{{0, 0, 0, 0}, nullptr, d_stream_samples};
    if (src_rate && !resample::valid_ratio(src_rate, dst_rate, &rs.rt)) return FLACGPU_ERR_INVALID_INPUT;
    if (n_windows == 0) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    hipStream_t st = pick_stream(c, hip_stream);
    if (src_rate) {
        rc = resample_table(c, rs.rt, src_rate, dst_rate, &rs.d_coeffs, st);
        if (rc) return rc;
    }
    if (weights) {
        rc = mix_weights(c, out_channels, c->fmt.channels, weights, &dv.weights, st);
        if (rc) return rc;
    }
    WindowsCall wc;
    rc = windows_cover(c, table_first, (const idx::IndexResult *)d_index_results, d_frame_first_sample, d_stream_samples,
                       n_windows, window_stream, window_start, window_count, caps, dv, wc, st, src_rate ? &rs : nullptr, lv);
    if (rc) return rc;
    return windows_decode(c, d_data, table_first, d_frame_offsets, d_frame_bytes, wc, window_stream, window_count, dv,
                          (uint8_t *)d_out, offsets, (window::WindowResult *)d_results, st, src_rate ? &rs : nullptr, lv);
}

}  // namespace

int flacgpu_levels_windows_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                                  const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                  const flacgpu_index_result *d_index_results, const uint64_t *d_frame_first_sample,
                                  const uint64_t *d_stream_samples, uint32_t n_windows, const uint32_t *window_stream,
                                  const uint64_t *window_start, const uint64_t *window_count, uint32_t hop, uint32_t *d_peak,
                                  int64_t *d_sum, double *d_energy, const uint64_t *out_offsets, const uint64_t *out_caps,
                                  flacgpu_window_result *d_results, void *hip_stream) {
    if (!c || hop == 0u || hop > levels::kMaxHop || !d_peak || !d_sum || !d_energy || ((uintptr_t)d_peak & 3u) ||
        ((uintptr_t)d_sum & 7u) || ((uintptr_t)d_energy & 7u))
        return FLACGPU_ERR_INVALID_INPUT;
    const Levels lv{hop, d_peak, d_sum, d_energy};
    return windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                          d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                          deliver::SAMPLE_BYTES, 0u, 0u, nullptr, nullptr, out_offsets, out_caps, d_results, hip_stream, 0u, 0u,
                          nullptr, &lv);
}

int flacgpu_decode_windows_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                                  const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                  const flacgpu_index_result *d_index_results, const uint64_t *d_frame_first_sample,
                                  const uint64_t *d_stream_samples, uint32_t n_windows, const uint32_t *window_stream,
                                  const uint64_t *window_start, const uint64_t *window_count, uint8_t *d_pcm_out,
                                  const uint64_t *pcm_offsets, const uint64_t *pcm_caps, flacgpu_window_result *d_results,
                                  void *hip_stream) {
    return windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                          d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                          deliver::SAMPLE_BYTES, 0u, 0u, nullptr, d_pcm_out, pcm_offsets, pcm_caps, d_results, hip_stream);
}

int flacgpu_decode_windows_device_as(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                                     const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                     const flacgpu_index_result *d_index_results, const uint64_t *d_frame_first_sample,
                                     const uint64_t *d_stream_samples, uint32_t n_windows, const uint32_t *window_stream,
                                     const uint64_t *window_start, const uint64_t *window_count, uint32_t sample_format,
                                     uint32_t flags, void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                     flacgpu_window_result *d_results, void *hip_stream) {
    if (!c || sample_format >= deliver::SAMPLE_FORMATS || (flags & ~deliver::DELIVER_FLAGS) ||
        ((uintptr_t)d_out & (deliver::elem_size(sample_format) - 1u)))
        return FLACGPU_ERR_INVALID_INPUT;
    return windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                          d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                          sample_format, flags, 0u, nullptr, d_out, out_offsets, out_caps, d_results, hip_stream);
}

int flacgpu_decode_windows_device_mix(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                                      const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                      const flacgpu_index_result *d_index_results, const uint64_t *d_frame_first_sample,
                                      const uint64_t *d_stream_samples, uint32_t n_windows, const uint32_t *window_stream,
                                      const uint64_t *window_start, const uint64_t *window_count, uint32_t sample_format,
                                      uint32_t flags, uint32_t out_channels, const uint8_t *channel_masks, void *d_out,
                                      const uint64_t *out_offsets, const uint64_t *out_caps, flacgpu_window_result *d_results,
                                      void *hip_stream) {
    if (!c || sample_format >= deliver::SAMPLE_FORMATS || (flags & ~deliver::DELIVER_FLAGS) ||
        ((uintptr_t)d_out & (deliver::elem_size(sample_format) - 1u)) || !channel_masks || out_channels < 1u ||
        out_channels > deliver::kMixMaxChannels)
        return FLACGPU_ERR_INVALID_INPUT;
    return windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                          d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                          sample_format, flags, out_channels, channel_masks, d_out, out_offsets, out_caps, d_results,
                          hip_stream);
}

int flacgpu_decode_windows_device_resample(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams,
                                           const uint64_t *table_first, const uint64_t *d_frame_offsets,
                                           const uint32_t *d_frame_bytes, const flacgpu_index_result *d_index_results,
                                           const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                           uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                           const uint64_t *window_count, uint32_t sample_format, uint32_t flags,
                                           uint32_t out_channels, const uint8_t *channel_masks, uint32_t src_rate,
                                           uint32_t dst_rate, void *d_out, const uint64_t *out_offsets, const uint64_t *out_caps,
                                           flacgpu_window_result *d_results, void *hip_stream) {
    if (!c || sample_format >= deliver::SAMPLE_FORMATS || sample_format == deliver::SAMPLE_I32 ||
        (flags & ~deliver::DELIVER_FLAGS) || ((uintptr_t)d_out & (deliver::elem_size(sample_format) - 1u)) ||
        !resample::valid_ratio(src_rate, dst_rate, nullptr))
        return FLACGPU_ERR_INVALID_INPUT;
    if (channel_masks && (out_channels < 1u || out_channels > deliver::kMixMaxChannels)) return FLACGPU_ERR_INVALID_INPUT;
    return windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                          d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                          sample_format, flags, out_channels, channel_masks, d_out, out_offsets, out_caps, d_results, hip_stream,
                          src_rate, dst_rate);
}

}  // extern "C"

namespace {

// An operand table of k_features: `cols` columns of `depth` entries as blocks of 64 lanes x 4 floats,
// block (column tile ct, k block kb, plane p of `planes`) at ((ct * nkb + kb) * planes + p) * 256,
// lane l's float s the entry of column ct * 16 + (l & 15) at k = kb * 16 + 4 s + (l >> 4); zero
// where the column or k is past the table's.  at(p, col, k): the entry.
template <class At>
int feat_blocks(uint32_t planes, uint32_t cols, uint32_t depth, At at, std::vector<float> &blk) {
    const uint32_t nct = (cols + 15u) / 16u, nkb = (depth + 15u) / 16u;
    try {
        blk.assign((size_t)nct * nkb * planes * 256u, 0.0f);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    size_t o = 0;
    for (uint32_t ct = 0; ct < nct; ct++)
        for (uint32_t kb = 0; kb < nkb; kb++)
            for (uint32_t p = 0; p < planes; p++)
                for (uint32_t l = 0; l < 64u; l++)
                    for (uint32_t s = 0; s < 4u; s++, o++) {
                        const uint32_t col = ct * 16u + (l & 15u), k = kb * 16u + 4u * s + (l >> 4);
                        if (col < cols && k < depth) blk[o] = at(p, col, k);
                    }
    return FLACGPU_OK;
}

int feat_upload(const std::vector<float> &blk, DevBuf<float> &d, hipStream_t st) {
    HIPCHK(d.grow(blk.size()));
    HIPCHK(hipMemcpyAsync(d.get(), blk.data(), blk.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // blk goes out of scope
    return FLACGPU_OK;
}

// The device STFT table of n_fft: flacgpu_features_table's, in operand blocks (the cos and the sin
// plane of a block side by side), uploaded by the first call of the context that needs it, which
// waits for st once more than the others; kept for the context's life.
int feat_table(flacgpu_ctx *c, uint32_t N, const float **d_table, hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    for (const FeatTable &t : x->feat_tables)
        if (t.n_fft == N) {
            *d_table = t.blocks.get();
            return FLACGPU_OK;
        }
    const uint32_t B = N / 2u + 1u;
    std::vector<float> h, blk;
    size_t n = 0;
    try {
        h.resize((size_t)2u * B * N);
        x->feat_tables.reserve(x->feat_tables.size() + 1u);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    int rc = flacgpu_features_table(N, h.data(), h.size(), &n);
    if (rc) return rc;
    rc = feat_blocks(2u, B, N, [&](uint32_t p, uint32_t b, uint32_t k) { return h[((size_t)p * B + b) * N + k]; }, blk);
    if (rc) return rc;
    DevBuf<float> d;
    rc = feat_upload(blk, d, st);
    if (rc) return rc;
    *d_table = d.get();
    x->feat_tables.push_back({N, std::move(d)});
    return FLACGPU_OK;
}

// The device copy of a filter bank F[R][B], found again by its content; a new one is uploaded as
// the table is.  The context keeps the last kMaxFeatFilters banks: before the oldest is dropped st
// is waited for, since work queued on it may still read that bank.
int feat_filter(flacgpu_ctx *c, uint32_t R, uint32_t B, const float *F, const float **d_filters, hipStream_t st) {
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    const size_t n = (size_t)R * B;
    for (const FeatFilter &f : x->feat_filters)
        if (f.rows == R && f.bins == B && std::memcmp(f.host.data(), F, n * sizeof(float)) == 0) {
            *d_filters = f.blocks.get();
            return FLACGPU_OK;
        }
    FeatFilter f;
    std::vector<float> blk;
    try {
        f.host.assign(F, F + n);
        x->feat_filters.reserve(x->feat_filters.size() + 1u);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    f.rows = R;
    f.bins = B;
    int rc = feat_blocks(1u, R, B, [&](uint32_t, uint32_t r, uint32_t b) { return F[(size_t)r * B + b]; }, blk);
    if (rc) return rc;
    rc = feat_upload(blk, f.blocks, st);
    if (rc) return rc;
    if (x->feat_filters.size() >= kMaxFeatFilters) {
        HIPCHK(hipStreamSynchronize(st));
        x->feat_filters.erase(x->feat_filters.begin());
    }
    *d_filters = f.blocks.get();
    x->feat_filters.push_back(std::move(f));
    return FLACGPU_OK;
}

// The one body of the feature delivery, in two stages.  Stage 1 is windows_device itself: every
// window's extended span [start - N / 2, + (frames - 1) * H + N), clipped at the stream's start on
// the host (`clip` samples that k_features reads as zeros), goes as planar padded F32 into the
// context's scratch.  Stage 2, k_features, reads those planes and stage 1's results and writes the
// elements and the results.  `weights` (host, out_channels x C, never with masks): stage 1 mixes by
// the weighted rule, as flacgpu_decode_windows_device_to asks.
int features_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                    const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes, const flacgpu_index_result *d_index_results,
                    const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples, uint32_t n_windows,
                    const uint32_t *window_stream, const uint64_t *window_start, const uint64_t *window_frames,
                    uint32_t sample_format, uint32_t out_channels, const uint8_t *channel_masks, const float *weights,
                    uint32_t src_rate, uint32_t dst_rate, const flacgpu_features *ft, const float *filters, void *d_out,
                    const uint64_t *out_offsets, const uint64_t *out_caps, flacgpu_window_result *d_results, void *hip_stream) {
    if (!c || !ft || !d_data || !table_first || !d_frame_offsets || !d_frame_bytes || !d_index_results ||
        !d_frame_first_sample || !d_stream_samples || n_windows > 65535u)
        return FLACGPU_ERR_INVALID_INPUT;
    const feat::Params p{ft->n_fft, ft->hop, ft->n_rows};
    if (!feat::valid(p) || (p.n_rows && !filters)) return FLACGPU_ERR_INVALID_INPUT;
    if (sample_format != deliver::SAMPLE_F32 && sample_format != deliver::SAMPLE_F16 && sample_format != deliver::SAMPLE_BF16)
        return FLACGPU_ERR_INVALID_INPUT;
    if ((uintptr_t)d_out & (deliver::elem_size(sample_format) - 1u)) return FLACGPU_ERR_INVALID_INPUT;
    if (n_windows && (!window_stream || !window_start || !window_frames || !d_out || !out_offsets || !out_caps || !d_results))
        return FLACGPU_ERR_INVALID_INPUT;
    if (channel_masks && !deliver::mix_valid(c->fmt.channels, out_channels, channel_masks, sample_format))
        return FLACGPU_ERR_INVALID_INPUT;
    if (weights && (channel_masks || !deliver::mixw_valid(c->fmt.channels, out_channels, weights, sample_format)))
        return FLACGPU_ERR_INVALID_INPUT;
    resample::Ratio rt{0, 0, 0, 0};
    if ((src_rate || dst_rate) && !resample::valid_ratio(src_rate, dst_rate, &rt)) return FLACGPU_ERR_INVALID_INPUT;
    const uint32_t B = feat::bins(p), n_rows = feat::rows(p), K = channel_masks || weights ? out_channels : c->fmt.channels;
    for (size_t i = 0; i < (size_t)p.n_rows * B; i++)
        if (!std::isfinite(filters[i])) return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t w = 0; w < n_windows; w++) {
        if (window_stream[w] >= n_streams || out_offsets[w] + out_caps[w] < out_offsets[w]) return FLACGPU_ERR_INVALID_INPUT;
        if (window_frames[w] && window_frames[w] - 1u > (0x7FFFFFFFull - p.n_fft) / p.hop) return FLACGPU_ERR_INVALID_INPUT;
    }
    if (n_windows == 0) return FLACGPU_OK;
    const FeatGeometry g = feat_geometry(p.n_fft, p.hop, p.n_rows);
    std::vector<FeatWindow> fw;
    std::vector<uint64_t> s_start, s_count, s_off, s_cap;
    try {
        fw.resize(n_windows);
        s_start.resize(n_windows);
        s_count.resize(n_windows);
        s_off.resize(n_windows);
        s_cap.resize(n_windows);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    uint64_t x_total = 0, max_items = 0;
    const uint32_t half = p.n_fft / 2u;
    for (uint32_t w = 0; w < n_windows; w++) {
        const uint64_t frames = window_frames[w], start = window_start[w];  // frames < 2^31: no product below passes 2^45
        FeatWindow &f = fw[w];
        f.too_small = (uint64_t)K * n_rows * frames > out_caps[w] ? 1u : 0u;
        f.clip = start < half ? (uint32_t)(half - start) : 0u;
        f.frames = (uint32_t)frames;
        f.stream = window_stream[w];
        f.start = start;
        f.out_off = out_offsets[w];
        f.x_off = x_total;
        f.count = f.too_small ? 0u : feat::span(p, frames) - (frames ? f.clip : 0u);  // a TOO_SMALL window is dropped from stage 1
        s_start[w] = f.count ? start + f.clip - half : 0u;
        s_count[w] = f.count;
        s_off[w] = f.x_off;
        s_cap[w] = (uint64_t)K * f.count;
        x_total += (s_cap[w] + 3u) & ~(uint64_t)3u;
        if (f.count) max_items = std::max(max_items, (uint64_t)K * ((frames + g.frames - 1u) / g.frames));
    }
    if (x_total > (1ull << 45)) return FLACGPU_ERR_OUT_OF_MEMORY;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    DecScratch *d = c->dec.get();
    hipStream_t st = pick_stream(c, hip_stream);
    const float *d_table = nullptr, *d_filters = nullptr;
    rc = feat_table(c, p.n_fft, &d_table, st);
    if (rc) return rc;
    if (p.n_rows) {
        rc = feat_filter(c, p.n_rows, B, filters, &d_filters, st);
        if (rc) return rc;
    }
    HIPCHK(d->feat_x.grow(x_total + 4u, &st));  // an earlier call on this stream may still read the old one
    FeatWindow *d_fw = nullptr;
    window::WindowResult *d_s1 = nullptr;
    auto carve = [&](uint8_t *base) {
        Carve v{base};
        v.take(n_windows, d_fw);
        return v.take(n_windows, d_s1);
    };
    HIPCHK(fit(d->feat_win, carve, &st));
    HIPCHK(hipMemcpyAsync(d_fw, fw.data(), (uint64_t)n_windows * sizeof(FeatWindow), hipMemcpyHostToDevice, st));
    rc = windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                        d_stream_samples, n_windows, window_stream, s_start.data(), s_count.data(), deliver::SAMPLE_F32,
                        deliver::DELIVER_PLANAR | deliver::DELIVER_PAD, out_channels, channel_masks, d->feat_x.get(), s_off.data(),
                        s_cap.data(), (flacgpu_window_result *)d_s1, hip_stream, src_rate, dst_rate, weights);
    if (rc) return rc;
    HIPCHK(launch_features(d_fw, d_s1, d_stream_samples, rt, d->feat_x.get(), d_table, d_filters, (uint8_t *)d_out,
                           (window::WindowResult *)d_results, p, K, sample_format, n_windows, max_items, st));
    return FLACGPU_OK;
}

// The one body of the filtered delivery, in two stages shaped as features_device's.  Stage 1 is
// windows_device itself: every window's span [start + d - (T - 1), start + count + d) of its filter,
// clipped at the stream's start on the host (`clip` samples that k_window_fir reads as zeros), goes as
// planar padded F32 into the context's scratch (feat_x and feat_win: a call is one delivery or the
// other).  Stage 2, k_window_fir, reads those planes, stage 1's results and the caller's taps and
// writes the elements and the results; the capacity rule is deliver::too_small's over the window's
// own n, which only the device knows, so k_window_fir applies it.
int fir_device(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
               const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes, const flacgpu_index_result *d_index_results,
               const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples, uint32_t n_windows,
               const uint32_t *window_stream, const uint64_t *window_start, const uint64_t *window_count,
               const flacgpu_window_delivery *how, const float *d_taps, uint64_t taps_len, uint32_t n_filters,
               const flacgpu_fir *filters, const uint32_t *window_filter, void *d_out, const uint64_t *out_offsets,
               const uint64_t *out_caps, flacgpu_window_result *d_results, void *hip_stream) {
    if (!c || !how || how->size != sizeof(flacgpu_window_delivery) || how->features || (how->channel_masks && how->channel_weights))
        return FLACGPU_ERR_INVALID_INPUT;
    if (!d_data || !table_first || !d_frame_offsets || !d_frame_bytes || !d_index_results || !d_frame_first_sample ||
        !d_stream_samples || n_windows > 65535u)
        return FLACGPU_ERR_INVALID_INPUT;
    const uint32_t format = how->sample_format, flags = how->flags;
    if (format != deliver::SAMPLE_F32 && format != deliver::SAMPLE_F16 && format != deliver::SAMPLE_BF16)
        return FLACGPU_ERR_INVALID_INPUT;
    if ((flags & ~deliver::DELIVER_FLAGS) || ((uintptr_t)d_out & (deliver::elem_size(format) - 1u))) return FLACGPU_ERR_INVALID_INPUT;
    const uint8_t *masks = how->channel_masks;
    const float *weights = how->channel_weights;
    if (masks && !deliver::mix_valid(c->fmt.channels, how->out_channels, masks, format)) return FLACGPU_ERR_INVALID_INPUT;
    if (weights && !deliver::mixw_valid(c->fmt.channels, how->out_channels, weights, format)) return FLACGPU_ERR_INVALID_INPUT;
    resample::Ratio rt{0, 0, 0, 0};
    if ((how->src_rate || how->dst_rate) && !resample::valid_ratio(how->src_rate, how->dst_rate, &rt)) return FLACGPU_ERR_INVALID_INPUT;
    const uint32_t K = masks || weights ? how->out_channels : c->fmt.channels;
    if (n_filters && (!d_taps || ((uintptr_t)d_taps & 3u) || !filters)) return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t f = 0; f < n_filters; f++) {
        const fir::Filter ff{filters[f].offset, filters[f].taps, filters[f].delay, filters[f].rows, filters[f].reserved};
        if (!fir::filter_valid(ff, K, taps_len)) return FLACGPU_ERR_INVALID_INPUT;
    }
    if (n_windows && (!window_stream || !window_start || !window_count || !window_filter || !d_out || !out_offsets || !out_caps ||
                      !d_results))
        return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t w = 0; w < n_windows; w++) {
        if (window_stream[w] >= n_streams || out_offsets[w] + out_caps[w] < out_offsets[w] || window_filter[w] >= n_filters)
            return FLACGPU_ERR_INVALID_INPUT;
        if (!fir::span_valid(window_count[w], filters[window_filter[w]].taps)) return FLACGPU_ERR_INVALID_INPUT;
    }
    if (n_windows == 0) return FLACGPU_OK;
    std::vector<FirWindow> fw;
    std::vector<uint64_t> s_start, s_count, s_off, s_cap;
    try {
        fw.resize(n_windows);
        s_start.resize(n_windows);
        s_count.resize(n_windows);
        s_off.resize(n_windows);
        s_cap.resize(n_windows);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    uint64_t x_total = 0, max_items = 0;
    const uint32_t tile = fir_geometry(1u).tile;  // the same for every T
    for (uint32_t w = 0; w < n_windows; w++) {
        const flacgpu_fir &f = filters[window_filter[w]];
        const fir::Span sp = fir::span(window_start[w], window_count[w], f.taps, f.delay);
        FirWindow &a = fw[w];
        a.x_off = x_total;
        a.s_count = sp.count;
        a.start = window_start[w];
        a.out_off = out_offsets[w];
        a.cap = out_caps[w];
        a.tap_off = f.offset;
        a.count = (uint32_t)window_count[w];
        a.clip = sp.clip;
        a.stream = window_stream[w];
        a.taps = f.taps;
        a.rows = f.rows;
        a.pad = 0u;
        s_start[w] = sp.first;
        s_count[w] = sp.count;
        s_off[w] = a.x_off;
        s_cap[w] = (uint64_t)K * sp.count;
        x_total += (s_cap[w] + 3u) & ~(uint64_t)3u;
        max_items = std::max(max_items, (uint64_t)K * ((window_count[w] + tile - 1u) / tile));
    }
    if (x_total > (1ull << 45)) return FLACGPU_ERR_OUT_OF_MEMORY;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    DecScratch *d = c->dec.get();
    hipStream_t st = pick_stream(c, hip_stream);
    HIPCHK(d->feat_x.grow(x_total + 4u, &st));  // an earlier call on this stream may still read the old one
    FirWindow *d_fw = nullptr;
    window::WindowResult *d_s1 = nullptr;
    auto carve = [&](uint8_t *base) {
        Carve v{base};
        v.take(n_windows, d_fw);
        return v.take(n_windows, d_s1);
    };
    HIPCHK(fit(d->feat_win, carve, &st));
    HIPCHK(hipMemcpyAsync(d_fw, fw.data(), (uint64_t)n_windows * sizeof(FirWindow), hipMemcpyHostToDevice, st));
    rc = windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                        d_stream_samples, n_windows, window_stream, s_start.data(), s_count.data(), deliver::SAMPLE_F32,
                        deliver::DELIVER_PLANAR | deliver::DELIVER_PAD, how->out_channels, masks, d->feat_x.get(), s_off.data(),
                        s_cap.data(), (flacgpu_window_result *)d_s1, hip_stream, how->src_rate, how->dst_rate, weights);
    if (rc) return rc;
    HIPCHK(launch_window_fir(d_fw, d_s1, d_stream_samples, rt, d->feat_x.get(), d_taps, (uint8_t *)d_out,
                             (window::WindowResult *)d_results, K, format, flags, n_windows, max_items, st));
    return FLACGPU_OK;
}

}  // namespace

extern "C" {

int flacgpu_decode_windows_device_features(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams,
                                           const uint64_t *table_first, const uint64_t *d_frame_offsets,
                                           const uint32_t *d_frame_bytes, const flacgpu_index_result *d_index_results,
                                           const uint64_t *d_frame_first_sample, const uint64_t *d_stream_samples,
                                           uint32_t n_windows, const uint32_t *window_stream, const uint64_t *window_start,
                                           const uint64_t *window_frames, uint32_t sample_format, uint32_t out_channels,
                                           const uint8_t *channel_masks, uint32_t src_rate, uint32_t dst_rate,
                                           const flacgpu_features *ft, const float *filters, void *d_out,
                                           const uint64_t *out_offsets, const uint64_t *out_caps,
                                           flacgpu_window_result *d_results, void *hip_stream) {
    return features_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                           d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_frames,
                           sample_format, out_channels, channel_masks, nullptr, src_rate, dst_rate, ft, filters, d_out, out_offsets,
                           out_caps, d_results, hip_stream);
}

// The delivery as a struct.  Without weights it is the existing call the struct describes, behind
// that call's own checks; with weights the same bodies (windows_device, features_device) run the
// weighted mix in place of the masks.
int flacgpu_decode_windows_device_to(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                                     const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                     const flacgpu_index_result *d_index_results, const uint64_t *d_frame_first_sample,
                                     const uint64_t *d_stream_samples, uint32_t n_windows, const uint32_t *window_stream,
                                     const uint64_t *window_start, const uint64_t *window_count,
                                     const flacgpu_window_delivery *how, void *d_out, const uint64_t *out_offsets,
                                     const uint64_t *out_caps, flacgpu_window_result *d_results, void *hip_stream) {
    if (!c || !how || how->size != sizeof(flacgpu_window_delivery) || (how->channel_masks && how->channel_weights))
        return FLACGPU_ERR_INVALID_INPUT;
    if (how->features && how->flags) return FLACGPU_ERR_INVALID_INPUT;
    const bool rates = how->src_rate || how->dst_rate;
    const float *W = how->channel_weights;
    if (how->features)
        return features_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                               d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                               how->sample_format, how->out_channels, how->channel_masks, W, how->src_rate, how->dst_rate,
                               how->features, how->filters, d_out, out_offsets, out_caps, d_results, hip_stream);
    if (!W) {
        if (rates)
            return flacgpu_decode_windows_device_resample(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes,
                                                          d_index_results, d_frame_first_sample, d_stream_samples, n_windows,
                                                          window_stream, window_start, window_count, how->sample_format,
                                                          how->flags, how->out_channels, how->channel_masks, how->src_rate,
                                                          how->dst_rate, d_out, out_offsets, out_caps, d_results, hip_stream);
        if (how->channel_masks)
            return flacgpu_decode_windows_device_mix(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes,
                                                     d_index_results, d_frame_first_sample, d_stream_samples, n_windows,
                                                     window_stream, window_start, window_count, how->sample_format, how->flags,
                                                     how->out_channels, how->channel_masks, d_out, out_offsets, out_caps,
                                                     d_results, hip_stream);
        return flacgpu_decode_windows_device_as(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                                                d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start,
                                                window_count, how->sample_format, how->flags, d_out, out_offsets, out_caps,
                                                d_results, hip_stream);
    }
    // weights: the checks of _as (or of _resample), then the matrix over the context's channels
    if (how->sample_format >= deliver::SAMPLE_FORMATS || (how->flags & ~deliver::DELIVER_FLAGS) ||
        ((uintptr_t)d_out & (deliver::elem_size(how->sample_format) - 1u)) ||
        (rates && !resample::valid_ratio(how->src_rate, how->dst_rate, nullptr)) ||
        !deliver::mixw_valid(c->fmt.channels, how->out_channels, W, how->sample_format))
        return FLACGPU_ERR_INVALID_INPUT;
    return windows_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results,
                          d_frame_first_sample, d_stream_samples, n_windows, window_stream, window_start, window_count,
                          how->sample_format, how->flags, how->out_channels, nullptr, d_out, out_offsets, out_caps, d_results,
                          hip_stream, how->src_rate, how->dst_rate, W);
}

int flacgpu_decode_windows_device_fir(flacgpu_ctx *c, const uint8_t *d_data, uint32_t n_streams, const uint64_t *table_first,
                                      const uint64_t *d_frame_offsets, const uint32_t *d_frame_bytes,
                                      const flacgpu_index_result *d_index_results, const uint64_t *d_frame_first_sample,
                                      const uint64_t *d_stream_samples, uint32_t n_windows, const uint32_t *window_stream,
                                      const uint64_t *window_start, const uint64_t *window_count,
                                      const flacgpu_window_delivery *how, const float *d_taps, uint64_t taps_len,
                                      uint32_t n_filters, const flacgpu_fir *filters, const uint32_t *window_filter, void *d_out,
                                      const uint64_t *out_offsets, const uint64_t *out_caps, flacgpu_window_result *d_results,
                                      void *hip_stream) {
    return fir_device(c, d_data, n_streams, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                      d_stream_samples, n_windows, window_stream, window_start, window_count, how, d_taps, taps_len, n_filters,
                      filters, window_filter, d_out, out_offsets, out_caps, d_results, hip_stream);
}

// every chunk's frames and frame table are uploaded, its results land at results + f0
int flacgpu_decode_frames(flacgpu_ctx *c, const uint8_t *frames, const uint32_t *frame_bytes, uint64_t n_frames,
                          uint8_t *pcm_out, size_t pcm_cap, uint64_t *n_samples, flacgpu_decode_result *results) {
    if (!c || !n_samples || !results || (n_frames && (!frames || !frame_bytes)) || (pcm_cap && !pcm_out))
        return FLACGPU_ERR_INVALID_INPUT;
    *n_samples = 0;
    if (n_frames == 0) return FLACGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    DecScratch *d = c->dec.get();
    hipStream_t st = c->stream.get();
    std::vector<uint64_t> foff;
    uint64_t src = 0, written = 0;
    for (uint64_t f0 = 0; f0 < n_frames; f0 += c->max_frames) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(c->max_frames, n_frames - f0);
        foff.assign(n, 0);
        uint64_t bytes = 0;
        for (uint32_t i = 0; i < n; i++) {
            foff[i] = bytes;
            bytes += frame_bytes[f0 + i];
        }
        HIPCHK(d->d_frames.grow(bytes + 16u));  // the chunk before this one was waited for
        HIPCHK(hipMemcpyAsync(d->d_frames.get(), frames + src, bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d->d_foff, foff.data(), (uint64_t)n * 8u, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d->d_fbytes, frame_bytes + f0, (uint64_t)n * 4u, hipMemcpyHostToDevice, st));
        rc = decode_chunk(c, d->d_frames.get(), d->d_foff, d->d_fbytes, n, pcm_out, pcm_cap, &written, n_samples,
                          (dec::Result *)results + f0, [] {});
        if (rc) return rc;
        src += bytes;
    }
    return FLACGPU_OK;
}

}  // extern "C"

// The frames are uploaded once and indexed on the device, and every chunk's table is a slice of
// that index; a chunk's PCM, once in pcm_out, is hashed while the next chunk decodes.  Returns 1
// where the device index does not give a frame table (it refuses the stream, or its scratch cannot
// be had): the caller then takes the host path, which names the error.
int fg::decode_stream_resident(flacgpu_ctx *c, const uint8_t *p, size_t len, uint32_t stream_bits, uint32_t stream_rate,
                               uint8_t *pcm_out, size_t pcm_cap, uint64_t *n_samples, uint8_t digest[16]) {
    if (len == 0 || len > 0xFFFFFFFFull) return 1;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    DecScratch *d = c->dec.get();
    hipStream_t st = c->stream.get();
    IdxScratch *x = idx_scratch(c);
    if (!x) return 1;
    const uint64_t fcap = table_cap_for(len);
    uint64_t *f_off = nullptr;
    uint32_t *f_bytes = nullptr;
    idx::IndexResult *d_res = nullptr;
    auto table = [&](uint8_t *base) {
        Carve v{base};
        v.take(fcap, f_off, f_bytes);
        return v.take(1, d_res);
    };
    if (fit(x->table, table, &st) != hipSuccess) return 1;
    if (d->d_frames.grow(len + 16u, &st) != hipSuccess) return 1;
    HIPCHK(hipMemcpyAsync(d->d_frames.get(), p, len, hipMemcpyHostToDevice, st));
    rc = index_core(c, d->d_frames.get(), len, stream_bits, stream_rate, f_off, f_bytes, fcap, d_res, st);
    if (rc == FLACGPU_ERR_OUT_OF_MEMORY) return 1;
    if (rc) return rc;
    idx::IndexResult ir{};
    HIPCHK(hipMemcpyAsync(&ir, d_res, sizeof(ir), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ir.status != idx::IDX_OK || ir.n_frames > fcap) return 1;
    const uint64_t n_frames = ir.n_frames;
    std::vector<dec::Result> res(c->max_frames);
    HostMd5 md5;
    uint64_t written = 0, hashed = 0;
    bool damaged = false;
    auto hash = [&] {
        md5.update(pcm_out + hashed, (size_t)(written - hashed));
        hashed = written;
    };
    for (uint64_t f0 = 0; f0 < n_frames; f0 += c->max_frames) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(c->max_frames, n_frames - f0);
        rc = decode_chunk(c, d->d_frames.get(), f_off + f0, f_bytes + f0, n, pcm_out, pcm_cap, &written, n_samples, res.data(),
                          hash);
        if (rc) return rc;
        for (uint32_t i = 0; i < n; i++)
            if (res[i].status) damaged = true;
    }
    if (damaged) return FLACGPU_ERR_INVALID_INPUT;  // a damaged frame: not a decodable file
    hash();
    md5.final(digest);
    return FLACGPU_OK;
}

// The device side of flacgpu_decode_files.  All files' frames go into one device buffer, each at a
// 64-byte aligned offset, and are indexed in one call; the PCM regions are then sized from every
// file's frame count and capacity, and all frames decode in chunks that run on from one file into
// the next.  The MD5 engine is flacgpu_md5_engine_for's choice for the batch: the device kernel over
// the decoded regions, or the host pool over the downloaded PCM.  take_single[i] = 1: the file is
// not clean here (the index refuses it, a frame is damaged or passes the capacity): the caller
// puts it through the single-file path, which names the error.
int fg::decode_files_resident(flacgpu_ctx *c, uint32_t n, const uint8_t *const *p, const size_t *len, const uint32_t *bits,
                              const uint32_t *rates, uint8_t *const *pcm_out, const size_t *pcm_cap, uint64_t *n_samples,
                              uint8_t *digests, uint8_t *take_single) {
    if (n == 0) return FLACGPU_OK;
    if (n > idx::kIdxMaxStreams) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    DecScratch *d = c->dec.get();
    hipStream_t st = c->stream.get();
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    const uint64_t per = (uint64_t)c->fmt.channels * c->fmt.bytes_per_sample;
    std::vector<uint64_t> offs, lens, pcm_offs, pcm_caps;
    std::vector<idx::IndexResult> ires;
    std::vector<streams::StreamResult> res;
    StreamTables tb;
    try {
        pcm_offs.resize(n);
        pcm_caps.resize(n);
        res.resize(n);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    rc = upload_files(c, n, p, len, offs, lens, st);
    if (rc) return rc;
    rc = streams_index(c, d->d_frames.get(), n, offs.data(), lens.data(), bits, rates, tb, ires, st);
    if (rc) return rc;
    // the regions: what the file's frames can hold at most, cut to the caller's capacity
    uint64_t pcm_total = 0, longest = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool ok = ires[i].status == idx::IDX_OK && ires[i].n_frames <= tb.caps[i];
        const uint64_t most = ok ? ires[i].n_frames * (uint64_t)c->fmt.max_block * per : 0u;
        pcm_offs[i] = pcm_total;
        pcm_caps[i] = std::min<uint64_t>(most, pcm_cap[i]);
        pcm_total += (pcm_caps[i] + 63u) & ~(uint64_t)63u;
        longest = std::max(longest, pcm_caps[i]);
    }
    const bool device_md5 = flacgpu_md5_engine_for(n, longest, pcm_total) == FLACGPU_MD5_DEVICE;
    HIPCHK(d->d_pcm.grow(pcm_total + 16u, &st));
    streams::StreamResult *d_res = nullptr;
    uint8_t *d_dig = nullptr;
    auto carve = [&](uint8_t *base) {
        Carve v{base};
        v.take(n, d_res);
        return v.take(16u * (uint64_t)n, d_dig);
    };
    HIPCHK(fit(x->files, carve, &st));
    rc = streams_decode(c, d->d_frames.get(), n, tb, ires, d->d_pcm.get(), pcm_offs.data(), pcm_caps.data(), d_res,
                        device_md5 ? d_dig : nullptr, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(res.data(), d_res, (uint64_t)n * sizeof(streams::StreamResult), hipMemcpyDeviceToHost, st));
    if (device_md5) HIPCHK(hipMemcpyAsync(digests, d_dig, 16u * (uint64_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<const void *> hp;
    std::vector<uint64_t> hl;
    std::vector<uint32_t> hi;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t bytes = res[i].n_samples * per;
        const bool clean = res[i].index_status == idx::IDX_OK && res[i].bad_frames == 0 && bytes <= pcm_caps[i];
        take_single[i] = clean ? 0 : 1;
        if (!clean) continue;
        n_samples[i] = res[i].n_samples;
        if (bytes) HIPCHK(hipMemcpyAsync(pcm_out[i], d->d_pcm.get() + pcm_offs[i], bytes, hipMemcpyDeviceToHost, st));
        if (!device_md5) {
            hp.push_back(pcm_out[i]);
            hl.push_back(bytes);
            hi.push_back(i);
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (!device_md5 && !hi.empty()) {
        std::vector<uint8_t> dg(16u * hi.size());
        rc = flacgpu_md5_many((uint32_t)hi.size(), hp.data(), hl.data(), nullptr, nullptr, dg.data());
        if (rc) return rc;
        for (size_t k = 0; k < hi.size(); k++) std::copy(dg.begin() + 16 * k, dg.begin() + 16 * (k + 1), digests + 16u * hi[k]);
    }
    return FLACGPU_OK;
}

// The device side of flacgpu_decode_files_windows.  The files' frames go into one device buffer as
// in decode_files_resident and are indexed in one call; the positions and the windows run on those
// tables, the delivered bytes land back to back in device memory, and only they and the windows'
// results come back.  status[w]: 0, FLACGPU_ERR_INVALID_INPUT (the device index refuses the file,
// or a covering frame is damaged) or FLACGPU_ERR_OUTPUT_TOO_SMALL.
int fg::decode_files_windows_resident(flacgpu_ctx *c, uint32_t n, const uint8_t *const *p, const size_t *len,
                                      const uint32_t *bits, const uint32_t *rates, uint32_t n_windows,
                                      const uint32_t *window_file, const uint64_t *window_start, const uint64_t *window_count,
                                      uint8_t *const *pcm_out, const uint64_t *pcm_cap, uint64_t *n_samples, int *status) {
    if (n_windows == 0) return FLACGPU_OK;
    if (n == 0 || n > idx::kIdxMaxStreams || n_windows > 65535u) return FLACGPU_ERR_INVALID_INPUT;
    HIPCHK(hipSetDevice(c->device));
    int rc = dec_scratch(c);
    if (rc) return rc;
    DecScratch *d = c->dec.get();
    hipStream_t st = c->stream.get();
    IdxScratch *x = idx_scratch(c);
    if (!x) return FLACGPU_ERR_OUT_OF_MEMORY;
    const uint64_t per = (uint64_t)c->fmt.channels * c->fmt.bytes_per_sample;
    std::vector<uint64_t> offs, lens, first, caps, out_offs;
    std::vector<window::WindowResult> res;
    try {
        first.resize(n);
        caps.resize(n);
        out_offs.resize(n_windows);
        res.resize(n_windows);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    rc = upload_files(c, n, p, len, offs, lens, st);
    if (rc) return rc;
    uint64_t entries = 0;
    for (uint32_t i = 0; i < n; i++) {
        first[i] = entries;
        caps[i] = table_cap_for(len[i]);
        entries += caps[i];
    }
    uint64_t *f_off = nullptr, *f_pos = nullptr, *d_totals = nullptr;
    uint32_t *f_bytes = nullptr;
    idx::IndexResult *d_ires = nullptr;
    auto table = [&](uint8_t *base) {
        Carve v{base};
        v.take(entries, f_off, f_pos);
        v.take(n, d_totals, d_ires);
        return v.take(entries, f_bytes);
    };
    HIPCHK(fit(x->table, table, &st));
    rc = index_streams_core(c, d->d_frames.get(), n, offs.data(), lens.data(), bits, rates, first.data(), caps.data(), f_off, f_bytes,
                            d_ires, st);
    if (rc) return rc;
    rc = positions_core(c, d->d_frames.get(), n, first.data(), caps.data(), f_off, f_bytes, d_ires, bits, rates, f_pos, d_totals, st);
    if (rc) return rc;
    const deliver::Delivery bytes = deliver::identity_delivery(deliver::SAMPLE_BYTES, 0u, c->fmt.channels, c->fmt.bytes_per_sample);
    WindowsCall wc;
    rc = windows_cover(c, first.data(), d_ires, f_pos, d_totals, n_windows, window_file, window_start, window_count, pcm_cap,
                       bytes, wc, st);
    if (rc) return rc;
    uint64_t out_total = 0;
    for (uint32_t w = 0; w < n_windows; w++) {
        const window::Cover &r = wc.recs[w];
        out_offs[w] = out_total;
        if (r.status != window::WIN_OK) continue;
        if (r.n_samples > r.span) return FLACGPU_ERR_INTERNAL;
        out_total += (r.n_samples * per + 15u) & ~(uint64_t)15u;
    }
    uint8_t *d_out = nullptr;
    window::WindowResult *d_wres = nullptr;
    auto carve = [&](uint8_t *base) {
        Carve v{base};
        v.take(n_windows, d_wres);
        return v.take(out_total + 16u, d_out);
    };
    HIPCHK(fit(x->win_out, carve, &st));
    rc = windows_decode(c, d->d_frames.get(), first.data(), f_off, f_bytes, wc, window_file, window_count, bytes, d_out,
                        out_offs.data(), d_wres, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(res.data(), d_wres, (uint64_t)n_windows * sizeof(window::WindowResult), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t w = 0; w < n_windows; w++) {
        n_samples[w] = 0;
        if (res[w].status == window::WIN_TOO_SMALL) status[w] = FLACGPU_ERR_OUTPUT_TOO_SMALL;
        else if (res[w].status != window::WIN_OK) status[w] = FLACGPU_ERR_INVALID_INPUT;
        else {
            status[w] = FLACGPU_OK;
            n_samples[w] = res[w].n_samples;
            const uint64_t bytes = res[w].n_samples * per;
            if (bytes) HIPCHK(hipMemcpyAsync(pcm_out[w], d_out + out_offs[w], bytes, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    return FLACGPU_OK;
}
