// fg_dec_api.cpp -- the host-only side of the decoder's C ABI: the frame index of a FLAC file or
// of a bare run of frames (no GPU), and the whole-file decode: metadata here, the frames through
// the device index and decode (fg_dec_host.cpp decode_stream_resident), or, where the device index
// refuses them, through the host index and flacgpu_decode_frames; flacgpu_decode_files does the
// same for many files through one batch (fg_dec_host.cpp decode_files_resident).  Plain C++ over
// include/flacgpu.h and the shared decode core.  And the host statement of the resampling rule
// (fg_resample.hpp): the coefficient table of a ratio and the sample rule over F32 elements; and of
// the feature rule (fg_features.hpp): the STFT table and the rule over one channel of F32 elements;
// and of the filter rule (fg_fir.hpp) over one channel of F32 elements.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/flacgpu.h"
#include "fg_dec.hpp"
#include "fg_deliver.hpp"
#include "fg_features.hpp"
#include "fg_fir.hpp"
#include "fg_index.hpp"
#include "fg_internal.hpp"
#include "fg_levels.hpp"
#include "fg_md5_host.hpp"
#include "fg_resample.hpp"

using namespace fg;

namespace {

uint64_t rd_be(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[i];
    return v;
}

using idx::header_at;  // the device index (fg_index.hip) tests its candidates with the same function

// Frame sizes of the frames in [p, p + len): a frame ends where the next position with a sync
// code and a CRC-8-clean header follows a good CRC-16 over everything since the frame's start.
int index_frames(const uint8_t *p, size_t len, uint32_t stream_bits, uint32_t stream_rate, std::vector<uint32_t> &sizes) {
    size_t s = 0;
    while (s < len) {
        uint32_t hdr = 0;
        if (!header_at(p + s, len - s, stream_bits, stream_rate, &hdr)) return FLACGPU_ERR_INVALID_INPUT;
        // crc = CRC-16 of [s, upto); a candidate end e needs it over [s, e - 2)
        uint32_t crc = 0;
        size_t upto = s, e = s + hdr + 3u;  // at least one subframe byte and the CRC-16
        bool found = false;
        for (; e <= len; e++) {
            while (upto < e - 2u) crc = crc_byte_v(crc, p[upto++]);
            if (crc != (((uint32_t)p[e - 2] << 8) | p[e - 1])) continue;
            uint32_t nh = 0;
            if (e == len || header_at(p + e, len - e, stream_bits, stream_rate, &nh)) {
                found = true;
                break;
            }
        }
        if (!found || e - s > 0xFFFFFFFFull) return FLACGPU_ERR_INVALID_INPUT;
        sizes.push_back((uint32_t)(e - s));
        s = e;
    }
    return FLACGPU_OK;
}

// "fLaC" and the metadata blocks (RFC 9639 8): STREAMINFO (8.2) to *si, the others skipped by length
int parse_metadata(const uint8_t *p, size_t len, flacgpu_streaminfo *si, size_t *first) {
    if (len < 4 || std::memcmp(p, "fLaC", 4) != 0) return FLACGPU_ERR_INVALID_INPUT;
    size_t pos = 4;
    bool have_si = false;
    for (;;) {
        if (pos + 4 > len) return FLACGPU_ERR_INVALID_INPUT;
        const bool last = (p[pos] & 0x80) != 0;
        const uint32_t type = p[pos] & 0x7F;
        const size_t n = (size_t)rd_be(p + pos + 1, 3);
        pos += 4;
        if (n > len - pos) return FLACGPU_ERR_INVALID_INPUT;
        if (type == 0) {
            if (n != 34) return FLACGPU_ERR_INVALID_INPUT;
            const uint8_t *q = p + pos;
            std::memset(si, 0, sizeof(*si));
            si->min_block_size = (uint16_t)rd_be(q, 2);
            si->max_block_size = (uint16_t)rd_be(q + 2, 2);
            si->min_frame_size = (uint32_t)rd_be(q + 4, 3);
            si->max_frame_size = (uint32_t)rd_be(q + 7, 3);
            const uint64_t v = rd_be(q + 10, 8);  // rate 20, channels-1 3, bits-1 5, samples 36
            si->sample_rate = (uint32_t)(v >> 44);
            si->channels = (uint8_t)(((v >> 41) & 7u) + 1u);
            si->bit_depth = (uint8_t)(((v >> 36) & 31u) + 1u);
            si->interchannel_samples = v & ((1ull << 36) - 1u);
            std::memcpy(si->md5, q + 18, 16);
            have_si = true;
        }
        pos += n;
        if (last) break;
    }
    if (!have_si) return FLACGPU_ERR_INVALID_INPUT;
    *first = pos;
    return FLACGPU_OK;
}

}  // namespace

extern "C" {

int flacgpu_flac_index(const void *flac, size_t len, flacgpu_streaminfo *streaminfo, size_t *first_frame_offset,
                       uint32_t *frame_bytes, size_t cap, size_t *n_frames) {
    if (!flac || !n_frames || (cap && !frame_bytes)) return FLACGPU_ERR_INVALID_INPUT;
    const uint8_t *p = (const uint8_t *)flac;
    *n_frames = 0;
    size_t first = 0;
    uint32_t bits = 16, rate = 0;
    if (streaminfo) {  // a file; NULL: a bare run of frames
        const int rc = parse_metadata(p, len, streaminfo, &first);
        if (rc) return rc;
        bits = streaminfo->bit_depth;
        rate = streaminfo->sample_rate;
    }
    if (first_frame_offset) *first_frame_offset = first;
    std::vector<uint32_t> sizes;
    const int rc = index_frames(p + first, len - first, bits, rate, sizes);
    if (rc) return rc;
    *n_frames = sizes.size();
    if (sizes.size() > cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
    if (!sizes.empty()) std::memcpy(frame_bytes, sizes.data(), sizes.size() * sizeof(uint32_t));
    return FLACGPU_OK;
}

int flacgpu_decode_file(flacgpu_ctx *ctx, const void *flac, size_t len, uint8_t *pcm_out, size_t pcm_cap,
                        uint64_t *n_samples, int *md5_ok) {
    if (!ctx || !flac || !n_samples || (pcm_cap && !pcm_out)) return FLACGPU_ERR_INVALID_INPUT;
    *n_samples = 0;
    if (md5_ok) *md5_ok = 0;
    const uint8_t *p = (const uint8_t *)flac;
    flacgpu_streaminfo si;
    size_t first = 0;
    int rc = parse_metadata(p, len, &si, &first);
    if (rc) return rc;
    flacgpu_config cfg;
    rc = flacgpu_get_config(ctx, &cfg);
    if (rc) return rc;
    if (si.channels != cfg.channels || si.bit_depth != cfg.bits_per_sample) return FLACGPU_ERR_INVALID_INPUT;
    uint8_t digest[16];
    rc = decode_stream_resident(ctx, p + first, len - first, si.bit_depth, si.sample_rate, pcm_out, pcm_cap, n_samples, digest);
    if (rc == 1) {
        // the device index gave no frame table: the host index and the host-buffer decode, which
        // refuse what they always refused
        *n_samples = 0;
        std::vector<uint32_t> sizes;
        rc = index_frames(p + first, len - first, si.bit_depth, si.sample_rate, sizes);
        if (rc) return rc;
        std::vector<flacgpu_decode_result> res(sizes.size() ? sizes.size() : 1);
        rc = flacgpu_decode_frames(ctx, p + first, sizes.data(), sizes.size(), pcm_out, pcm_cap, n_samples, res.data());
        if (rc) return rc;
        for (size_t i = 0; i < sizes.size(); i++)
            if (res[i].status) return FLACGPU_ERR_INVALID_INPUT;  // a damaged frame: not a decodable file
        HostMd5 h;
        h.update(pcm_out, (size_t)(*n_samples * cfg.channels * (cfg.bits_per_sample / 8u)));
        h.final(digest);
    } else if (rc) {
        return rc;
    }
    if (md5_ok)
        *md5_ok = std::memcmp(digest, si.md5, 16) == 0 &&
                  (si.interchannel_samples == 0 || si.interchannel_samples == *n_samples);
    return FLACGPU_OK;
}

// The files whose metadata and stream parameters are good go through the device in one batch
// (fg_dec_host.cpp decode_files_resident); a file that is not clean there is decoded again by
// flacgpu_decode_file, so its status, sample count and bytes are the single-file ones.
int flacgpu_decode_files(flacgpu_ctx *ctx, uint32_t n_files, const void *const *flac, const size_t *len,
                         uint8_t *const *pcm_out, const size_t *pcm_cap, uint64_t *n_samples, int *md5_ok, int *status) {
    if (!ctx || (n_files && (!flac || !len || !pcm_out || !pcm_cap || !n_samples || !status)))
        return FLACGPU_ERR_INVALID_INPUT;
    if (n_files == 0) return FLACGPU_OK;
    flacgpu_config cfg;
    int rc = flacgpu_get_config(ctx, &cfg);
    if (rc) return rc;
    std::vector<flacgpu_streaminfo> si(n_files);
    std::vector<uint32_t> which, bits, rates;  // the batch: file index, STREAMINFO's depth and rate
    std::vector<const uint8_t *> ptr;
    std::vector<size_t> lens, caps;
    std::vector<uint8_t *> outs;
    for (uint32_t i = 0; i < n_files; i++) {
        n_samples[i] = 0;
        if (md5_ok) md5_ok[i] = 0;
        size_t first = 0;
        if (!flac[i] || (pcm_cap[i] && !pcm_out[i])) {
            status[i] = FLACGPU_ERR_INVALID_INPUT;
            continue;
        }
        const uint8_t *p = (const uint8_t *)flac[i];
        status[i] = parse_metadata(p, len[i], &si[i], &first);
        if (status[i]) continue;
        if (si[i].channels != cfg.channels || si[i].bit_depth != cfg.bits_per_sample) {
            status[i] = FLACGPU_ERR_INVALID_INPUT;
            continue;
        }
        which.push_back(i);
        bits.push_back(si[i].bit_depth);
        rates.push_back(si[i].sample_rate);
        ptr.push_back(p + first);
        lens.push_back(len[i] - first);
        outs.push_back(pcm_out[i]);
        caps.push_back(pcm_cap[i]);
    }
    const uint32_t nb = (uint32_t)which.size();
    std::vector<uint64_t> ns(nb, 0);
    std::vector<uint8_t> digests(16u * (size_t)nb + 1u), single(nb + 1u, 0);
    rc = decode_files_resident(ctx, nb, ptr.data(), lens.data(), bits.data(), rates.data(), outs.data(), caps.data(),
                               ns.data(), digests.data(), single.data());
    if (rc) return rc;
    for (uint32_t k = 0; k < nb; k++) {
        const uint32_t i = which[k];
        if (single[k]) {
            status[i] = flacgpu_decode_file(ctx, flac[i], len[i], pcm_out[i], pcm_cap[i], &n_samples[i],
                                            md5_ok ? &md5_ok[i] : nullptr);
            continue;
        }
        n_samples[i] = ns[k];
        if (md5_ok)
            md5_ok[i] = std::memcmp(&digests[16u * (size_t)k], si[i].md5, 16) == 0 &&
                        (si[i].interchannel_samples == 0 || si[i].interchannel_samples == ns[k]);
    }
    return FLACGPU_OK;
}

// The files whose metadata and stream parameters are good go through the device in one batch
// (fg_dec_host.cpp decode_files_windows_resident) with the windows that name them; a window of
// another file gets that file's status.
int flacgpu_decode_files_windows(flacgpu_ctx *ctx, uint32_t n_files, const void *const *flac, const size_t *len,
                                 uint32_t n_windows, const uint32_t *window_file, const uint64_t *window_start,
                                 const uint64_t *window_count, uint8_t *const *pcm_out, const size_t *pcm_cap,
                                 uint64_t *n_samples, int *status) {
    if (!ctx || n_windows > 65535u || (n_files && (!flac || !len)) ||
        (n_windows && (!window_file || !window_start || !window_count || !pcm_out || !pcm_cap || !n_samples || !status)))
        return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t w = 0; w < n_windows; w++)
        if (window_file[w] >= n_files || (pcm_cap[w] && !pcm_out[w])) return FLACGPU_ERR_INVALID_INPUT;
    if (n_windows == 0) return FLACGPU_OK;
    flacgpu_config cfg;
    int rc = flacgpu_get_config(ctx, &cfg);
    if (rc) return rc;
    constexpr uint32_t kUnused = 0xFFFFFFFFu;
    std::vector<int> file_status(n_files, FLACGPU_OK);
    std::vector<uint32_t> slot(n_files, kUnused), bits, rates;  // slot: the file's place in the batch
    std::vector<const uint8_t *> ptr;
    std::vector<size_t> lens;
    for (uint32_t i = 0; i < n_files; i++) {
        flacgpu_streaminfo si;
        size_t first = 0;
        if (!flac[i]) {
            file_status[i] = FLACGPU_ERR_INVALID_INPUT;
            continue;
        }
        const uint8_t *p = (const uint8_t *)flac[i];
        file_status[i] = parse_metadata(p, len[i], &si, &first);
        if (file_status[i]) continue;
        if (si.channels != cfg.channels || si.bit_depth != cfg.bits_per_sample) {
            file_status[i] = FLACGPU_ERR_INVALID_INPUT;
            continue;
        }
        slot[i] = (uint32_t)ptr.size();
        bits.push_back(si.bit_depth);
        rates.push_back(si.sample_rate);
        ptr.push_back(p + first);
        lens.push_back(len[i] - first);
    }
    std::vector<uint32_t> which, w_slot;  // the batch's windows: window index, its file's slot
    std::vector<uint64_t> w_start, w_count, w_cap;
    std::vector<uint8_t *> w_out;
    for (uint32_t w = 0; w < n_windows; w++) {
        n_samples[w] = 0;
        status[w] = file_status[window_file[w]];
        if (status[w]) continue;
        which.push_back(w);
        w_slot.push_back(slot[window_file[w]]);
        w_start.push_back(window_start[w]);
        w_count.push_back(window_count[w]);
        w_cap.push_back(pcm_cap[w]);
        w_out.push_back(pcm_out[w]);
    }
    const uint32_t nw = (uint32_t)which.size();
    if (nw == 0) return FLACGPU_OK;
    std::vector<uint64_t> ns(nw, 0);
    std::vector<int> st(nw, 0);
    rc = decode_files_windows_resident(ctx, (uint32_t)ptr.size(), ptr.data(), lens.data(), bits.data(), rates.data(), nw,
                                       w_slot.data(), w_start.data(), w_count.data(), w_out.data(), w_cap.data(), ns.data(),
                                       st.data());
    if (rc) return rc;
    for (uint32_t k = 0; k < nw; k++) {
        n_samples[which[k]] = ns[k];
        status[which[k]] = st[k];
    }
    return FLACGPU_OK;
}

int flacgpu_resample_filter(uint32_t src_rate, uint32_t dst_rate, uint32_t *up, uint32_t *down, uint32_t *taps, float *coeffs,
                            size_t cap, size_t *n) {
    resample::Ratio r;
    if (!n || (cap && !coeffs) || !resample::valid_ratio(src_rate, dst_rate, &r)) return FLACGPU_ERR_INVALID_INPUT;
    if (up) *up = r.L;
    if (down) *down = r.M;
    if (taps) *taps = r.T;
    *n = (size_t)r.L * r.T;
    if (*n > cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
    double row64[resample::kMaxTaps];
    for (uint32_t p = 0; p < r.L; p++) resample::filter_row(r, p, row64, coeffs + (size_t)p * r.T);
    return FLACGPU_OK;
}

int flacgpu_resample_f32_host(const float *x, uint64_t total, uint32_t src_rate, uint32_t dst_rate, uint64_t start,
                              uint64_t count, float *y, uint64_t *n) {
    resample::Ratio r;
    if (!n || (total && !x) || total > (1ull << 40) || !resample::valid_ratio(src_rate, dst_rate, &r))
        return FLACGPU_ERR_INVALID_INPUT;
    *n = 0;
    const uint64_t got = resample::delivered(resample::out_total(r, total), start, count);
    if (got == 0) return FLACGPU_OK;
    if (!y) return FLACGPU_ERR_INVALID_INPUT;
    std::vector<float> h;
    try {
        h.resize((size_t)r.L * r.T);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    double row64[resample::kMaxTaps];
    for (uint32_t p = 0; p < r.L; p++) resample::filter_row(r, p, row64, h.data() + (size_t)p * r.T);
    for (uint64_t t = 0; t < got; t++) {
        uint32_t p;
        const int64_t first = (int64_t)resample::source_index(r, start + t, &p) - (int64_t)r.Hw + 1;
        y[t] = resample::fir(h.data() + (size_t)p * r.T, r.T, [&](uint32_t k) {
            const int64_t i = first + (int64_t)k;
            return i >= 0 && (uint64_t)i < total ? x[i] : 0.0f;
        });
    }
    *n = got;
    return FLACGPU_OK;
}

int flacgpu_mix_weights_valid(uint32_t channels, uint32_t out_channels, const float *weights, uint32_t sample_format) {
    return deliver::mixw_valid(channels, out_channels, weights, sample_format) ? 1 : 0;
}

int flacgpu_mix_weights_f32_host(const int32_t *samples, uint64_t n, uint32_t channels, uint32_t bits, uint32_t out_channels,
                                 const float *weights, float *y) {
    if ((bits != 8u && bits != 16u && bits != 24u && bits != 32u) || n > (1ull << 40) ||
        !deliver::mixw_valid(channels, out_channels, weights, deliver::SAMPLE_F32))
        return FLACGPU_ERR_INVALID_INPUT;
    if (n == 0) return FLACGPU_OK;
    if (!samples || !y) return FLACGPU_ERR_INVALID_INPUT;
    const int64_t lo = -((int64_t)1 << (bits - 1u)), hi = ((int64_t)1 << (bits - 1u)) - 1;
    for (uint64_t i = 0; i < n * channels; i++)
        if (samples[i] < lo || samples[i] > hi) return FLACGPU_ERR_INVALID_INPUT;  // not a sample of `bits` bits
    for (uint64_t t = 0; t < n; t++)
        for (uint32_t k = 0; k < out_channels; k++) {
            float acc = 0.0f;
            for (uint32_t c = 0; c < channels; c++)
                acc = deliver::mixw_step(acc, weights[(size_t)k * channels + c], samples[t * channels + c], bits);
            y[t * out_channels + k] = acc;
        }
    return FLACGPU_OK;
}

int flacgpu_levels_host(const int32_t *samples, uint64_t n, uint32_t channels, uint32_t hop, uint32_t *peak, int64_t *sum,
                        double *energy) {
    if (hop == 0u || hop > levels::kMaxHop || channels == 0u || n > (1ull << 40)) return FLACGPU_ERR_INVALID_INPUT;
    if (n == 0) return FLACGPU_OK;
    if (!samples || !peak || !sum || !energy) return FLACGPU_ERR_INVALID_INPUT;
    const uint64_t nb = levels::n_blocks(n, hop);
    for (uint64_t j = 0; j < nb; j++) {
        const uint64_t t0 = j * hop, len = levels::block_len(n, hop, j);
        for (uint32_t c = 0; c < channels; c++) {
            levels::Acc a = levels::acc_zero();
            for (uint64_t t = t0; t < t0 + len; t++) levels::acc_add(a, samples[t * channels + c]);
            peak[j * channels + c] = a.peak;
            sum[j * channels + c] = a.sum;
            energy[j * channels + c] = levels::acc_energy(a);
        }
    }
    return FLACGPU_OK;
}

int flacgpu_fir_f32_host(const float *x, uint64_t total, const float *taps, uint32_t n_taps, uint32_t delay, uint64_t start,
                         uint64_t count, float *y, uint64_t *n) {
    if (!n || (total && !x) || total > (1ull << 40) || !taps) return FLACGPU_ERR_INVALID_INPUT;
    const fir::Filter f{0u, n_taps, delay, 1u, 0u};
    if (!fir::filter_valid(f, 1u, n_taps) || !fir::span_valid(count, n_taps)) return FLACGPU_ERR_INVALID_INPUT;
    for (uint32_t k = 0; k < n_taps; k++)
        if (!std::isfinite(taps[k])) return FLACGPU_ERR_INVALID_INPUT;
    *n = resample::delivered(total, start, count);
    if (count == 0) return FLACGPU_OK;
    if (!y) return FLACGPU_ERR_INVALID_INPUT;
    // *n > 0 only where start < total <= 2^40: no index below passes 2^42
    for (uint64_t t = 0; t < *n; t++)
        y[t] = fir::element(taps, n_taps, delay, start, t, [&](int64_t i) { return i >= 0 && (uint64_t)i < total ? x[i] : 0.0f; });
    for (uint64_t t = *n; t < count; t++) y[t] = 0.0f;
    return FLACGPU_OK;
}

int flacgpu_features_table(uint32_t n_fft, float *table, size_t cap, size_t *n) {
    const feat::Params p{n_fft, 1u, 0u};
    if (!n || (cap && !table) || !feat::valid(p)) return FLACGPU_ERR_INVALID_INPUT;
    const uint32_t N = n_fft, B = feat::bins(p);
    *n = (size_t)2u * B * N;
    if (*n > cap) return FLACGPU_ERR_OUTPUT_TOO_SMALL;
    // feat::table_entry with the N window values and the N angles' cosines and sines computed once
    double w[feat::kMaxFft], cv[feat::kMaxFft], sv[feat::kMaxFft];
    for (uint32_t m = 0; m < N; m++) {
        const double a = feat::kTwoPi * (double)m / (double)N;
        w[m] = feat::hann(N, m);
        cv[m] = cos(a);
        sv[m] = sin(a);
    }
    for (uint32_t b = 0; b < B; b++)
        for (uint32_t k = 0; k < N; k++) {
            const uint32_t m = (uint32_t)(((uint64_t)b * k) % N);
            table[(size_t)b * N + k] = (float)(w[k] * cv[m]);
            table[((size_t)B + b) * N + k] = (float)(-w[k] * sv[m]);
        }
    return FLACGPU_OK;
}

int flacgpu_features_f32_host(const float *x, uint64_t total, const flacgpu_features *ft, const float *filters, uint64_t start,
                              uint64_t frames, float *y, uint64_t *n) {
    if (!n || !ft || (total && !x) || total > (1ull << 40)) return FLACGPU_ERR_INVALID_INPUT;
    const feat::Params p{ft->n_fft, ft->hop, ft->n_rows};
    if (!feat::valid(p) || (p.n_rows && !filters)) return FLACGPU_ERR_INVALID_INPUT;
    const uint32_t N = p.n_fft, B = feat::bins(p), R = feat::rows(p);
    for (size_t i = 0; i < (size_t)p.n_rows * B; i++)
        if (!std::isfinite(filters[i])) return FLACGPU_ERR_INVALID_INPUT;
    if (frames && frames - 1u > (0x7FFFFFFFull - N) / p.hop) return FLACGPU_ERR_INVALID_INPUT;
    *n = feat::delivered(p, total, start, frames);
    if (frames == 0) return FLACGPU_OK;
    if (!y) return FLACGPU_ERR_INVALID_INPUT;
    std::vector<float> table, xf(N), P(B);
    size_t tn = 0;
    try {
        table.resize((size_t)2u * B * N);
    } catch (...) {
        return FLACGPU_ERR_OUT_OF_MEMORY;
    }
    const int rc = flacgpu_features_table(N, table.data(), table.size(), &tn);
    if (rc) return rc;
    for (uint64_t t = 0; t < frames; t++) {
        // sample i of the frame is x[first + i]; a start past 2^41 >= 2 * total + span is wholly outside
        const bool far = start > (1ull << 41);
        const int64_t first = far ? 0 : (int64_t)(start + t * p.hop) - (int64_t)(N / 2u);
        bool any = false;
        for (uint32_t i = 0; i < N; i++) {
            const int64_t at = first + (int64_t)i;
            const bool in = !far && at >= 0 && (uint64_t)at < total;
            xf[i] = in ? x[at] : 0.0f;
            any = any || in;
        }
        for (uint32_t b = 0; b < B && any; b++) P[b] = feat::bin_power(table.data(), N, b, [&](uint32_t i) { return xf[i]; });
        for (uint32_t r = 0; r < R; r++) {
            float v = 0.0f;  // a frame wholly outside the stream: every chain stays at +0.0f
            if (any) v = p.n_rows ? feat::filter_row_skip(filters + (size_t)r * B, P.data(), B) : P[r];
            y[(size_t)r * frames + t] = v;
        }
    }
    return FLACGPU_OK;
}

}  // extern "C"
