// fg_geom.hpp -- which kernels a context launches, with how many threads and how much LDS: a pure
// function of the configuration and the output-invariant knobs.  flacgpu_open (fg_api.cpp) calls
// enc_geometry once and keeps the result; the stand-alone host program of the tests
// (tests/cpp/geom_host_main.cpp, tests/test_geom_host.py) pins it row by row against
// tests/golden/geometry.json.  dec_geometry is the same for the decoder's reconstruct kernel
// (launch_dec_recon calls it; tests/cpp/decgeom_host_main.cpp, tests/golden/dec_geometry.json).  No HIP, no environment, no state: compiles under hipcc and plain g++
// (a host-only includer defines __host__ / __device__ away before including, for fg_layout.hpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/flacgpu.h"
#include "fg_common.hpp"
#include "fg_layout.hpp"

// chunk sets of the pipelined host-buffer path (encode_pipelined): chunk i uploads into set i % 3
// while chunk i-1 encodes and chunks i-2, i-3 download -- with two sets the upload of chunk i had
// to wait for the encode of chunk i-2 and the encode for the download of chunk i-2, so a slow
// download or a late host thread stalled both directions of PCIe (round-4 batches reached 33-44 GB/s
// of H2D against 57 GB/s measured alone)
constexpr uint32_t kPipeSets = 4;  // the most; fg::Knobs::pipe_sets is the number in use (2..4)
constexpr uint32_t kPipeSetsDefault = 3;

namespace fg {

// The output-invariant tuning knobs (schedule / kernel-variant choices; every setting is
// parity-tested: tests/test_gpu_parity.py, test_gpu_plan.py; INTEGRATION.md lists them), as the
// environment gave them when the context was opened.  A tri-state is -1 where the variable is not
// set (or says neither): enc_geometry then keeps its own choice.
struct Knobs {
    // ---- these change the geometry ----
    int pack_dbuf = -1;   // FLACGPU_PACK_DBUF: 1 = "1", 0 = anything else: single-buffered pack staging
    int pack4 = -1;       // FLACGPU_PACK4: 0 = "0" (k_pack for full 16-bit stereo frames), 1 = anything else
    int packw = -1;       // FLACGPU_PACKW: 1 / 0 = k_packw forced on / off
    bool packw_wps2 = false;  // FLACGPU_PACKW_WPS=2: two waves per written subframe
    int packw_dbuf = -1;  // FLACGPU_PACKW_DBUF: as pack_dbuf, for k_packw's staging
    int pack_split = -1;  // FLACGPU_PACK_SPLIT: 0 = "0" (no channel-half pack), 1 = anything else
    bool md5_kernel_set = false;  // FLACGPU_MD5_KERNEL: batched stream MD5, 1 = coalesced LDS-DMA ring,
    int md5_kernel = 0;           // 0 = per-lane loads, 2 = three-chunk ring
    int ana1 = -1;        // FG_DIAG, FLACGPU_ANA1: 0 = k_analyze, 1 / 2 = k_ana1 variant
    bool fused = false;   // FG_DIAG, FLACGPU_FUSED=1
    // ---- these change only the schedule ----
    bool xcd_queue = true;  // split analysis: per-XCD item queues (fg_device.hpp xcd_ticket)
    bool pack_xcdq = true;  // split pack: the same (fg_packw.hpp)
    // split analysis (bit 0) / pack (bit 1): each item's ticket taken right before its DMA, so a
    // frame's two halves are staged close together (c4 A/B r4l: analysis 5.03 -> 4.95 ms, analysis
    // traffic 1.82x -> 1.44x of the PCM (r4n); the pack's bit measured no gain, r4o)
    uint32_t split_jit = 1;
    uint32_t pipe_sets = kPipeSetsDefault;  // chunk sets in use (FLACGPU_PIPE_SETS = 2: the round-4 schedule; 4)
    // issue priority of the stream-MD5 waves beside the encode: 1 trades 2-5 % of the encode for a
    // 35-58 % shorter MD5 chain -- for a workload whose MD5 would bind the step.
    // Bits 8 and up: FLACGPU_MD5_DIAG (FG_DIAG)
    int md5_prio = 0;
    // FG_DIAG only: grid reserves, the overlapped schedule's shape at open, spinning host waits
    uint32_t enc_prio = 0;  // issue priority 1 for the C2 encode waves (FLACGPU_ENC_PRIO)
    int md5_reserve = -1;   // 1: the analysis grid leaves one workgroup slot per stream-MD5 workgroup
                            //    queued beside it, 2: the pack grid too, 0: none, -1: auto
    uint32_t ovl_chunks = 0, ovl_ana = 2, ovl_pack = 2, ovl_min_frames = 4096;  // flacgpu_ctx's, at open
    bool spin_sync = false;  // FLACGPU_SPIN_SYNC=1: spinning events for the host waits
};

// The variables behind Knobs.  The diagnostic ones are not even named in a release library
// (tests/test_abi.py).
constexpr const char *kKnobNames[] = {
    "FLACGPU_PACK_DBUF", "FLACGPU_PACK4",     "FLACGPU_PACKW",      "FLACGPU_PACKW_WPS", "FLACGPU_PACKW_DBUF",
    "FLACGPU_PACK_SPLIT", "FLACGPU_MD5_KERNEL", "FLACGPU_XCD_QUEUE", "FLACGPU_PACK_XCDQ", "FLACGPU_SPLIT_JIT",
    "FLACGPU_PIPE_SETS",  "FLACGPU_MD5_PRIO",
#if FG_DIAG
    "FLACGPU_ANA1",       "FLACGPU_FUSED",     "FLACGPU_ENC_PRIO",   "FLACGPU_MD5_RESERVE", "FLACGPU_MD5_DIAG",
    "FLACGPU_OVERLAP",    "FLACGPU_OVL_ANA",   "FLACGPU_OVL_PACK",   "FLACGPU_OVL_MIN",   "FLACGPU_SPIN_SYNC",
#endif
};

// The text `e` of variable `name` into its knob; false where `name` is none of kKnobNames.
inline bool knob_set(Knobs &k, const char *name, const char *e) {
    auto is = [&](const char *n) { return strcmp(name, n) == 0; };
    if (is("FLACGPU_PACK_DBUF")) k.pack_dbuf = e[0] == '1';
    else if (is("FLACGPU_PACK4")) k.pack4 = e[0] != '0';
    else if (is("FLACGPU_PACKW")) k.packw = e[0] == '1' ? 1 : (e[0] == '0' ? 0 : -1);
    else if (is("FLACGPU_PACKW_WPS")) k.packw_wps2 = e[0] == '2';
    else if (is("FLACGPU_PACKW_DBUF")) k.packw_dbuf = e[0] == '1';
    else if (is("FLACGPU_PACK_SPLIT")) k.pack_split = e[0] != '0';
    else if (is("FLACGPU_MD5_KERNEL")) {
        k.md5_kernel_set = true;
        k.md5_kernel = atoi(e);
    } else if (is("FLACGPU_XCD_QUEUE")) k.xcd_queue = e[0] != '0';
    else if (is("FLACGPU_PACK_XCDQ")) k.pack_xcdq = e[0] != '0';
    else if (is("FLACGPU_SPLIT_JIT")) k.split_jit = (uint32_t)atoi(e) & 3u;
    else if (is("FLACGPU_PIPE_SETS")) {
        const int v = atoi(e);
        k.pipe_sets = v >= 2 && v <= (int)kPipeSets ? (uint32_t)v : kPipeSetsDefault;
    } else if (is("FLACGPU_MD5_PRIO")) k.md5_prio = (k.md5_prio & ~0xFF) | (atoi(e) ? 1 : 0);
#if FG_DIAG
    else if (is("FLACGPU_ANA1")) k.ana1 = e[0] == '0' ? 0 : (e[0] == '2' ? 2 : 1);
    else if (is("FLACGPU_FUSED")) k.fused = e[0] == '1';
    else if (is("FLACGPU_ENC_PRIO")) k.enc_prio = e[0] == '1' ? 1u : 0u;
    else if (is("FLACGPU_MD5_RESERVE")) k.md5_reserve = atoi(e);
    else if (is("FLACGPU_MD5_DIAG")) k.md5_prio |= atoi(e) << 8;
    else if (is("FLACGPU_OVERLAP")) k.ovl_chunks = (uint32_t)atoi(e);
    else if (is("FLACGPU_OVL_ANA")) k.ovl_ana = (uint32_t)atoi(e);
    else if (is("FLACGPU_OVL_PACK")) k.ovl_pack = (uint32_t)atoi(e);
    else if (is("FLACGPU_OVL_MIN")) k.ovl_min_frames = (uint32_t)(atoi(e) > 1 ? atoi(e) : 1);
    else if (is("FLACGPU_SPIN_SYNC")) k.spin_sync = e[0] == '1';
#endif
    else return false;
    return true;
}

// Everything flacgpu_open derives from the configuration and the knobs.
struct EncGeom {
    uint32_t C = 0, B = 0, bits = 0, stereo = 0;
    uint32_t image_bytes = 0, desc_stride = 0;
    // full-frame analysis (k_analyze; staging double-buffered where it fits) and the tail kernel's
    uint32_t nt = 0, lds = 0, lds_tail = 0;
    bool stage_dbuf = false;
    bool ana_split = false;  // full-frame analysis in channel halves (fg_device.hpp k_analyze)
    uint32_t nt_split = 0, lds_split = 0;
    // k_pack: tail frames, and the full frames that no other pack kernel takes
    uint32_t nt_pack = 0, lds_pack = 0, crc_hmax = 0;
    bool pack_dbuf = false;
    // full 16-bit two-channel frames are packed by k_pack4 (four waves per subframe): 512 threads;
    // 32-bit or 3+ channel frames by k_packw.  nt_pack4 == 0: neither
    uint32_t nt_pack4 = 0, lds_pack4 = 0, crc_hmax4 = 0;
    bool pack_split = false;  // full-frame pack in channel halves (fg_packw.hpp k_packw<..., true>)
    uint32_t nt_psplit = 0, lds_psplit = 0, image_split = 0, crc_hmaxs = 0;
    int md5_kernel = 1;  // batched stream MD5 (Knobs::md5_kernel, or the configuration's default)
    // FG_DIAG: one wave per full 16-bit stereo frame (fg_ana1.hpp k_ana1) instead of one per candidate
    bool ana1 = false;
    uint32_t ana1_variant = 1;
    // FG_DIAG: fused single-pass encode of full 16-bit stereo frames (fg_fused.hpp): analysis and
    // pack in one kernel of 256 threads, frame offsets by an in-kernel look-back over per-slot status words
    bool fused = false;
    uint32_t lds_fused = 0, crc_hmaxf = 0;
};

constexpr uint32_t kLdsLimit = 160u * 1024u;  // LDS of a gfx950 CU, and the most one workgroup may ask for

// CRC fold: half-segments of H words (odd), H <= ceil(image words / (2 * threads))
inline uint32_t crc_hmax_for(uint32_t image_bytes, uint32_t threads) {
    return ((image_bytes / 4u + 2u * threads - 1u) / (2u * threads)) | 1u;
}

// cfg has passed flacgpu_open's validation.  FLACGPU_ERR_INVALID_CONFIG: a kernel's LDS does not fit.
inline int enc_geometry(const flacgpu_config &cfg, const Knobs &k, EncGeom &g) {
    g = EncGeom();
    g.C = cfg.channels;
    g.bits = cfg.bits_per_sample;
    g.B = g.bits / 8;
    g.stereo = (g.C == 2 && cfg.stereo_decorrelation) ? 1u : 0u;
    const uint32_t nw = g.stereo ? 4u : g.C;
    const uint32_t n_out = g.stereo ? 2u : g.C;
    g.nt = 64u * nw;
    g.nt_pack = 64u * n_out;
    g.image_bytes = fg_round16(frame_bound_bytes(kBlock, g.C, g.bits, g.stereo != 0) + 16u);
    g.desc_stride = desc_stride(n_out);
    const bool lpc = cfg.prediction != 0;
    // 24-bit LPC analysis runs three waves per SIMD (fg_device.hpp): double-buffer only where
    // three workgroups still fit the LDS
    const uint32_t ana_wgs = (lpc && g.B == 3) ? (FG_C3_W == 3 ? 3u : 2u) : 1u;
    g.stage_dbuf = ana_layout(g.C, g.B, nw, true, true, lpc).total * ana_wgs <= kLdsLimit;
    g.lds = ana_layout(g.C, g.B, nw, true, g.stage_dbuf, lpc).total;
    g.lds_tail = ana_layout(g.C, g.B, nw, false, false, lpc).total;
    // Frames of 4+ independent channels too large to double-buffer: analyse them in channel
    // halves (one workgroup per half, staged single-buffered) when a half is whole dwords of
    // every interchannel row and two halves fit a CU -- c4: three 51-KiB workgroups per CU
    // instead of one 96-KiB frame (analysis 5.35 -> 4.77 ms per 65536 frames, same-box A/B).
    if (!g.stereo && g.C >= 4u && (g.C & 1u) == 0 && ((g.C / 2u) * g.B) % 4u == 0 && !g.stage_dbuf) {
        const uint32_t ch = g.C / 2u, lh = ana_layout(ch, g.B, ch, true, false, lpc).total;
        if (2u * lh <= kLdsLimit) {
            g.ana_split = true;
            g.nt_split = 64u * ch;
            g.lds_split = lh;
        }
    }
    // pack: double-buffer the staging when that keeps the register-limited occupancy
    // (4 workgroups per CU; 2 for 32-bit samples)
    const uint32_t pack_wgs = g.B == 4 ? 2u : 4u;
    g.pack_dbuf = pack_layout(g.C, g.B, g.image_bytes, true).total * pack_wgs <= kLdsLimit;
    if (k.pack_dbuf >= 0) g.pack_dbuf = g.pack_dbuf && k.pack_dbuf;
    // 32-bit samples (c5): the 48-KiB three-chunk ring (kernel 2) -- same-box A/B r4m, 2 reps:
    // c5 24.19-24.25k -> 24.67-24.68k MS/s (MD5 10.1 -> 9.5 ms, analysis 8.84 -> 8.58 ms beside
    // it); c3 neutral, C2 -4 %, so the others keep kernel 1
    if (g.B == 4u) g.md5_kernel = 2;
    if (k.md5_kernel_set) g.md5_kernel = k.md5_kernel;
    g.lds_pack = pack_layout(g.C, g.B, g.image_bytes, g.pack_dbuf).total;
    g.crc_hmax = crc_hmax_for(g.image_bytes, g.nt_pack);
    const bool pack4 = g.C == 2 && g.B == 2 && !lpc;
    if (pack4) g.nt_pack4 = k.pack4 == 0 ? 0u : 512u;  // A/B knob
    bool packw_dbuf = true;
    // k_packw (fg_packw.hpp) where k_pack's occupancy is poor: 32-bit samples (i64 lanes, 2 waves
    // per SIMD) or more than two written subframes (one workgroup per CU).  Mono/stereo 8-24-bit
    // frames stay on k_pack: its small single-buffered workgroups keep 4-5 frames in flight per
    // CU, which measured faster (c3 pack alone: 1.26 ms vs 1.40-1.66 ms for the packw variants).
    bool use_packw = g.B == 4u || n_out > 2u;
    if (k.packw >= 0) use_packw = k.packw != 0;  // A/B knob
    if (!g.nt_pack4 && use_packw) {
        // WPS waves per written subframe, 16 (<= 4 subframes) or 32 samples per lane;
        // double-buffered staging where two workgroups per CU still fit
        uint32_t wps = n_out <= 4u ? 4u : 2u;
        if (k.packw_wps2 && n_out <= 8u) wps = 2u;  // tuning knob
        g.nt_pack4 = 64u * n_out * wps;
        packw_dbuf = packw_layout(g.C, g.B, wps, g.image_bytes, true, n_out).total * 2u <= kLdsLimit;
        if (k.packw_dbuf >= 0) packw_dbuf = packw_dbuf && k.packw_dbuf;  // tuning knob
        g.pack_dbuf = packw_dbuf;  // k_pack then runs tail frames only (never double-buffered)
    }
    if (g.nt_pack4) {
        g.lds_pack4 = pack4 ? pack4_layout(g.image_bytes).total
                            : packw_layout(g.C, g.B, g.nt_pack4 / (64u * n_out), g.image_bytes, packw_dbuf, n_out).total;
        g.crc_hmax4 = crc_hmax_for(g.image_bytes, g.nt_pack4);
    }
    // Frames whose single-buffered k_packw staging admits one workgroup per CU and whose analysis
    // runs in channel halves are packed in channel halves too (two workgroups per CU, see k_packw)
    if (g.ana_split && use_packw && !packw_dbuf) {
        const uint32_t ch = g.C / 2u;
        const uint32_t img = fg_round16(frame_bound_bytes(kBlock, ch, g.bits, false) + 16u);
        const uint32_t lh = packw_layout(ch, g.B, 2u, img, false, ch).total;
        if (2u * lh <= kLdsLimit && k.pack_split != 0) {  // A/B knob
            g.pack_split = true;
            g.nt_psplit = 64u * ch * 2u;
            g.lds_psplit = lh;
            g.image_split = img;
            g.crc_hmaxs = crc_hmax_for(img, g.nt_psplit);
        }
    }
#if FG_DIAG
    if (g.C == 2 && g.B == 2 && !lpc && g.stereo) {
        // k_ana1 measured slower than k_analyze so far: opt-in
        g.ana1 = k.ana1 > 0;
        g.ana1_variant = k.ana1 == 2 ? 2u : 1u;
        g.fused = k.fused;  // A/B knob
        g.lds_fused = ana_layout(2, 2, 4, true, false, false, g.image_bytes).total;
        g.crc_hmaxf = crc_hmax_for(g.image_bytes, 256u);
    }
#endif
    if (g.lds > kLdsLimit || g.lds_tail > kLdsLimit || g.lds_pack > kLdsLimit || g.lds_pack4 > kLdsLimit)
        return FLACGPU_ERR_INVALID_CONFIG;
    return FLACGPU_OK;
}

// ---- the decoder's reconstruct kernel (fg_dec.hip: k_dec_recon) ------------------------------
// One workgroup of W waves restores W subframes at a time, each into a plane of LDS: `elem`-byte
// elements (4; 8 for 32-bit samples: the 33-bit side channel and the verifier decoder's 64-bit
// sums), plane_words of them: the block rounded up to B = 4096, 8192 or 16384, and B / 64 pad
// elements, one per segment of a B-sample frame (fg_dec.hip phys()).
// A frame of more channels than W takes ceil(C / W) rounds in each of two passes.
struct DecGeom {
    bool ok = false;
    uint32_t elem = 0, plane_words = 0, W = 0, lds = 0, passes = 0;
};

constexpr uint32_t kDecStaticLds = 16;  // k_dec_recon's own __shared__ words (static_assert there)

// channels 1..8, bits 8 / 16 / 24 / 32, block 1..FLACGPU_DECODER_MAX_BLOCK: the context's largest frame.
inline DecGeom dec_geometry(uint32_t channels, uint32_t bits, uint32_t block) {
    DecGeom g;
    if (channels < 1 || channels > 8 || (bits != 8 && bits != 16 && bits != 24 && bits != 32)) return g;
    if (block < 1 || block > FLACGPU_DECODER_MAX_BLOCK) return g;
    g.elem = bits == 32 ? 8u : 4u;
    const uint32_t B = block <= 4096u ? 4096u : (block <= 8192u ? 8192u : 16384u);
    g.plane_words = B + B / 64u;
    const uint32_t plane_bytes = g.plane_words * g.elem;
    if (B == 4096u) {
        // every channel's wave at once (8 x 16.25 KiB = 130 KiB at most); 64-bit planes: at most
        // four waves (4 x 32.5 KiB) -- what every context launched with before larger blocks existed
        g.W = bits == 32 ? (channels < 4u ? channels : 4u) : channels;
    } else {
        // one workgroup per CU: as many planes as the CU's LDS holds beside the kernel's own words
        const uint32_t fit = (kLdsLimit - kDecStaticLds) / plane_bytes;
        g.W = channels < fit ? channels : fit;
    }
    // the stereo decorrelation reads both planes of a frame in one round
    if (g.W < (channels < 2u ? channels : 2u)) return g;
    // (that rule alone would admit one 64-bit plane of 16384: the stated limit covers mono too)
    if (bits == 32 && block > FLACGPU_DECODER_MAX_BLOCK_32) return g;
    g.lds = g.W * plane_bytes;
    g.passes = channels > g.W ? 2u : 1u;
    g.ok = true;
    return g;
}

}  // namespace fg
