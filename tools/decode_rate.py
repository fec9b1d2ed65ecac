#!/usr/bin/env python3
"""Decode / verify rate of the device FLAC frame decoder beside the CPU verifier decoder.

CPU figure first (before anything initialises the GPU): fdec_frames_to_pcm of liboracle_fast on
one core over the C2 synthetic stream.  Then, per preset (c2: 2 x 16-bit fixed prediction; c5:
2 x 32-bit, LPC 12), a batch of frames encoded on the GPU and left in HBM is decoded by
flacgpu_decode_frames_device in verify mode (compare with the PCM) and in output mode (write the
PCM): HIP events around the call, warm-up, repeats, the median; the parse and reconstruct kernel
times from flacgpu_kernel_time in a pass of their own.  Writes one JSON document.

The index leg (--index-out) takes the C2 batch as a FLAC file: the host frame index
flacgpu_flac_index over its frames (wall clock, best of 3), the device index
flacgpu_flac_index_device over the same bytes in HBM (HIP events, warm-up, the median), the device
decode of the frames it found (the same way), and flacgpu_decode_file end to end (wall clock).

    python tools/decode_rate.py --out profiles/dec_rate.json --index-out profiles/index_rate.json
    python tools/decode_rate.py --legs index --index-out profiles/index_rate.json

The files leg (--files-out) cuts the same C2 batch into 64 files of 256 frames: a loop of
flacgpu_decode_file against one flacgpu_decode_files on the same context (wall clock, the two
alternated, best of 3 each after one warm call each, the MD5 engine the batch chose recorded), and
64 flacgpu_flac_index_device calls against one flacgpu_flac_index_streams_device over the same
bytes in HBM (HIP events, warm-up, the median).

    python tools/decode_rate.py --legs files --files-out profiles/decode_files_rate.json

The windows leg (--windows-out) takes the same 64 files of 256 frames and one window of 65536
samples per file, starting at a sample that is no multiple of the block size:
flacgpu_decode_windows_device from tables and positions that stay resident against
flacgpu_decode_streams_device on the same bytes (HIP events, the two alternated, the median), the
positions call alone, flacgpu_decode_files_windows against flacgpu_decode_files end to end (wall
clock, alternated, best of 3 each after one warm call each), and a call of windows that cover
whole streams with its timed kernels, whose difference bounds the copy pass.

    python tools/decode_rate.py --legs windows --windows-out profiles/decode_windows_rate.json

The deliver leg (--deliver-out; opt-in, not part of `all`) takes the windows leg's files and
windows: flacgpu_decode_windows_device_as (planar, padded; f32, and again bf16) against what a
caller of the byte call does to get the identical tensor -- flacgpu_decode_windows_device, then
view(int16) -> reshape -> to(float32) -> scale -> transpose -> contiguous() in torch -- alternated
(HIP events, the median), and windows that cover whole streams through both calls with their timed
kernels, whose differences bound the delivery pass and the copy pass.

    python tools/decode_rate.py --legs deliver --deliver-out profiles/decode_deliver_rate.json

The bigblock leg (--bigblock-out; opt-in, not part of `all`) takes one 16-bit stereo PCM buffer of
2^20 samples, encoded by the CPU oracle encoder at blocks 4096, 4608 and 16384 (--blocks), as
--streams streams of one device buffer through flacgpu_decode_streams_device -- the 4096 row on a
flacgpu_open context, the others on a decode-only one: HIP events around the call, warm-up, the
median, and the parse and reconstruct kernel times in a pass of their own.  FLACGPU_LIB names
another build of the library for the same row of an earlier commit.

    python tools/decode_rate.py --legs bigblock --bigblock-out profiles/decode_bigblock_rate.json

The mix leg (--mix-out; opt-in, not part of `all`) takes the windows leg's files and windows, stereo
to mono, f32, planar and padded: flacgpu_decode_windows_device_mix with the mask of both channels
against flacgpu_decode_windows_device_as followed by x.mean(dim=1, keepdim=True), alternated (HIP
events, the median).  The two tensors are compared; they may differ in the last place, since the
mix rounds the exact sum once and torch rounds each channel's element and then their mean.

    python tools/decode_rate.py --legs mix --mix-out profiles/decode_mix_rate.json

The resample leg (--resample-out; opt-in, not part of `all`) takes the same files and source windows,
both channels, f32, planar and padded: flacgpu_decode_windows_device_resample 44100 -> 48000 over the
output samples that sit in each source window, against flacgpu_decode_windows_device_mix of the
source window itself, alternated (HIP events, the median).  The difference is what the FIR pass adds
to a call bound by the parse kernel.  The first outputs of the first and the last file are compared
with flacgpu.resample_f32_host over the PCM, bit for bit.

    python tools/decode_rate.py --legs resample --resample-out profiles/decode_resample_rate.json

The features leg (--features-out; opt-in, not part of `all`) takes the resample leg's files and windows, both
channels, at n_fft 400, hop 160 and 80 mel rows, f32: flacgpu_decode_windows_device_features at the
files' own rate and 44100 -> 48000, each beside the call a caller had before it -- the _mix or
_resample delivery of the same samples, then torch.stft (zero padding at the crop's edges) and the
matmul with the same mel matrix -- alternated in one run.  It records the medians and their ratio; no
ratio is claimed in advance.  The first frames of the first and last window are compared with
flacgpu.features_f32_host bit for bit, and the interior frames of the two paths with each other.

    python tools/decode_rate.py --legs features --features-out profiles/decode_features_rate.json

The levels leg (--levels-out; opt-in, not part of `all`) takes the resample leg's files and windows and
measures them without delivering them: flacgpu_levels_windows_device at hop 441 and at hop = the
window, against flacgpu_decode_windows_device_as (I32, planar) followed by torch's abs().amax, sum
and double().square().sum a block.  Medians of --repeats alternated runs, both sides, between events
on the stream; the records of two windows are first compared with numpy over the PCM.

    python tools/decode_rate.py --legs levels --levels-out profiles/decode_levels_rate.json

The write leg (--write-out; opt-in, not part of `all`) takes the resample leg's PCM as 64 float32
[channel, time] tensors on the device and builds a bank of them at 16 bits two ways, alternated in one
process: FlacBank.from_tensors, and the route a caller had before it -- the tensors scaled, rounded
and cast by torch ops and moved to the host, Encoder.encode_files, FlacBank(files).  Wall clock with
the device synchronised at both ends, one warm call each, the medians of --repeats.  The first and
the last file of the two routes are compared byte for byte, and a crop of each with the tensor.

    python tools/decode_rate.py --legs write --write-out profiles/bank_write_rate.json

The downmix leg (--downmix-out; opt-in, not part of `all`) takes 6-channel 16-bit files of the same
sizes and windows and delivers them as stereo f32, planar and padded, two ways, alternated in one
process: flacgpu_decode_windows_device_to with the ITU 6-to-2 weight matrix, and the route a caller
had before it -- flacgpu_decode_windows_device_as of all six channels followed by torch.einsum with
the same matrix.  Wall clock with the device synchronised at both ends, one warm call each, the
medians of --repeats.  The first and the last window are compared with flacgpu.mix_weights_f32_host
over the PCM bit for bit; the two tensors are compared with each other (they may differ in the last
place: einsum need not be the one chain of fused multiply-adds).  No ratio is claimed in advance.

    python tools/decode_rate.py --legs downmix --downmix-out profiles/decode_downmix_rate.json

The fir leg (--fir-out; opt-in, not part of `all`) takes the resample leg's files and windows, both
channels, f32, planar and padded, through a causal filter of 64, 512 and 4096 taps:
flacgpu_decode_windows_device_fir against flacgpu_decode_windows_device_as followed by torch, once
as conv1d and once as an rfft / irfft product, alternated in one process (HIP events, three warm
calls each, the medians of --repeats).  The first outputs of the first and the last window are
compared with flacgpu.fir_f32_host over the PCM bit for bit; the torch routes, which read zeros
before the crop where the call reads the file, are compared with the call on the interior samples,
the largest difference relative to the largest value.  No ratio is claimed in advance, and the
kernel's own time is not separated from the call's.

    python tools/decode_rate.py --legs fir --fir-out profiles/decode_fir_rate.json
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zig-flac_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PRESETS = {"c2": (2, 16, 44100, 0), "c5": (2, 32, 192000, 12)}


def cpu_rate(frames: int) -> dict:
    import oracle_ref
    import synth

    ch, bits, rate, _ = PRESETS["c2"]
    n = frames * 4096
    pcm = synth.synth_pcm(n, ch, bits, rate)
    L = oracle_ref.lib(fast=True)
    L.fdec_frames_to_pcm.restype = ctypes.c_long
    bitstream, _, _ = oracle_ref.encode_stream(pcm, ch, bits, rate)
    out = ctypes.create_string_buffer(len(pcm))
    best = None
    for _ in range(3):
        t = time.perf_counter()
        r = L.fdec_frames_to_pcm(bitstream, ctypes.c_size_t(len(bitstream)), ch, bits, rate, bits // 8, out,
                                 ctypes.c_uint64(n), ctypes.c_uint64(0), None, ctypes.c_uint64(0))
        dt = time.perf_counter() - t
        assert r == n and out.raw == pcm
        best = dt if best is None else min(best, dt)
    return {"frames": frames, "seconds": best, "msamples_per_s": n / best / 1e6}


def gpu_rate(name: str, frames: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacgpu
    import synth

    ch, bits, rate, lpc = PRESETS[name]
    dev = torch.device("cuda", 0)
    n = frames * 4096
    # a few distinct seconds of signal, tiled: the batch's content, not its length, costs host time
    unit = synth.synth_pcm(64 * 4096, ch, bits, rate)
    pcm = (unit * ((frames + 63) // 64))[: n * ch * (bits // 8)]
    with flacgpu.Encoder(ch, bits, rate, device=0, max_frames=frames, lpc_order=lpc) as enc:
        plan = enc.plan([0], [n])
        d_pcm = torch.from_numpy(np.frombuffer(pcm, dtype=np.uint8).copy()).to(dev)
        d_out = torch.zeros(int(plan.out_bound), dtype=torch.uint8, device=dev)
        d_fb = torch.zeros(frames, dtype=torch.int32, device=dev)
        d_off = torch.zeros(frames, dtype=torch.int64, device=dev)
        d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
        d_res = torch.zeros(32 * frames, dtype=torch.uint8, device=dev)
        d_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        d_dec = torch.zeros(len(pcm), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        enc.encode_plan_device(plan, d_pcm.data_ptr(), d_out.data_ptr(), int(plan.out_bound), d_fb.data_ptr(),
                               d_off.data_ptr(), d_tot.data_ptr(), None, st)
        enc.sync_check(st)
        bitstream_bytes = int(d_tot[0].item())

        def run(mode):
            enc.decode_frames_device(d_out.data_ptr(), d_off.data_ptr(), d_fb.data_ptr(), frames, d_res.data_ptr(),
                                     d_bad.data_ptr(), d_pcm_out=d_dec.data_ptr() if mode == "output" else None,
                                     pcm_cap=len(pcm), d_pcm_expect=d_pcm.data_ptr() if mode == "verify" else None,
                                     stream=st)

        res = {"frames": frames, "channels": ch, "bits": bits, "lpc": lpc, "bitstream_bytes": bitstream_bytes}
        for mode in ("verify", "output"):
            for _ in range(warmup):
                run(mode)
            enc.sync_check(st)
            assert int(d_bad.item()) == 0
            ms = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(mode)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            med = statistics.median(ms)
            res[mode] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "msamples_per_s": n / med / 1e3}
            # the two kernels, timed in a pass of their own
            enc.set_timing(True)
            enc.reset_timing()
            for _ in range(repeats):
                run(mode)
            enc.sync_check(st)
            np_, parse = enc.kernel_time(flacgpu.K_DEC_PARSE)
            nr, recon = enc.kernel_time(flacgpu.K_DEC_RECON)
            enc.set_timing(False)
            res[mode]["parse_ms"] = parse / max(np_, 1)
            res[mode]["recon_ms"] = recon / max(nr, 1)
        assert d_dec.cpu().numpy().tobytes() == pcm, "decoded PCM differs from the input"
        plan.close()
    return res


def index_rate(frames: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacgpu
    import synth

    ch, bits, rate, _ = PRESETS["c2"]
    dev = torch.device("cuda", 0)
    n = frames * 4096
    unit = synth.synth_pcm(64 * 4096, ch, bits, rate)
    pcm = (unit * ((frames + 63) // 64))[: n * ch * (bits // 8)]
    L = flacgpu.load_library()
    with flacgpu.Encoder(ch, bits, rate, device=0, max_frames=frames) as enc:
        flac = enc.encode_file(pcm)
        # host index of the frames alone (the bytes the device index gets), best of 3
        si = flacgpu.StreamInfo()
        first, nf = ctypes.c_size_t(0), ctypes.c_size_t(0)
        cap = len(flac) // 8 + 1
        sizes = (ctypes.c_uint32 * cap)()
        assert L.flacgpu_flac_index(flac, len(flac), ctypes.byref(si), ctypes.byref(first), sizes, cap, ctypes.byref(nf)) == 0
        assert nf.value == frames
        body = flac[first.value:]
        host_s = None
        for _ in range(3):
            t = time.perf_counter()
            rc = L.flacgpu_flac_index(body, len(body), None, None, sizes, cap, ctypes.byref(nf))
            dt = time.perf_counter() - t
            assert rc == 0 and nf.value == frames
            host_s = dt if host_s is None else min(host_s, dt)
        want = np.frombuffer(sizes, dtype=np.uint32)[:frames].copy()
        # the same bytes in HBM, as they sit in the file (the first frame's offset is odd)
        d_file = torch.from_numpy(np.frombuffer(flac, dtype=np.uint8).copy()).to(dev)
        d_off = torch.zeros(cap, dtype=torch.int64, device=dev)
        d_fb = torch.zeros(cap, dtype=torch.int32, device=dev)
        d_ir = torch.zeros(16, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(32 * frames, dtype=torch.uint8, device=dev)
        d_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        d_dec = torch.zeros(len(pcm), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        d_frames = d_file.data_ptr() + first.value

        def index():
            enc.flac_index_device(d_frames, len(body), d_off.data_ptr(), d_fb.data_ptr(), cap, d_ir.data_ptr(),
                                  stream_bits=bits, stream_rate=rate, stream=st)

        def decode():
            enc.decode_frames_device(d_frames, d_off.data_ptr(), d_fb.data_ptr(), frames, d_res.data_ptr(),
                                     d_bad.data_ptr(), d_pcm_out=d_dec.data_ptr(), pcm_cap=len(pcm), stream=st)

        def timed(fn):
            for _ in range(warmup):
                fn()
            enc.sync_check(st)
            ms = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

        res = {"frames": frames, "channels": ch, "bits": bits, "file_bytes": len(flac), "frame_bytes": len(body),
               "first_frame_offset": first.value,
               "host_index": {"seconds_best_of_3": host_s, "mb_per_s": len(body) / host_s / 1e6}}
        res["device_index"] = timed(index)
        ir = flacgpu.IndexResult.from_buffer_copy(d_ir.cpu().numpy().tobytes())
        assert ir.status == 0 and ir.n_frames == frames
        assert (d_fb[:frames].cpu().numpy().view(np.uint32) == want).all(), "device index differs from the host index"
        res["device_index"]["gb_per_s"] = len(body) / res["device_index"]["ms_median"] / 1e6
        res["device_index"]["x_host_index"] = host_s * 1e3 / res["device_index"]["ms_median"]
        res["device_decode"] = timed(decode)
        assert int(d_bad.item()) == 0 and d_dec.cpu().numpy().tobytes() == pcm
        res["device_index"]["of_device_decode"] = res["device_index"]["ms_median"] / res["device_decode"]["ms_median"]
        # the whole file, host buffers in and out (the first call allocates: not timed)
        out = ctypes.create_string_buffer(len(pcm))
        ns, ok = ctypes.c_uint64(0), ctypes.c_int(0)
        wall = []
        for i in range(4):
            t = time.perf_counter()
            rc = L.flacgpu_decode_file(enc.ctx, flac, len(flac), out, len(pcm), ctypes.byref(ns), ctypes.byref(ok))
            wall.append(time.perf_counter() - t)
            assert rc == 0 and ok.value == 1 and ns.value == n
        assert out.raw == pcm
        res["decode_file"] = {"seconds_first_call": wall[0], "seconds_best_of_3": min(wall[1:]),
                              "msamples_per_s": n / min(wall[1:]) / 1e6}
        # what of it is the MD5 chain of the PCM on one host core
        import hashlib
        t = time.perf_counter()
        hashlib.md5(pcm).digest()
        res["decode_file"]["hashlib_md5_seconds"] = time.perf_counter() - t
    return res


def files_rate(n_files: int, frames_each: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacgpu
    import synth

    ch, bits, rate, _ = PRESETS["c2"]
    per = ch * (bits // 8)
    dev = torch.device("cuda", 0)
    unit = synth.synth_pcm(64 * 4096, ch, bits, rate)
    n_each = frames_each * 4096
    pcm = (unit * ((frames_each + 63) // 64))[: n_each * per]
    L = flacgpu.load_library()
    with flacgpu.Encoder(ch, bits, rate, device=0, max_frames=n_files * frames_each) as enc:
        flacs = enc.encode_files([pcm] * n_files)
        first = flacgpu.flac_index(flacs[0])[1]
        P = ctypes.c_void_p
        srcs = [ctypes.create_string_buffer(f, len(f)) for f in flacs]
        outs = [ctypes.create_string_buffer(len(pcm)) for _ in flacs]
        a_src = (P * n_files)(*[ctypes.addressof(b) for b in srcs])
        a_out = (P * n_files)(*[ctypes.addressof(b) for b in outs])
        a_len = (ctypes.c_size_t * n_files)(*[len(f) for f in flacs])
        a_cap = (ctypes.c_size_t * n_files)(*[len(pcm)] * n_files)
        ns = (ctypes.c_uint64 * n_files)()
        ok = (ctypes.c_int * n_files)()
        status = (ctypes.c_int * n_files)()

        def loop():
            one_ns, one_ok = ctypes.c_uint64(0), ctypes.c_int(0)
            t = time.perf_counter()
            for i in range(n_files):
                rc = L.flacgpu_decode_file(enc.ctx, srcs[i], len(flacs[i]), outs[i], len(pcm), ctypes.byref(one_ns),
                                           ctypes.byref(one_ok))
                assert rc == 0 and one_ok.value == 1 and one_ns.value == n_each
            return time.perf_counter() - t

        def batch():
            t = time.perf_counter()
            rc = L.flacgpu_decode_files(enc.ctx, n_files, a_src, a_len, a_out, a_cap, ns, ok, status)
            dt = time.perf_counter() - t
            assert rc == 0 and list(status) == [0] * n_files and list(ok) == [1] * n_files and list(ns) == [n_each] * n_files
            return dt

        loop()  # one warm call each: the allocations
        batch()
        assert all(o.raw == pcm for o in outs)
        t_loop, t_batch = [], []
        for _ in range(3):
            t_loop.append(loop())
            t_batch.append(batch())
        engine = flacgpu.md5_engine_for(n_files, len(pcm), n_files * len(pcm))
        total = n_files * n_each
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits,
               "pcm_bytes": n_files * len(pcm), "flac_bytes": sum(len(f) for f in flacs),
               "md5_engine": "device" if engine == flacgpu.MD5_DEVICE else "host",
               "md5_rates": flacgpu.md5_rates().as_dict(),
               "decode_file_loop": {"seconds_best_of_3": min(t_loop), "seconds": t_loop,
                                    "msamples_per_s": total / min(t_loop) / 1e6},
               "decode_files": {"seconds_best_of_3": min(t_batch), "seconds": t_batch,
                                "msamples_per_s": total / min(t_batch) / 1e6}}
        res["decode_files"]["x_loop"] = min(t_loop) / min(t_batch)

        # the index alone: the files' frames in one HBM buffer, each at a 64-byte aligned offset
        bodies = [f[first:] for f in flacs]
        offs, at = [], 0
        for b in bodies:
            offs.append(at)
            at += (len(b) + 63) & ~63
        host = np.zeros(at + 16, dtype=np.uint8)
        for o, b in zip(offs, bodies):
            host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        d_buf = torch.from_numpy(host).to(dev)
        caps = [len(b) // 8 + 1 for b in bodies]
        tfirst = [int(v) for v in np.cumsum([0] + caps)[:-1]]
        d_off = torch.zeros(sum(caps), dtype=torch.int64, device=dev)
        d_fb = torch.zeros(sum(caps), dtype=torch.int32, device=dev)
        d_ir = torch.zeros(16 * n_files, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        lens = [len(b) for b in bodies]
        # the host arrays of the batched call, built once: the timed region is the C call
        u64 = lambda v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
        h_offs, h_lens, h_first, h_caps = u64(offs), u64(lens), u64(tfirst), u64(caps)
        h_bits, h_rates = (ctypes.c_uint32 * n_files)(*[bits] * n_files), (ctypes.c_uint32 * n_files)(*[rate] * n_files)
        stream = flacgpu._stream(st)

        def singles():
            for i in range(n_files):
                rc = L.flacgpu_flac_index_device(enc.ctx, d_buf.data_ptr() + offs[i], lens[i], bits, rate,
                                                 d_off.data_ptr() + 8 * tfirst[i], d_fb.data_ptr() + 4 * tfirst[i], caps[i],
                                                 d_ir.data_ptr() + 16 * i, stream)
                assert rc == 0

        def batched():
            rc = L.flacgpu_flac_index_streams_device(enc.ctx, d_buf.data_ptr(), n_files, h_offs, h_lens, h_bits, h_rates,
                                                     h_first, h_caps, d_off.data_ptr(), d_fb.data_ptr(), d_ir.data_ptr(),
                                                     stream)
            assert rc == 0

        def timed(fn):
            for _ in range(warmup):
                fn()
            enc.sync_check(st)
            ms = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

        def counts():
            raw = d_ir.cpu().numpy().tobytes()
            return [(r.status, r.n_frames) for r in (flacgpu.IndexResult * n_files).from_buffer_copy(raw)]

        res["index_singles"] = timed(singles)
        assert counts() == [(0, frames_each)] * n_files
        table = d_fb.cpu().numpy().copy()
        d_fb.zero_()
        d_ir.zero_()
        res["index_streams"] = timed(batched)
        assert counts() == [(0, frames_each)] * n_files and (d_fb.cpu().numpy() == table).all()
        res["index_streams"]["x_singles"] = res["index_singles"]["ms_median"] / res["index_streams"]["ms_median"]
        res["index_bytes"] = sum(lens)
    return res


@contextlib.contextmanager
def resident_windows(n_files: int, frames_each: int, window: int, channels: int = 0):
    """The resident set of the windows, deliver and mix legs: n_files C2 files (`channels`: of that
    many channels instead of two) of frames_each frames
    encoded on the GPU, their frames in one HBM buffer at 64-byte offsets and indexed once, and one
    window of `window` samples per file from a start that is no multiple of the block size.  The
    positions are the caller's to queue (r.positions()): the windows leg times them."""
    from types import SimpleNamespace

    import numpy as np
    import torch

    import flacgpu
    import synth

    ch, bits, rate, _ = PRESETS["c2"]
    ch = channels or ch
    per = ch * (bits // 8)
    dev = torch.device("cuda", 0)
    unit = synth.synth_pcm(64 * 4096, ch, bits, rate)
    n_each = frames_each * 4096
    pcm = (unit * ((frames_each + 63) // 64))[: n_each * per]
    start = (n_each // 3 // 4096) * 4096 + 1234  # not a multiple of the block size
    assert start % 4096 and start + window <= n_each
    with flacgpu.Encoder(ch, bits, rate, device=0, max_frames=n_files * frames_each) as enc:
        flacs = enc.encode_files([pcm] * n_files)
        first = flacgpu.flac_index(flacs[0])[1]
        bodies = [f[first:] for f in flacs]
        offs, at = [], 0
        for b in bodies:
            offs.append(at)
            at += (len(b) + 63) & ~63
        host = np.zeros(at + 16, dtype=np.uint8)
        for o, b in zip(offs, bodies):
            host[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        d_buf = torch.from_numpy(host).to(dev)
        lens = [len(b) for b in bodies]
        caps = [n // 8 + 1 for n in lens]
        tfirst = [int(v) for v in np.cumsum([0] + caps)[:-1]]
        d_off = torch.zeros(sum(caps), dtype=torch.int64, device=dev)
        d_fb = torch.zeros(sum(caps), dtype=torch.int32, device=dev)
        d_pos = torch.zeros(sum(caps), dtype=torch.int64, device=dev)
        d_tot = torch.zeros(n_files, dtype=torch.int64, device=dev)
        d_ir = torch.zeros(16 * n_files, dtype=torch.uint8, device=dev)
        d_wres = torch.zeros(32 * n_files, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        sbits, srates = [bits] * n_files, [rate] * n_files
        enc.flac_index_streams_device(d_buf.data_ptr(), offs, lens, tfirst, caps, d_off.data_ptr(), d_fb.data_ptr(),
                                      d_ir.data_ptr(), stream_bits=sbits, stream_rates=srates, stream=st)

        def positions():
            enc.flac_positions_streams_device(d_buf.data_ptr(), tfirst, caps, d_off.data_ptr(), d_fb.data_ptr(),
                                              d_ir.data_ptr(), d_pos.data_ptr(), d_tot.data_ptr(), stream_bits=sbits,
                                              stream_rates=srates, stream=st)

        def results():
            """[(status, n_samples)] of the last window call."""
            raw = d_wres.cpu().numpy().tobytes()
            return [(r.status, r.n_samples) for r in (flacgpu.WindowResult * n_files).from_buffer_copy(raw)]

        yield SimpleNamespace(
            enc=enc, ch=ch, bits=bits, rate=rate, per=per, dev=dev, pcm=pcm, n_each=n_each, start=start, flacs=flacs, offs=offs,
            lens=lens, d_buf=d_buf, d_wres=d_wres, st=st, sbits=sbits, srates=srates, positions=positions, results=results,
            tables=(d_buf.data_ptr(), tfirst, d_off.data_ptr(), d_fb.data_ptr(), d_ir.data_ptr(), d_pos.data_ptr(),
                    d_tot.data_ptr()),
            crops=[(i, start, window) for i in range(n_files)])


def event_ms(fn):
    """fn's time on the current stream between two HIP events."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms, keep=False):
    res = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    return dict(res, ms=ms) if keep else res


def windows_rate(n_files: int, frames_each: int, window: int, warmup: int, repeats: int) -> dict:
    import torch

    import flacgpu

    L = flacgpu.load_library()
    with resident_windows(n_files, frames_each, window) as r:
        enc, per, pcm, n_each, start, st, flacs, crops = r.enc, r.per, r.pcm, r.n_each, r.start, r.st, r.flacs, r.crops
        ch, bits, lens, positions, window_results = r.ch, r.bits, r.lens, r.positions, r.results
        want = pcm[start * per:(start + window) * per]
        d_sres = torch.zeros(32 * n_files, dtype=torch.uint8, device=r.dev)
        d_win = torch.zeros(n_files * window * per, dtype=torch.uint8, device=r.dev)
        d_all = torch.zeros(n_files * len(pcm), dtype=torch.uint8, device=r.dev)
        crop_offs, crop_caps = [i * window * per for i in range(n_files)], [window * per] * n_files
        wholes = [(i, 0, n_each) for i in range(n_files)]
        whole_offs, whole_caps = [i * len(pcm) for i in range(n_files)], [len(pcm)] * n_files

        def windows(wins, w_offs, w_caps, d_out):
            enc.decode_windows_device(*r.tables, wins, d_out.data_ptr(), w_offs, w_caps, r.d_wres.data_ptr(), stream=st)

        def streams():
            enc.decode_streams_device(r.d_buf.data_ptr(), r.offs, lens, d_all.data_ptr(), whole_offs, whole_caps,
                                      d_sres.data_ptr(), stream_bits=r.sbits, stream_rates=r.srates, stream=st)

        for _ in range(warmup):
            positions()
            windows(crops, crop_offs, crop_caps, d_win)
            streams()
        enc.sync_check(st)
        assert window_results() == [(0, window)] * n_files
        got = d_win.cpu().numpy().tobytes()
        assert all(got[o:o + len(want)] == want for o in crop_offs), "a window differs from the PCM it was cut from"
        ms_pos = [event_ms(positions) for _ in range(repeats)]
        ms_win, ms_all = [], []
        for _ in range(repeats):  # the two alternated
            ms_win.append(event_ms(lambda: windows(crops, crop_offs, crop_caps, d_win)))
            ms_all.append(event_ms(streams))
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "window_samples": window,
               "window_start": start, "flac_bytes": sum(lens), "pcm_bytes": n_files * len(pcm),
               "window_bytes": n_files * window * per,
               "positions": summary(ms_pos), "decode_windows_device": summary(ms_win), "decode_streams_device": summary(ms_all)}
        res["decode_windows_device"]["x_decode_streams_device"] = res["decode_streams_device"]["ms_median"] / res["decode_windows_device"]["ms_median"]
        # the copy: windows that cover whole streams do everything decode_streams_device does but the
        # index, plus the copy pass; events around the call, and the timed kernels of the same call
        # in a pass of their own.  The call less its timed kernels is an upper bound of the copy (it
        # holds the one wait, the uploads, the small kernels and the gaps between launches too).
        windows(wholes, whole_offs, whole_caps, d_all)
        enc.sync_check(st)
        assert window_results() == [(0, n_each)] * n_files
        assert d_all[:len(pcm)].cpu().numpy().tobytes() == pcm and d_all[-len(pcm):].cpu().numpy().tobytes() == pcm
        ms_whole = [event_ms(lambda: windows(wholes, whole_offs, whole_caps, d_all)) for _ in range(repeats)]
        enc.set_timing(True)
        enc.reset_timing()
        for _ in range(repeats):
            windows(wholes, whole_offs, whole_caps, d_all)
        enc.sync_check(st)
        kernels = {name: enc.kernel_time(k)[1] / repeats for name, k in
                   (("scan_ms", flacgpu.K_SCAN), ("parse_ms", flacgpu.K_DEC_PARSE), ("recon_ms", flacgpu.K_DEC_RECON))}
        enc.set_timing(False)
        res["whole_stream_windows"] = dict(summary(ms_whole), **kernels)
        copy_ms = statistics.median(ms_whole) - sum(kernels.values())
        res["whole_stream_windows"]["copy_ms_upper_bound"] = copy_ms
        res["whole_stream_windows"]["copy_gb_per_s_at_least"] = 2 * n_files * len(pcm) / copy_ms / 1e6  # read + write

        # ---- end to end from host memory: the windows against the whole files, alternated ----
        P = ctypes.c_void_p
        srcs = [ctypes.create_string_buffer(f, len(f)) for f in flacs]
        outs = [ctypes.create_string_buffer(len(pcm)) for _ in flacs]
        wouts = [ctypes.create_string_buffer(window * per) for _ in flacs]
        a_src = (P * n_files)(*[ctypes.addressof(b) for b in srcs])
        a_out = (P * n_files)(*[ctypes.addressof(b) for b in outs])
        a_wout = (P * n_files)(*[ctypes.addressof(b) for b in wouts])
        a_len = (ctypes.c_size_t * n_files)(*[len(f) for f in flacs])
        a_cap = (ctypes.c_size_t * n_files)(*[len(pcm)] * n_files)
        a_wcap = (ctypes.c_size_t * n_files)(*[window * per] * n_files)
        w_file = (ctypes.c_uint32 * n_files)(*range(n_files))
        w_start = (ctypes.c_uint64 * n_files)(*[start] * n_files)
        w_count = (ctypes.c_uint64 * n_files)(*[window] * n_files)
        ns = (ctypes.c_uint64 * n_files)()
        ok = (ctypes.c_int * n_files)()
        status = (ctypes.c_int * n_files)()

        def files_windows():
            t = time.perf_counter()
            rc = L.flacgpu_decode_files_windows(enc.ctx, n_files, a_src, a_len, n_files, w_file, w_start, w_count, a_wout,
                                                a_wcap, ns, status)
            dt = time.perf_counter() - t
            assert rc == 0 and list(status) == [0] * n_files and list(ns) == [window] * n_files
            return dt

        def files_whole():
            t = time.perf_counter()
            rc = L.flacgpu_decode_files(enc.ctx, n_files, a_src, a_len, a_out, a_cap, ns, ok, status)
            dt = time.perf_counter() - t
            assert rc == 0 and list(status) == [0] * n_files and list(ok) == [1] * n_files
            return dt

        files_windows()  # one warm call each: the allocations
        files_whole()
        assert all(o.raw == want for o in wouts) and all(o.raw == pcm for o in outs)
        t_win, t_all = [], []
        for _ in range(3):
            t_win.append(files_windows())
            t_all.append(files_whole())
        res["decode_files_windows"] = {"seconds_best_of_3": min(t_win), "seconds": t_win}
        res["decode_files"] = {"seconds_best_of_3": min(t_all), "seconds": t_all}
        res["decode_files_windows"]["x_decode_files"] = min(t_all) / min(t_win)
    return res


def deliver_rate(n_files: int, frames_each: int, window: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacgpu

    with resident_windows(n_files, frames_each, window) as r:
        enc, ch, bits, per, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.per, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        planar_pad = flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD

        def deliver(wins, fmt, x):
            count = wins[0][2]
            enc.decode_windows_device_as(*tables, wins, fmt, planar_pad, x.data_ptr(), [i * ch * count for i in range(len(wins))],
                                         [ch * count] * len(wins), d_wres.data_ptr(), stream=st)

        def copy(wins, d_out):
            count = wins[0][2]
            enc.decode_windows_device(*tables, wins, d_out.data_ptr(), [i * count * per for i in range(len(wins))],
                                      [count * per] * len(wins), d_wres.data_ptr(), stream=st)

        def today(wins, d_out, dtype):
            """What a caller of the byte call does for the same [window, channel, time] tensor."""
            copy(wins, d_out)
            x = d_out.view(torch.int16).view(len(wins), wins[0][2], ch).to(torch.float32) * (2.0 ** -(bits - 1))
            return x.to(dtype).transpose(1, 2).contiguous()

        def all_ok(n):
            return r.results() == [(0, n)] * n_files

        d_win = torch.zeros(n_files * window * per, dtype=torch.uint8, device=dev)
        x32 = torch.zeros((n_files, ch, window), dtype=torch.float32, device=dev)
        x16 = torch.zeros((n_files, ch, window), dtype=torch.bfloat16, device=dev)
        legs = {"as_f32": lambda: deliver(crops, flacgpu.SAMPLE_F32, x32),
                "torch_f32": lambda: today(crops, d_win, torch.float32),
                "as_bf16": lambda: deliver(crops, flacgpu.SAMPLE_BF16, x16),
                "torch_bf16": lambda: today(crops, d_win, torch.bfloat16)}
        for _ in range(warmup):
            for fn in legs.values():
                fn()
        enc.sync_check(st)
        assert all_ok(window)
        assert torch.equal(x32, today(crops, d_win, torch.float32)), "the delivered f32 tensor differs from the torch sequence's"
        assert torch.equal(x16, today(crops, d_win, torch.bfloat16)), "the delivered bf16 tensor differs from the torch sequence's"
        ms = {k: [] for k in legs}
        for _ in range(repeats):  # alternated
            for k, fn in legs.items():
                ms[k].append(event_ms(fn))
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "window_samples": window,
               "window_start": start, "window_bytes": n_files * window * per, "layout": "planar, padded"}
        for k in legs:
            res[k] = summary(ms[k])
        for f in ("f32", "bf16"):
            res["as_" + f]["x_torch"] = res["torch_" + f]["ms_median"] / res["as_" + f]["ms_median"]

        # the delivery pass: windows that cover whole streams, events around the call and the timed
        # kernels of the same call in a pass of their own; the call less its timed kernels is an upper
        # bound of the pass (it holds the one wait, the uploads, the small kernels and the gaps too).
        # The byte call the same way, for its copy pass, in the same run.
        wholes = [(i, 0, n_each) for i in range(n_files)]
        d_all = torch.zeros(n_files * len(pcm), dtype=torch.uint8, device=dev)
        xall = torch.zeros((n_files, ch, n_each), dtype=torch.float32, device=dev)

        def bound(fn):
            fn()
            enc.sync_check(st)
            assert all_ok(n_each)
            whole = [event_ms(fn) for _ in range(repeats)]
            enc.set_timing(True)
            enc.reset_timing()
            for _ in range(repeats):
                fn()
            enc.sync_check(st)
            kernels = {name: enc.kernel_time(k)[1] / repeats for name, k in
                       (("scan_ms", flacgpu.K_SCAN), ("parse_ms", flacgpu.K_DEC_PARSE), ("recon_ms", flacgpu.K_DEC_RECON))}
            enc.set_timing(False)
            return dict(summary(whole), **kernels), statistics.median(whole) - sum(kernels.values())

        res["whole_stream_as_f32"], deliver_ms = bound(lambda: deliver(wholes, flacgpu.SAMPLE_F32, xall))
        res["whole_stream_as_f32"]["deliver_ms_upper_bound"] = deliver_ms
        res["whole_stream_as_f32"]["deliver_gb_per_s_at_least"] = 3 * n_files * len(pcm) / deliver_ms / 1e6  # read + write twice as wide
        want = torch.from_numpy(np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch).T.astype(np.float32) * np.float32(2.0 ** -15))
        assert torch.equal(xall[0].cpu(), want) and torch.equal(xall[-1].cpu(), want)
        res["whole_stream_bytes"], copy_ms = bound(lambda: copy(wholes, d_all))
        res["whole_stream_bytes"]["copy_ms_upper_bound"] = copy_ms
        res["pcm_bytes"] = n_files * len(pcm)
    return res


def mix_rate(n_files: int, frames_each: int, window: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacgpu

    with resident_windows(n_files, frames_each, window) as r:
        enc, ch, bits, per, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.per, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        planar_pad = flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD
        x_mix = torch.zeros((n_files, 1, window), dtype=torch.float32, device=dev)
        x_as = torch.zeros((n_files, ch, window), dtype=torch.float32, device=dev)

        def mix():
            enc.decode_windows_device_mix(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, [3], x_mix.data_ptr(),
                                          [i * window for i in range(n_files)], [window] * n_files, d_wres.data_ptr(), stream=st)
            return x_mix

        def as_then_mean():
            enc.decode_windows_device_as(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, x_as.data_ptr(),
                                         [i * ch * window for i in range(n_files)], [ch * window] * n_files, d_wres.data_ptr(),
                                         stream=st)
            return x_as.mean(dim=1, keepdim=True)

        def all_ok():
            return r.results() == [(0, window)] * n_files

        legs = {"mix_f32": mix, "as_f32_then_mean": as_then_mean}
        for _ in range(warmup):
            for fn in legs.values():
                fn()
                enc.sync_check(st)
                assert all_ok()
        # the expectation from the PCM: the exact sum, rounded once
        v = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)[start:start + window].astype(np.int64).sum(axis=1)
        want = torch.from_numpy(v.astype(np.float32) * np.float32(2.0 ** -bits))
        got = mix().cpu()
        assert torch.equal(got[0, 0], want) and torch.equal(got[-1, 0], want), "the mixed tensor differs from the PCM's exact mean"
        other = as_then_mean().cpu()
        ms = {k: [] for k in legs}
        for _ in range(repeats):  # alternated
            for k, fn in legs.items():
                ms[k].append(event_ms(fn))
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "out_channels": 1, "mask": 3,
               "window_samples": window, "window_start": start, "window_bytes": n_files * window * per,
               "layout": "f32, planar, padded", "warmup": warmup, "repeats": repeats,
               "elements_that_differ_from_torch_mean": int((got != other).sum()), "elements": got.numel()}
        for k in legs:
            res[k] = summary(ms[k], keep=True)
        res["mix_f32"]["x_as_then_mean"] = res["as_f32_then_mean"]["ms_median"] / res["mix_f32"]["ms_median"]
    return res


def downmix_rate(n_files: int, frames_each: int, window: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacbank
    import flacgpu

    W = flacbank.downmix_matrix(6, 2, "itu")
    with resident_windows(n_files, frames_each, window, channels=6) as r:
        enc, ch, bits, per, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.per, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        planar_pad = flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD
        x_to = torch.zeros((n_files, 2, window), dtype=torch.float32, device=dev)
        x_as = torch.zeros((n_files, ch, window), dtype=torch.float32, device=dev)
        d_w = torch.from_numpy(W).to(dev)

        def to():
            enc.decode_windows_device_to(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, x_to.data_ptr(),
                                         [i * 2 * window for i in range(n_files)], [2 * window] * n_files, d_wres.data_ptr(),
                                         channel_weights=W, stream=st)
            return x_to

        def as_then_einsum():
            enc.decode_windows_device_as(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, x_as.data_ptr(),
                                         [i * ch * window for i in range(n_files)], [ch * window] * n_files, d_wres.data_ptr(),
                                         stream=st)
            return torch.einsum("kc,nct->nkt", d_w, x_as)

        def wall_ms(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3

        legs = {"to_itu_f32": to, "as_f32_then_einsum": as_then_einsum}
        for fn in legs.values():  # one warm call each
            fn()
            enc.sync_check(st)
            assert r.results() == [(0, window)] * n_files
        # the expectation from the PCM: the host statement of the rule
        v = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)[start:start + window]
        want = torch.from_numpy(np.ascontiguousarray(flacgpu.mix_weights_f32_host(v, bits, W).T))
        got = to().cpu()
        assert torch.equal(got[0], want) and torch.equal(got[-1], want), "the downmix differs from the host statement of the rule"
        other = as_then_einsum().cpu()
        ms = {k: [] for k in legs}
        for _ in range(repeats):  # alternated
            for k, fn in legs.items():
                ms[k].append(wall_ms(fn))
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "out_channels": 2,
               "weights": [[float(x) for x in row] for row in W], "window_samples": window, "window_start": start,
               "window_bytes": n_files * window * per, "layout": "f32, planar, padded", "clock": "wall, device synchronised",
               "warm_calls": 1, "repeats": repeats, "elements_that_differ_from_einsum": int((got != other).sum()),
               "max_abs_difference_from_einsum": float((got - other).abs().max()), "elements": got.numel()}
        for k in legs:
            res[k] = summary(ms[k], keep=True)
        res["to_itu_f32"]["x_as_then_einsum"] = res["as_f32_then_einsum"]["ms_median"] / res["to_itu_f32"]["ms_median"]
    return res


def resample_rate(n_files: int, frames_each: int, window: int, warmup: int, repeats: int, dst_rate: int = 48000) -> dict:
    import numpy as np
    import torch

    import flacgpu

    with resident_windows(n_files, frames_each, window) as r:
        enc, ch, bits, per, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.per, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        L, M, taps = flacgpu.resample_ratio(r.rate, dst_rate)
        out_start, out_count = -(-start * L // M), window * L // M  # the output samples that sit in the source window
        out_crops = [(i, out_start, out_count) for i in range(n_files)]
        planar_pad = flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD
        masks = [1 << c for c in range(ch)]
        x_mix = torch.zeros((n_files, ch, window), dtype=torch.float32, device=dev)
        x_res = torch.zeros((n_files, ch, out_count), dtype=torch.float32, device=dev)

        def mix():
            enc.decode_windows_device_mix(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, masks, x_mix.data_ptr(),
                                          [i * ch * window for i in range(n_files)], [ch * window] * n_files, d_wres.data_ptr(),
                                          stream=st)
            return x_mix

        def resample():
            enc.decode_windows_device_resample(*tables, out_crops, flacgpu.SAMPLE_F32, planar_pad, masks, r.rate, dst_rate,
                                               x_res.data_ptr(), [i * ch * out_count for i in range(n_files)],
                                               [ch * out_count] * n_files, d_wres.data_ptr(), stream=st)
            return x_res

        legs = {"resample_f32": (resample, out_count), "mix_f32": (mix, window)}
        for _ in range(warmup):  # the first resample call also builds and uploads the coefficient table
            for fn, n in legs.values():
                fn()
                enc.sync_check(st)
                assert r.results() == [(0, n)] * n_files
        # the expectation from the PCM: the host statement of the rule over channel 0's elements
        check = 4096
        v = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)[:, 0].astype(np.float32) * np.float32(2.0 ** -(bits - 1))
        want = torch.from_numpy(flacgpu.resample_f32_host(v, r.rate, dst_rate, out_start, check))
        got = resample().cpu()
        assert torch.equal(got[0, 0, :check], want) and torch.equal(got[-1, 0, :check], want), "the device differs from the host rule"
        ms = {k: [] for k in legs}
        for _ in range(repeats):  # alternated
            for k, (fn, _) in legs.items():
                ms[k].append(event_ms(fn))
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "src_rate": r.rate,
               "dst_rate": dst_rate, "L": L, "M": M, "taps": taps, "window_samples": window, "window_start": start,
               "out_window_samples": out_count, "out_window_start": out_start, "layout": "f32, planar, padded", "warmup": warmup,
               "repeats": repeats, "outputs_checked_against_the_host_rule": 2 * check}
        for k in legs:
            res[k] = summary(ms[k], keep=True)
        res["resample_f32"]["ms_over_mix"] = res["resample_f32"]["ms_median"] - res["mix_f32"]["ms_median"]
        res["resample_f32"]["x_mix"] = res["resample_f32"]["ms_median"] / res["mix_f32"]["ms_median"]
    return res


def fir_rate(n_files: int, frames_each: int, window: int, repeats: int, taps_list=(64, 512, 4096)) -> dict:
    """The resample leg's files and windows delivered through a causal FIR filter (delay 0) of 64,
    512 and 4096 taps, one call of flacgpu_decode_windows_device_fir, against what a user does today:
    flacgpu_decode_windows_device_as (F32, planar) and then torch, once as conv1d over the crop
    padded with zeros on the left and once as an rfft / irfft product.  Both torch routes read zeros
    where the call reads the file's samples before the crop, so they are compared on the interior
    samples t >= taps - 1 only.  HIP events around each route, three warm calls each, alternated."""
    import numpy as np
    import torch

    import flacgpu

    with resident_windows(n_files, frames_each, window) as r:
        enc, ch, bits, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        planar_pad = flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD
        offs, caps = [i * ch * window for i in range(n_files)], [ch * window] * n_files
        x_as = torch.zeros((n_files, ch, window), dtype=torch.float32, device=dev)
        x_fir = torch.zeros((n_files, ch, window), dtype=torch.float32, device=dev)
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "window_samples": window,
               "window_start": start, "layout": "f32, planar, padded", "delay": 0, "warm_calls": 3, "repeats": repeats,
               "clock": "HIP events around each route on the current stream, the routes alternated",
               "kernel_own_time": "not measured: the call is timed whole (stage 1 decodes taps - 1 samples more than _as)"}

        def deliver():
            enc.decode_windows_device_as(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, x_as.data_ptr(), offs, caps,
                                         d_wres.data_ptr(), stream=st)
            return x_as

        for T in taps_list:
            rng = np.random.RandomState(T)
            h = (rng.uniform(-1.0, 1.0, T) * np.exp(-np.arange(T) / (T / 3.0))).astype(np.float32)
            d_h = torch.from_numpy(h).to(dev)
            w_conv = d_h.flip(0).reshape(1, 1, T).contiguous()
            n_fft = 1 << (window + T - 2).bit_length()
            H = torch.fft.rfft(d_h, n_fft)

            def fir():
                enc.decode_windows_device_fir(*tables, crops, flacgpu.SAMPLE_F32, planar_pad, d_h.data_ptr(), T, [(0, T, 0, 1)],
                                              [0] * n_files, x_fir.data_ptr(), offs, caps, d_wres.data_ptr(), stream=st)
                return x_fir

            def as_then_conv1d():
                x = deliver().reshape(n_files * ch, 1, window)
                return torch.nn.functional.conv1d(torch.nn.functional.pad(x, (T - 1, 0)), w_conv).reshape(n_files, ch, window)

            def as_then_fft():
                return torch.fft.irfft(torch.fft.rfft(deliver(), n_fft) * H, n_fft)[..., :window]

            legs = {"fir_f32": fir, "as_f32_then_conv1d": as_then_conv1d, "as_f32_then_rfft_irfft": as_then_fft}
            for _ in range(3):
                for fn in legs.values():
                    fn()
                    enc.sync_check(st)
                    assert r.results() == [(0, window)] * n_files
            # the expectation from the PCM: the host statement of the rule over channel 0's elements
            check = 2048
            v = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)[:, 0].astype(np.float32) * np.float32(2.0 ** -(bits - 1))
            want = torch.from_numpy(flacgpu.fir_f32_host(v, h, 0, start, check)[0])
            got = fir().clone()
            assert torch.equal(got[0, 0, :check].cpu(), want) and torch.equal(got[-1, 0, :check].cpu(), want), \
                "the device differs from the host rule"
            top = float(got.abs().max())
            diff = {k: float((legs[k]()[..., T - 1:] - got[..., T - 1:]).abs().max()) / top for k in list(legs)[1:]}
            ms = {k: [] for k in legs}
            for _ in range(repeats):  # alternated
                for k, fn in legs.items():
                    ms[k].append(event_ms(fn))
            leg = {k: summary(ms[k], keep=True) for k in legs}
            for k, v_ in diff.items():
                leg[k]["max_interior_difference_over_max_value"] = v_
                leg[k]["x_fir"] = leg[k]["ms_median"] / leg["fir_f32"]["ms_median"]
            leg["outputs_checked_against_the_host_rule"] = 2 * check
            leg["rfft_size"] = n_fft
            res[f"taps_{T}"] = leg
        ms_as = []
        for _ in range(repeats):
            ms_as.append(event_ms(deliver))
        res["as_f32"] = summary(ms_as, keep=True)
    return res


def levels_rate(n_files: int, frames_each: int, window: int, warmup: int, repeats: int) -> dict:
    """The resample leg's files and windows measured, not delivered: flacgpu_levels_windows_device at
    hop 441 and at hop = the window, against flacgpu_decode_windows_device_as (I32, planar) followed
    by torch's abs().amax, sum and double().square().sum over the tensor reshaped to blocks (the short
    last block of hop 441 by a second set of the three reductions over its slice).  Both are timed
    between two events on the stream, alternated; the records of window 0 and of the last window
    are compared with numpy over the PCM before anything is timed."""
    import numpy as np
    import torch

    import flacgpu

    with resident_windows(n_files, frames_each, window) as r:
        enc, ch, bits, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        x = torch.zeros((n_files, ch, window), dtype=torch.int32, device=dev)
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "window_samples": window,
               "window_start": start, "warmup": warmup, "repeats": repeats,
               "comparator": "decode_windows_device_as (I32, planar), then torch abs().amax, sum, double().square().sum a block"}
        v = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)[start:start + window].astype(np.int64)
        for hop in (441, window):
            blocks = (window + hop - 1) // hop
            whole = window // hop
            peak = torch.zeros((n_files, blocks, ch), dtype=torch.int32, device=dev)
            total = torch.zeros((n_files, blocks, ch), dtype=torch.int64, device=dev)
            energy = torch.zeros((n_files, blocks, ch), dtype=torch.float64, device=dev)

            def levels():
                enc.levels_windows_device(*tables, crops, hop, peak.data_ptr(), total.data_ptr(), energy.data_ptr(),
                                          [i * blocks * ch for i in range(n_files)], [blocks * ch] * n_files, d_wres.data_ptr(),
                                          stream=st)

            def as_then_torch():
                enc.decode_windows_device_as(*tables, crops, flacgpu.SAMPLE_I32, flacgpu.DELIVER_PLANAR, x.data_ptr(),
                                             [i * ch * window for i in range(n_files)], [ch * window] * n_files, d_wres.data_ptr(),
                                             stream=st)
                out = []
                for part in ((x[:, :, :whole * hop].reshape(n_files, ch, whole, hop),) +
                             ((x[:, :, whole * hop:].unsqueeze(2),) if blocks > whole else ())):
                    out.append((part.abs().amax(dim=3), part.sum(dim=3), part.double().square().sum(dim=3)))
                return out

            legs = {"levels": levels, "as_i32_then_torch": as_then_torch}
            for _ in range(warmup):
                for fn in legs.values():
                    fn()
                    enc.sync_check(st)
                    assert r.results() == [(0, window)] * n_files
            levels()
            enc.sync_check(st)
            at = np.arange(0, window, hop)
            want = (np.maximum.reduceat(np.abs(v), at, axis=0), np.add.reduceat(v, at, axis=0),
                    np.add.reduceat(v * v, at, axis=0).astype(np.float64))  # 16 bits: the squares' sums are exact in int64
            for i in (0, n_files - 1):
                assert (peak[i].cpu().numpy() == want[0]).all() and (total[i].cpu().numpy() == want[1]).all()
                assert (energy[i].cpu().numpy() == want[2]).all(), "the device differs from the rule"
            ms = {k: [] for k in legs}
            for _ in range(repeats):  # alternated
                for k, fn in legs.items():
                    ms[k].append(event_ms(fn))
            leg = {k: summary(ms[k], keep=True) for k in legs}
            leg["blocks_per_window"] = blocks
            leg["levels"]["x_as_i32_then_torch"] = leg["as_i32_then_torch"]["ms_median"] / leg["levels"]["ms_median"]
            res[f"hop_{hop}"] = leg
    return res


def features_rate(n_files: int, frames_each: int, window: int, warmup: int, repeats: int, dst_rate: int = 48000) -> dict:
    import numpy as np
    import torch

    import flacbank
    import flacgpu

    n_fft, hop, n_mels = 400, 160, 80
    with resident_windows(n_files, frames_each, window) as r:
        enc, ch, bits, dev, pcm, n_each, st, crops = r.enc, r.ch, r.bits, r.dev, r.pcm, r.n_each, r.st, r.crops
        tables, d_wres, start = r.tables, r.d_wres, r.start
        r.positions()
        L, M, _ = flacgpu.resample_ratio(r.rate, dst_rate)
        out_start, out_count = -(-start * L // M), window * L // M
        planar_pad = flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD
        masks = [1 << c for c in range(ch)]
        mel = flacbank.mel_filters(16000, n_fft, n_mels)
        d_mel = torch.from_numpy(mel).to(dev)
        hann = torch.hann_window(n_fft, periodic=True, device=dev)
        v = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)[:, 0].astype(np.float32) * np.float32(2.0 ** -(bits - 1))
        res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "n_fft": n_fft, "hop": hop,
               "rows": n_mels, "layout": "f32, [window, channel, row, frame]", "warmup": warmup, "repeats": repeats}
        for name, src, dst, w_start, w_count in (("own_rate", 0, 0, start, window), ("resampled", r.rate, dst_rate, out_start, out_count)):
            frames = w_count // hop + 1  # torch.stft's count with center=True
            per = ch * n_mels * frames
            wins = [(i, w_start, frames) for i in range(n_files)]
            samp = [(i, w_start, w_count) for i in range(n_files)]
            x_feat = torch.zeros((n_files, ch, n_mels, frames), dtype=torch.float32, device=dev)
            x_pcm = torch.zeros((n_files, ch, w_count), dtype=torch.float32, device=dev)

            def features():
                enc.decode_windows_device_features(*tables, wins, flacgpu.SAMPLE_F32, masks, src, dst, n_fft, hop, mel,
                                                   x_feat.data_ptr(), [i * per for i in range(n_files)], [per] * n_files,
                                                   d_wres.data_ptr(), stream=st)
                return x_feat

            def deliver_then_torch():
                to = (x_pcm.data_ptr(), [i * ch * w_count for i in range(n_files)], [ch * w_count] * n_files, d_wres.data_ptr())
                if src:
                    enc.decode_windows_device_resample(*tables, samp, flacgpu.SAMPLE_F32, planar_pad, masks, src, dst, *to, stream=st)
                else:
                    enc.decode_windows_device_mix(*tables, samp, flacgpu.SAMPLE_F32, planar_pad, masks, *to, stream=st)
                z = torch.stft(x_pcm.reshape(n_files * ch, w_count), n_fft, hop, window=hann, center=True, pad_mode="constant",
                               return_complex=True)
                return torch.matmul(d_mel, z.real * z.real + z.imag * z.imag).reshape(n_files, ch, n_mels, frames)

            legs = {"features_f32": features, "deliver_then_stft_matmul": deliver_then_torch}
            for _ in range(warmup):  # the first features call also builds and uploads the two tables
                for fn in legs.values():
                    fn()
                    enc.sync_check(st)
            got, other = features().cpu(), deliver_then_torch().cpu()
            check = 8
            sig = v if not src else flacgpu.resample_f32_host(v, src, dst)
            want, _ = flacgpu.features_f32_host(sig, n_fft, hop, w_start, check, mel)
            assert torch.equal(got[0, 0, :, :check], torch.from_numpy(want)) and torch.equal(got[-1, 0, :, :check], torch.from_numpy(want)), \
                "the device differs from the host rule"
            inner = slice(2, frames - 3)  # the crop's edge frames differ by design: the stream's samples against zero padding
            rel = ((got[..., inner] - other[..., inner]).abs().max() / other[..., inner].abs().max()).item()
            assert rel < 1e-4, rel
            ms = {k: [] for k in legs}
            for _ in range(repeats):  # alternated
                for k, fn in legs.items():
                    ms[k].append(event_ms(fn))
            row = {"src_rate": src or r.rate, "dst_rate": dst or r.rate, "window_start": w_start, "window_samples": w_count,
                   "frames": frames, "frames_checked_against_the_host_rule": 2 * check, "interior_max_rel_diff_of_the_two_paths": rel}
            for k in legs:
                row[k] = summary(ms[k], keep=True)
            row["features_f32"]["x_deliver_then_stft_matmul"] = (row["deliver_then_stft_matmul"]["ms_median"] /
                                                                 row["features_f32"]["ms_median"])
            res[name] = row
    return res


def write_rate(n_files: int, frames_each: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacbank
    import flacgpu
    import synth

    ch, bits, rate, _ = PRESETS["c2"]
    dev = torch.device("cuda", 0)
    unit = synth.synth_pcm(64 * 4096, ch, bits, rate)
    n_each = frames_each * 4096
    pcm = (unit * ((frames_each + 63) // 64))[: n_each * ch * (bits // 8)]
    ints = np.frombuffer(pcm, dtype=np.int16).reshape(n_each, ch)
    x = torch.from_numpy(np.ascontiguousarray(ints.T).astype(np.float32) * np.float32(2.0 ** -(bits - 1))).to(dev)
    tensors = [x.clone() for _ in range(n_files)]  # [C, T] float32 on the device: what a data set of tensors is
    torch.cuda.synchronize(dev)

    def from_tensors():
        t = time.perf_counter()
        b = flacbank.FlacBank.from_tensors(tensors, rate, bits=bits)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t, b

    def host_detour():
        """The route without from_tensors: scale, round and cast in torch, to the host, encode_files, FlacBank(files)."""
        t = time.perf_counter()
        top = float(1 << (bits - 1))
        pcms = [(v * top).round().clamp(-top, top - 1).to(torch.int16).t().contiguous().cpu().numpy().tobytes() for v in tensors]
        with flacgpu.Encoder(ch, bits, rate, device=0, max_frames=n_files * frames_each) as enc:
            files = enc.encode_files(pcms)
        b = flacbank.FlacBank(files)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t, b, files

    _, a = from_tensors()  # one warm call each: the allocations, the library's first use
    _, b, files = host_detour()
    assert a.clipped == [0] * n_files and a.samples == b.samples == [n_each] * n_files
    assert a.file_bytes(0) == files[0] and a.file_bytes(n_files - 1) == files[-1], "the two routes write different files"
    (xa, _), (xb, _) = a.crops([0, n_files - 1], [1234, 99], 65536), b.crops([0, n_files - 1], [1234, 99], 65536)
    assert torch.equal(xa, xb) and torch.equal(xa[0], x[:, 1234:1234 + 65536]), "a crop differs from the tensor it was built from"
    flac_bytes = a.compressed_bytes
    a.close()
    b.close()
    s_new, s_old = [], []
    for _ in range(repeats):  # alternated
        dt, a = from_tensors()
        a.close()
        s_new.append(dt)
        dt, b, _ = host_detour()
        b.close()
        s_old.append(dt)
    total = n_files * n_each
    res = {"files": n_files, "frames_per_file": frames_each, "channels": ch, "bits": bits, "dtype": "float32",
           "tensor_bytes": n_files * x.numel() * 4, "pcm_bytes": n_files * len(pcm), "flac_bytes": flac_bytes, "repeats": repeats,
           "clock": "wall, the device synchronised at both ends; one warm call of each route before the timed ones",
           "from_tensors": {"seconds_median": statistics.median(s_new), "seconds": s_new,
                            "msamples_per_s": total / statistics.median(s_new) / 1e6},
           "host_detour": {"seconds_median": statistics.median(s_old), "seconds": s_old,
                           "msamples_per_s": total / statistics.median(s_old) / 1e6}}
    res["from_tensors"]["x_host_detour"] = res["host_detour"]["seconds_median"] / res["from_tensors"]["seconds_median"]
    return res


def bigblock_rate(blocks, n_streams: int, warmup: int, repeats: int) -> dict:
    import numpy as np
    import torch

    import flacgpu
    import oracle_ref
    import synth

    ch, bits, rate = 2, 16, 44100
    per = ch * (bits // 8)
    dev = torch.device("cuda", 0)
    n = 1 << 20
    pcm = synth.synth_pcm(n, ch, bits, rate)
    res = {"channels": ch, "bits": bits, "streams": n_streams, "samples_per_stream": n, "library": flacgpu.LIB_PATH, "rows": {}}
    for block in blocks:
        body, sizes, _ = oracle_ref.encode_stream(pcm, ch, bits, rate, block)
        frames = len(sizes)
        offs, at = [], 0
        for _ in range(n_streams):
            offs.append(at)
            at += (len(body) + 63) & ~63
        host = np.zeros(at + 16, dtype=np.uint8)
        for o in offs:
            host[o:o + len(body)] = np.frombuffer(body, dtype=np.uint8)
        d_buf = torch.from_numpy(host).to(dev)
        d_all = torch.zeros(n_streams * len(pcm), dtype=torch.uint8, device=dev)
        d_sres = torch.zeros(32 * n_streams, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        lens, pcm_offs, caps = [len(body)] * n_streams, [i * len(pcm) for i in range(n_streams)], [len(pcm)] * n_streams
        with flacgpu.Decoder(ch, bits, rate, device=0, max_frames=n_streams * frames, block_size=block) as d:
            def run():
                d.decode_streams_device(d_buf.data_ptr(), offs, lens, d_all.data_ptr(), pcm_offs, caps, d_sres.data_ptr(),
                                        stream_bits=[bits] * n_streams, stream_rates=[rate] * n_streams, stream=st)

            for _ in range(warmup):
                run()
            d.sync_check(st)
            sres = (flacgpu.StreamResult * n_streams).from_buffer_copy(d_sres.cpu().numpy().tobytes())
            assert [(r.n_frames, r.n_samples, r.bad_frames) for r in sres] == [(frames, n, 0)] * n_streams
            got = d_all.cpu().numpy().tobytes()
            assert got[:len(pcm)] == pcm and got[-len(pcm):] == pcm, "decoded PCM differs from the input"
            ms = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            d.set_timing(True)
            d.reset_timing()
            for _ in range(repeats):
                run()
            d.sync_check(st)
            kernels = {name: d.kernel_time(k)[1] / repeats for name, k in
                       (("index_ms", flacgpu.K_INDEX), ("parse_ms", flacgpu.K_DEC_PARSE), ("recon_ms", flacgpu.K_DEC_RECON))}
            d.set_timing(False)
        med = statistics.median(ms)
        total = n_streams * n
        res["rows"][str(block)] = dict({"frames": n_streams * frames, "flac_bytes": n_streams * len(body), "ms_median": med,
                                        "ms_min": min(ms), "ms_max": max(ms), "ms": ms, "msamples_per_s": total / med / 1e3,
                                        "recon_ns_per_sample": kernels["recon_ms"] * 1e6 / total,
                                        "parse_ns_per_sample": kernels["parse_ms"] * 1e6 / total}, **kernels)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dec_rate.json"))
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--cpu-frames", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--legs", choices=("all", "decode", "index", "files", "windows", "deliver", "bigblock", "mix", "resample", "features", "write", "downmix", "levels", "fir"),
                    default="all")
    ap.add_argument("--write-out", default=os.path.join(ROOT, "profiles", "bank_write_rate.json"))
    ap.add_argument("--downmix-out", default=os.path.join(ROOT, "profiles", "decode_downmix_rate.json"))
    ap.add_argument("--levels-out", default=os.path.join(ROOT, "profiles", "decode_levels_rate.json"))
    ap.add_argument("--fir-out", default=os.path.join(ROOT, "profiles", "decode_fir_rate.json"))
    ap.add_argument("--resample-out", default=os.path.join(ROOT, "profiles", "decode_resample_rate.json"))
    ap.add_argument("--features-out", default=os.path.join(ROOT, "profiles", "decode_features_rate.json"))
    ap.add_argument("--mix-out", default=os.path.join(ROOT, "profiles", "decode_mix_rate.json"))
    ap.add_argument("--bigblock-out", default=os.path.join(ROOT, "profiles", "decode_bigblock_rate.json"))
    ap.add_argument("--blocks", default="4096,4608,16384")
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--deliver-out", default=os.path.join(ROOT, "profiles", "decode_deliver_rate.json"))
    ap.add_argument("--windows-out", default=os.path.join(ROOT, "profiles", "decode_windows_rate.json"))
    ap.add_argument("--window", type=int, default=65536)
    ap.add_argument("--files-out", default=os.path.join(ROOT, "profiles", "decode_files_rate.json"))
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--index-out", default=os.path.join(ROOT, "profiles", "index_rate.json"))
    a = ap.parse_args()
    if a.legs == "bigblock":  # opt-in: `all` leaves it out
        br = bigblock_rate([int(b) for b in a.blocks.split(",")], a.streams, a.warmup, a.repeats)
        print(json.dumps({"bigblock": br}), flush=True)
        with open(a.bigblock_out, "w") as f:
            json.dump(br, f, indent=1)
            f.write("\n")
        return
    if a.legs == "write":  # opt-in: `all` leaves it out
        wr = {"c2": write_rate(a.files, a.frames // a.files, a.repeats)}
        print(json.dumps({"write": wr}), flush=True)
        with open(a.write_out, "w") as f:
            json.dump(wr, f, indent=1)
            f.write("\n")
        return
    if a.legs == "downmix":  # opt-in: `all` leaves it out
        dm = {"c6_16": downmix_rate(a.files, a.frames // a.files, a.window, a.repeats)}
        print(json.dumps({"downmix": dm}), flush=True)
        with open(a.downmix_out, "w") as f:
            json.dump(dm, f, indent=1)
            f.write("\n")
        return
    if a.legs == "mix":  # opt-in: `all` leaves it out
        mr = {"c2": mix_rate(a.files, a.frames // a.files, a.window, a.warmup, a.repeats)}
        print(json.dumps({"mix": mr}), flush=True)
        with open(a.mix_out, "w") as f:
            json.dump(mr, f, indent=1)
            f.write("\n")
        return
    if a.legs == "levels":  # opt-in: `all` leaves it out
        lr = {"c2": levels_rate(a.files, a.frames // a.files, a.window, a.warmup, a.repeats)}
        print(json.dumps({"levels": lr}), flush=True)
        with open(a.levels_out, "w") as f:
            json.dump(lr, f, indent=1)
        return
    if a.legs == "fir":  # opt-in: `all` leaves it out
        fr = {"c2": fir_rate(a.files, a.frames // a.files, a.window, a.repeats)}
        print(json.dumps({"fir": fr}), flush=True)
        with open(a.fir_out, "w") as f:
            json.dump(fr, f, indent=1)
            f.write("\n")
        return
    if a.legs == "resample":  # opt-in: `all` leaves it out
        rr = {"c2": resample_rate(a.files, a.frames // a.files, a.window, a.warmup, a.repeats)}
        print(json.dumps({"resample": rr}), flush=True)
        with open(a.resample_out, "w") as f:
            json.dump(rr, f, indent=1)
            f.write("\n")
        return
    if a.legs == "features":  # opt-in: `all` leaves it out
        fr = {"c2": features_rate(a.files, a.frames // a.files, a.window, a.warmup, a.repeats)}
        print(json.dumps({"features": fr}), flush=True)
        with open(a.features_out, "w") as f:
            json.dump(fr, f, indent=1)
            f.write("\n")
        return
    if a.legs == "deliver":  # opt-in: `all` leaves it out
        dr = {"c2": deliver_rate(a.files, a.frames // a.files, a.window, a.warmup, a.repeats)}
        print(json.dumps({"deliver": dr}), flush=True)
        with open(a.deliver_out, "w") as f:
            json.dump(dr, f, indent=1)
            f.write("\n")
        return
    if a.legs in ("all", "windows"):
        wr = {"c2": windows_rate(a.files, a.frames // a.files, a.window, a.warmup, a.repeats)}
        print(json.dumps({"windows": wr}), flush=True)
        with open(a.windows_out, "w") as f:
            json.dump(wr, f, indent=1)
            f.write("\n")
        if a.legs == "windows":
            return
    if a.legs in ("all", "files"):
        fr = {"c2": files_rate(a.files, a.frames // a.files, a.warmup, a.repeats)}
        print(json.dumps({"files": fr}), flush=True)
        with open(a.files_out, "w") as f:
            json.dump(fr, f, indent=1)
            f.write("\n")
        if a.legs == "files":
            return
    if a.legs != "decode":
        idx = {"c2": index_rate(a.frames, a.warmup, a.repeats)}
        print(json.dumps({"index": idx}), flush=True)
        with open(a.index_out, "w") as f:
            json.dump(idx, f, indent=1)
            f.write("\n")
        if a.legs == "index":
            return
    doc = {"cpu_oracle_fast_c2": cpu_rate(a.cpu_frames)}
    print(json.dumps({"cpu": doc["cpu_oracle_fast_c2"]}), flush=True)
    for name in ("c2", "c5"):
        frames = a.frames if name == "c2" else a.frames // 2  # c5's PCM is twice as wide
        doc[name] = gpu_rate(name, frames, a.warmup, a.repeats)
        for mode in ("verify", "output"):
            doc[name][mode]["x_cpu_core"] = doc[name][mode]["msamples_per_s"] / doc["cpu_oracle_fast_c2"]["msamples_per_s"]
        print(json.dumps({name: doc[name]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
