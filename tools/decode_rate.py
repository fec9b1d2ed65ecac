#!/usr/bin/env python3
"""Decode / verify rate of the device FLAC frame decoder beside the CPU verifier decoder.

CPU figure first (before anything initialises the GPU): fdec_frames_to_pcm of liboracle_fast on
one core over the C2 synthetic stream.  Then, per preset (c2: 2 x 16-bit fixed prediction; c5:
2 x 32-bit, LPC 12), a batch of frames encoded on the GPU and left in HBM is decoded by
flacgpu_decode_frames_device in verify mode (compare with the PCM) and in output mode (write the
PCM): HIP events around the call, warm-up, repeats, the median; the parse and reconstruct kernel
times from flacgpu_kernel_time in a pass of their own.  Writes one JSON document.

    python tools/decode_rate.py --out profiles/dec_rate.json
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dec_rate.json"))
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--cpu-frames", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
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
