"""Contexts opened, used and closed over and over: what a context owns goes when it is closed.

A context holds its device memory, streams and events in owners (zig-flac_amd/csrc/fg_own.hpp) and
flacgpu_close only deletes it, so a buffer that some call allocates lazily is either a member of
one of the context's parts or a leak.  Each of the four kinds of context -- an encoder at 2 x 16
bits, one at 2 x 24 bits with LPC, one at 8 x 24 bits (the geometry that analyses and packs in
channel halves) and a decode-only context for blocks of up to 8192 -- goes through CYCLES cycles of
open / one call of every family that allocates lazily / close:

  encode with decision records and kernel timing on; an MD5 update on the device engine; a plan of
  more frames than the context holds, so that the plan owns its descriptors, encoded with its MD5;
  decode_frames, decode_files and decode_files_windows; and one resampled window call over resident
  tables, so that a coefficient table is cached.

(The decode-only context makes the decode calls, and every encode entry point must refuse it.)
Frames have 256 samples, a stream has three, a context holds four: the plan, decode_files and the
window calls all pass the context's frame count.

The last cycle's outputs equal the first cycle's byte for byte.  The device's free memory after the
last cycle is lower than after the second by less than 4 times the context's own footprint,
pcm_cap + out_cap of flacgpu_open for the configuration: the PCM of max_frames full frames and
their frame images.  A leak of the context's buffers would show as about CYCLES - 2 = 22 times that
footprint; the margin of 4 is room for the other tenants of the card, not a measurement.  Every
device tensor of the test is allocated before the first cycle, so nothing but the library allocates
between the two readings."""
import ctypes
import hashlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

RATE, DST_RATE, BLOCK, FRAMES, MAX_FRAMES, CYCLES = 44100, 48000, 256, 3, 4, 24
N = BLOCK * FRAMES  # samples of a stream
# kind: (channels, bits, LPC order, max_block of a decode-only context or 0)
KINDS = {"enc_2ch16": (2, 16, 0, 0), "enc_2ch24_lpc": (2, 24, 8, 0), "enc_8ch24_split": (8, 24, 0, 0),
         "dec_2ch16_block8192": (2, 16, 0, 8192)}
WINDOWS = [(0, 10, 300), (1, 0, 200), (1, 500, 300)]  # (stream, start, count) in samples at DST_RATE, inside the streams
# flacgpu_get_config on the decode-only context, as the library returned it before the context was
# split into parts: the stream, block_size = max_block, the encode options zero
DECODER_CONFIG = (RATE, 8192, 2, 16, 0, 0, 0, 0)


def image_bytes(lib, cfg):
    """What flacgpu_open keeps for one frame of its output: the frame bound and 16 bytes, in 16-byte units."""
    return (lib.flacgpu_frame_bound_bytes(ctypes.byref(cfg)) + 16 + 15) // 16 * 16


def footprint(lib, cfg, max_frames):
    """pcm_cap + out_cap of flacgpu_open(cfg, max_frames)."""
    per = cfg.channels * (cfg.bits_per_sample // 8)
    return max_frames * 4096 * per + 64 + max_frames * image_bytes(lib, cfg)


class Arena:
    """Every device tensor the cycles of one kind use, allocated once."""

    def __init__(self, channels, bits, pcms, image):
        import torch

        dev = torch.device("cuda", 0)
        per = channels * (bits // 8)
        self.torch, self.st = torch, torch.cuda.current_stream(dev).cuda_stream
        self.offs = [0, (len(pcms[0]) + 63) // 64 * 64]
        blob = bytearray(self.offs[1] + len(pcms[1]) + 64)
        for o, p in zip(self.offs, pcms):
            blob[o:o + len(p)] = p
        self.d_pcm = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
        nf = 2 * FRAMES
        self.out_cap = nf * image
        self.d_out = torch.zeros(self.out_cap, dtype=torch.uint8, device=dev)
        self.d_fb = torch.zeros(nf, dtype=torch.int32, device=dev)
        self.d_off = torch.zeros(nf, dtype=torch.int64, device=dev)
        self.d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
        self.d_md5 = torch.zeros(32, dtype=torch.uint8, device=dev)
        # the resident streams of the window call: two bare runs of frames, their tables and positions
        self.blob_cap = 2 * (N * per + 4096)
        self.entries = self.blob_cap // 8 + 2
        self.d_blob = torch.zeros(self.blob_cap, dtype=torch.uint8, device=dev)
        self.d_toff = torch.zeros(self.entries, dtype=torch.int64, device=dev)
        self.d_tfb = torch.zeros(self.entries, dtype=torch.int32, device=dev)
        self.d_pos = torch.zeros(self.entries, dtype=torch.int64, device=dev)
        self.d_ires = torch.zeros(2 * 16, dtype=torch.uint8, device=dev)
        self.d_totals = torch.zeros(2, dtype=torch.int64, device=dev)
        self.d_wres = torch.zeros(32 * len(WINDOWS), dtype=torch.uint8, device=dev)
        self.d_wout = torch.zeros(sum(w[2] for w in WINDOWS) * channels, dtype=torch.float32, device=dev)

    def host(self, t):
        return t.cpu().numpy().tobytes()


def decode_calls(d, a, frames, sizes, flacs, pcms, out):
    """The decode families on the open context d; their outputs are appended to `out`."""
    import flacgpu

    got, res = d.decode_frames(frames, sizes)
    assert got == pcms[0] and [r.status for r in res] == [0] * FRAMES
    files = d.decode_files(flacs)
    assert files == [(0, pcms[0], True), (0, pcms[1], True)]
    per = d.channels * d.bytes_per_sample
    wins = d.decode_files_windows(flacs, [(0, 5, 500), (1, 300, 1000)])
    assert wins == [(0, pcms[0][5 * per:505 * per], b""), (0, pcms[1][300 * per:], b"")]
    # the resampled window call: the files' frames resident, indexed, their positions scanned
    bare = [f[flacgpu.flac_index(f)[1]:] for f in flacs]
    offs = [0, (len(bare[0]) + 63) // 64 * 64]
    assert offs[1] + len(bare[1]) + 16 <= a.blob_cap
    caps = [len(b) // 8 + 1 for b in bare]
    first = [0, caps[0]]
    assert sum(caps) <= a.entries
    for o, b in zip(offs, bare):
        a.d_blob[o:o + len(b)].copy_(a.torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()))
    tables = (a.d_blob.data_ptr(), first, a.d_toff.data_ptr(), a.d_tfb.data_ptr(), a.d_ires.data_ptr())
    d.flac_index_streams_device(a.d_blob.data_ptr(), offs, [len(b) for b in bare], first, caps, *tables[2:],
                                stream_bits=[d.bits] * 2, stream_rates=[RATE] * 2, stream=a.st)
    d.flac_positions_streams_device(a.d_blob.data_ptr(), first, caps, *tables[2:], a.d_pos.data_ptr(), a.d_totals.data_ptr(),
                                    stream_bits=[d.bits] * 2, stream_rates=[RATE] * 2, stream=a.st)
    a.d_wout.zero_()
    counts = [w[2] * d.channels for w in WINDOWS]
    d.decode_windows_device_resample(*tables, a.d_pos.data_ptr(), a.d_totals.data_ptr(), WINDOWS, flacgpu.SAMPLE_F32, 0, None,
                                     RATE, DST_RATE, a.d_wout.data_ptr(), [sum(counts[:w]) for w in range(len(counts))],
                                     counts, a.d_wres.data_ptr(), stream=a.st)
    d.sync_check(a.st)
    wres = list((flacgpu.WindowResult * len(WINDOWS)).from_buffer_copy(a.host(a.d_wres)))
    assert [(r.status, r.n_samples) for r in wres] == [(0, w[2]) for w in WINDOWS]
    out += [got, b"".join(f[1] for f in files), b"".join(w[1] for w in wins), a.host(a.d_wres), a.host(a.d_wout)]


def encoder_cycle(kind, a, pcms):
    import flacgpu

    channels, bits, lpc, _ = KINDS[kind]
    out = []
    with flacgpu.Encoder(channels, bits, RATE, device=0, max_frames=MAX_FRAMES, block_size=BLOCK, lpc_order=lpc) as enc:
        enc.set_records(True)
        enc.set_timing(True)
        frames, sizes = enc.encode_frames(pcms[0])
        recs = enc.records()
        assert len(sizes) == len(recs) == FRAMES and sum(sizes) == len(frames)
        assert enc.kernel_time(flacgpu.K_PACK)[0] > 0
        out += [frames, b"".join(bytes(r) for r in recs)]
        enc.set_records(False)
        enc.set_md5_engine(flacgpu.MD5_DEVICE)
        out.append(enc.md5(pcms[1]))
        enc.set_md5_engine(flacgpu.MD5_HOST)
        assert out[-1] == enc.md5(pcms[1])
        plan = enc.plan(a.offs, [N, N])
        assert plan.n_frames == 2 * FRAMES > MAX_FRAMES and plan.out_bound == a.out_cap
        enc.encode_plan_device(plan, a.d_pcm.data_ptr(), a.d_out.data_ptr(), a.out_cap, a.d_fb.data_ptr(), a.d_off.data_ptr(),
                               a.d_tot.data_ptr(), d_md5=a.d_md5.data_ptr(), stream=a.st)
        enc.sync_check(a.st)
        plan.close()
        total = int(a.d_tot[0].item())
        planned = a.host(a.d_out)[:total]
        assert planned[:len(frames)] == frames and a.host(a.d_md5)[16:] == out[2]
        out += [planned, a.host(a.d_fb), a.host(a.d_md5)]
        flacs = enc.encode_files(pcms)
        out += flacs
        decode_calls(enc, a, frames, sizes, flacs, pcms, out)
    return out


def decoder_cycle(kind, a, pcms, frames, sizes, flacs):
    import flacgpu

    channels, bits, _, max_block = KINDS[kind]
    out = []
    with flacgpu.Decoder(channels, bits, RATE, device=0, max_frames=MAX_FRAMES, block_size=max_block) as d:
        cfg = flacgpu.Config()
        assert d.lib.flacgpu_get_config(d.ctx, ctypes.byref(cfg)) == 0
        assert tuple(getattr(cfg, f) for f, _ in flacgpu.Config._fields_) == DECODER_CONFIG
        planes = np.zeros((channels, BLOCK), dtype=np.int32)
        null = ctypes.c_void_p()
        refused = [lambda: d.encode_frames(pcms[0]), lambda: d.write_frame(planes, 0), lambda: d.encode_file(pcms[0]),
                   lambda: d.encode_files(pcms), lambda: d.set_md5_engine(flacgpu.MD5_DEVICE), lambda: d.plan([0], [N]),
                   lambda: d.set_records(True), lambda: d.set_overlap(1),
                   lambda: flacgpu._check(d.lib.flacgpu_encode_plan_device_ex(
                       d.ctx, null, null, null, 0, null, null, null, null, null, null, null), "encode_plan_device_ex"),
                   lambda: flacgpu._check(d.lib.flacgpu_encode_plan_device(d.ctx, null, null, null, 0, null, null, null, null,
                                                                           null), "encode_plan_device"),
                   lambda: flacgpu._check(d.lib.flacgpu_verify_plan_device(d.ctx, null, null, null, null, null, null, null,
                                                                           null), "verify_plan_device")]
        for k, call in enumerate(refused):
            with pytest.raises(flacgpu.FlacGpuError) as e:
                call()
            assert e.value.code == -1, k
        assert d.records() == [] and d.md5(pcms[0]) == hashlib.md5(pcms[0]).digest()
        decode_calls(d, a, frames, sizes, flacs, pcms, out)
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_cycles_release_what_they_allocate(kind):
    import flacgpu
    import torch

    channels, bits, lpc, max_block = KINDS[kind]
    lib = flacgpu.load_library()
    pcms = [synth.synth_pcm(N, channels, bits, RATE, stream=40 + i) for i in range(2)]
    cfg = flacgpu.Config(*DECODER_CONFIG) if max_block else flacgpu.Config(RATE, BLOCK, channels, bits, 1, 8, 30, lpc)
    own = footprint(lib, cfg, MAX_FRAMES)
    arena = Arena(channels, bits, pcms, image_bytes(lib, cfg))
    if max_block:
        with flacgpu.Encoder(channels, bits, RATE, device=0, max_frames=MAX_FRAMES, block_size=BLOCK) as enc:
            frames, sizes = enc.encode_frames(pcms[0])
            flacs = enc.encode_files(pcms)
        cycle = lambda: decoder_cycle(kind, arena, pcms, frames, sizes, flacs)  # noqa: E731
    else:
        cycle = lambda: encoder_cycle(kind, arena, pcms)  # noqa: E731
    free = {}
    for i in range(1, CYCLES + 1):
        out = cycle()
        if i == 1:
            first = out
        if i in (2, CYCLES):
            torch.cuda.synchronize()
            free[i] = torch.cuda.mem_get_info(0)[0]
    assert len(out) == len(first) and all(x == y for x, y in zip(out, first))
    lost = free[2] - free[CYCLES]
    print(f"{kind}: footprint {own} bytes, free memory after cycle 2 minus after cycle {CYCLES}: {lost} bytes")
    assert lost < 4 * own
