"""The device FLAC frame decoder / verifier (zig-flac_amd/csrc/fg_dec.hip) on the GPU.

Round trips of CPU-encoded streams (the expected PCM is the input, cross-checked with the CPU
verifier decoder), hand-built frames no encoder here writes, per-frame statuses of corrupted
frames inside batches of good ones (only input the sanitizer run of test_decode_host.py's host
program has decoded first, and the statuses must equal that program's), the host-buffer decode
in several chunks of max_frames, the verify of a plan encode, and the whole-file decode."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import decode_cases as dc  # noqa: E402
import make_golden  # noqa: E402
import oracle_ref  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _decoder(ch, bits, rate=44100, max_frames=192, block=4096):
    import flacgpu

    return flacgpu.Decoder(ch, bits, rate, device=0, max_frames=max_frames, block_size=block)


def _results(t, n):
    import flacgpu

    raw = t.cpu().numpy().tobytes()
    return list((flacgpu.DecodeResult * n).from_buffer_copy(raw[: 32 * n]))


def device_decode(d, frames, pcm_offsets=None, out_bytes=0, expect=None, guard=0, write=True):
    """flacgpu_decode_frames_device over a list of frames -> (output buffer incl. guards, results,
    bad count).  pcm_offsets None: consecutive blocks of one stream."""
    torch, dev = _torch()
    n = len(frames)
    offs = np.cumsum([0] + [len(f) for f in frames])[:-1].astype(np.int64)
    d_fr = torch.from_numpy(np.frombuffer(b"".join(frames) + bytes(16), dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(offs).to(dev)
    d_fb = torch.from_numpy(np.array([len(f) for f in frames], dtype=np.int32)).to(dev)
    d_po = torch.from_numpy(np.array(pcm_offsets, dtype=np.int64)).to(dev) if pcm_offsets is not None else None
    d_out = torch.full((guard + max(out_bytes, 1) + guard,), 0xA5, dtype=torch.uint8, device=dev)
    d_exp = torch.from_numpy(np.frombuffer(expect, dtype=np.uint8).copy()).to(dev) if expect is not None else None
    d_res = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_bad = torch.full((1,), 77, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    d.decode_frames_device(d_fr.data_ptr(), d_off.data_ptr(), d_fb.data_ptr(), n, d_res.data_ptr(), d_bad.data_ptr(),
                           d_pcm_offsets=d_po.data_ptr() if d_po is not None else None,
                           d_pcm_out=d_out.data_ptr() + guard if write else None, pcm_cap=out_bytes,
                           d_pcm_expect=d_exp.data_ptr() if d_exp is not None else None, stream=st)
    d.sync_check(st)
    return d_out.cpu().numpy().tobytes(), _results(d_res, n), int(d_bad.item())


def _split(stream, sizes):
    out, pos = [], 0
    for n in sizes:
        out.append(stream[pos:pos + n])
        pos += n
    return out


def _round_trip(ch, bits, n, rate=44100, block=4096, first_frame=0, stream=0, **kw):
    pcm = synth.synth_pcm(n, ch, bits, rate, stream=stream)
    fr, sizes, _ = oracle_ref.encode_stream(pcm, ch, bits, rate, block, first_frame=first_frame, **kw)
    ref, _ = oracle_ref.decode_frames(fr, ch, bits, rate, n, first_number=first_frame)
    assert ref == pcm
    with _decoder(ch, bits, rate, block=block) as d:
        got, res = d.decode_frames(fr, sizes)
    assert [r.status for r in res] == [0] * len(sizes)
    assert [r.number for r in res] == [first_frame + i for i in range(len(sizes))]
    assert [r.block_size for r in res] == [min(block, n - i * block) for i in range(len(sizes))]
    assert got == pcm


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_round_trip_layouts(ch, bits):
    _round_trip(ch, bits, 2 * 4096 + 1234)


@pytest.mark.parametrize("bits,kw", [(16, {"stereo": False}), (16, {"part_order": 0}), (16, {"part_order": 8}),
                                     (16, {"param": 2}), (24, {"param": 2}), (24, {"lpc": 8}), (24, {"lpc": 12}),
                                     (32, {"lpc": 8}), (32, {"lpc": 12})],
                         ids=lambda v: str(v).replace(" ", ""))
def test_round_trip_options(bits, kw):
    _round_trip(2, bits, 2 * 4096 + 777, stream=3, **kw)


def test_round_trip_block_1152():
    _round_trip(2, 16, 3 * 1152 + 100, block=1152)
    _round_trip(3, 8, 2 * 1152 + 7, block=1152)


def test_round_trip_tails_and_frame_numbers():
    for tail in (1, 2, 5, 63, 64, 65, 192, 4095):
        _round_trip(2, 16, 4096 + tail, stream=tail)
    for first in (0, 127, 128, 2 ** 31 + 5, 2 ** 36 - 5):
        _round_trip(1, 16, 4096 + 100, first_frame=first)


def test_specials_golden():
    c = next(c for c in dc.MANIFEST if c["name"] == "specials")
    frames, raw = dc.golden_frames(c)
    pcm = make_golden.make_pcm(c["name"], c["channels"], c["bits"], c["rate"], c["n_samples"], c["stream_seed"])
    with _decoder(c["channels"], c["bits"], c["rate"], block=c["block"]) as d:
        got, res = d.decode_frames(raw, c["frame_bytes"])
    assert [r.status for r in res] == [0] * len(frames) and got == pcm


def test_full_scale_32_bit():
    rng = np.random.default_rng(5)
    x = rng.integers(-2 ** 31, 2 ** 31, size=(4096 + 300) * 2, dtype=np.int64).astype(np.int32)
    x[:64] = 2 ** 31 - 1
    x[64:128] = -2 ** 31
    x[128:256:2] = 2 ** 31 - 1  # left at +full scale, right at -full scale: a 33-bit side channel
    x[129:256:2] = -2 ** 31
    pcm = x.tobytes()
    fr, sizes, _ = oracle_ref.encode_stream(pcm, 2, 32, 192000)
    with _decoder(2, 32, 192000) as d:
        got, res = d.decode_frames(fr, sizes)
    assert [r.status for r in res] == [0, 0] and got == pcm


def test_frame_counts_and_guard_bands():
    ch, bits, block = 2, 16, 256
    n = 130 * block
    pcm = synth.synth_pcm(n, ch, bits, 44100, stream=9)
    fr, sizes, _ = oracle_ref.encode_stream(pcm, ch, bits, 44100, block)
    frames = _split(fr, sizes)
    per = block * ch * 2
    with _decoder(ch, bits, block=block) as d:
        for k in (1, 63, 64, 65, 130):
            buf, res, bad = device_decode(d, frames[:k], out_bytes=k * per, guard=4096)
            assert bad == 0 and [r.status for r in res] == [0] * k
            assert buf[4096:4096 + k * per] == pcm[: k * per]
            assert buf[:4096] == b"\xa5" * 4096 and buf[4096 + k * per:] == b"\xa5" * 4096
        # a buffer one byte too small for the last frame: RANGE, and nothing of it written
        buf, res, bad = device_decode(d, frames[:3], out_bytes=3 * per - 1, guard=4096)
        assert [r.status for r in res] == [0, 0, dc.STATUS["RANGE"]] and bad == 1
        assert buf[4096:4096 + 2 * per] == pcm[: 2 * per] and set(buf[4096 + 2 * per:]) == {0xA5}
    # odd frame regions (3 channels x 1 byte x 1151 samples): every 16-byte unit edge case
    pcm = synth.synth_pcm(5 * 1151, 3, 8, 44100, stream=2)
    fr, sizes, _ = oracle_ref.encode_stream(pcm, 3, 8, 44100, 1151)
    with _decoder(3, 8, block=1151) as d:
        buf, res, bad = device_decode(d, _split(fr, sizes), out_bytes=len(pcm), guard=4099)
        assert bad == 0 and buf[4099:4099 + len(pcm)] == pcm
        assert set(buf[:4099]) == {0xA5} and set(buf[4099 + len(pcm):]) == {0xA5}


def test_hand_built_frames():
    for h in dc.hand_built():
        want = dc.oracle_pcm(h["frame"], h["channels"], h["bits"], 44100, h["number"])
        with _decoder(h["channels"], h["bits"], max_frames=4) as d:
            got, res = d.decode_frames(h["frame"], [len(h["frame"])])
        assert res[0].status == 0 and res[0].number == h["number"] and res[0].block_size == h["block"], h["name"]
        assert got == h["pcm"], h["name"]  # the samples the frame was written from
        assert got == want, h["name"]


_CHUNKED = {}


def _chunked_stream():
    """2 channels, 16 bits, four frames with a short last one: (pcm, frames, sizes), encoded once."""
    if not _CHUNKED:
        pcm = synth.synth_pcm(3 * 4096 + 555, 2, 16, 44100, stream=6)
        fr, sizes, _ = oracle_ref.encode_stream(pcm, 2, 16, 44100)
        assert len(sizes) == 4
        _CHUNKED["v"] = (pcm, fr, [int(s) for s in sizes])
    return _CHUNKED["v"]


def _host_decode(d, frames, sizes, cap):
    """flacgpu_decode_frames through ctypes -> (return code, the whole output buffer, samples, results)."""
    import flacgpu

    n = len(sizes)
    out = ctypes.create_string_buffer(b"\xa5" * cap, cap)
    fb = (ctypes.c_uint32 * n)(*sizes)
    res = (flacgpu.DecodeResult * n)()
    ns = ctypes.c_uint64(0)
    src = ctypes.create_string_buffer(bytes(frames), len(frames))
    rc = d.lib.flacgpu_decode_frames(d.ctx, src, fb, n, out, cap, ctypes.byref(ns), res)
    return rc, out.raw, ns.value, list(res)


def test_decode_frames_in_chunks():
    pcm, fr, sizes = _chunked_stream()
    for max_frames in (1, 2, 3):  # 3: a ragged last chunk of one frame
        with _decoder(2, 16, max_frames=max_frames) as d:
            got, res = d.decode_frames(fr, sizes)
        assert got == pcm, max_frames
        assert [r.status for r in res] == [0, 0, 0, 0], max_frames
        assert [r.number for r in res] == [0, 1, 2, 3], max_frames
        assert [r.block_size for r in res] == [4096, 4096, 4096, 555], max_frames


def test_decode_frames_output_too_small_in_second_chunk():
    pcm, fr, sizes = _chunked_stream()
    with _decoder(2, 16, max_frames=2) as d:
        rc, buf, _, _ = _host_decode(d, fr, sizes, len(pcm) - 1)
    assert rc == -4  # FLACGPU_ERR_OUTPUT_TOO_SMALL
    first = 2 * 4096 * 4  # the first chunk's two frames
    assert buf[:first] == pcm[:first]


_RESULT_FIELDS = ("status", "block_size", "number", "sample_rate", "first_bad", "channel_assign", "bits")


def test_decode_frames_damaged_frame_in_second_chunk():
    pcm, fr, sizes = _chunked_stream()
    at = sum(sizes[:2]) + sizes[2] // 2  # a subframe byte of frame 2, far from its header and CRC
    bad = bytearray(fr)
    bad[at] ^= 0x08
    bad = bytes(bad)
    with _decoder(2, 16, max_frames=64) as d:
        _, want, n_bad = device_decode(d, _split(bad, sizes), out_bytes=len(pcm))
    assert n_bad == 1 and [r.status != 0 for r in want] == [False, False, True, False]
    with _decoder(2, 16, max_frames=2) as d:
        rc, _, _, res = _host_decode(d, bad, sizes, len(pcm))
    assert rc == 0
    for i in range(4):
        for f in _RESULT_FIELDS:
            assert getattr(res[i], f) == getattr(want[i], f), (i, f)


def _status_batch(tmp_path, exe, c, good_frames, good_pcm, bad_frames):
    """Corrupted frames between good ones in one device call; statuses against the host program's."""
    import test_decode_host as th

    host, _ = th.run_host(exe, tmp_path, bad_frames, c["channels"], c["bits"], c.get("rate", 44100), c.get("block", 4096))
    assert all(s != 0 for s in host["status"])
    per = c["channels"] * (c["bits"] // 8)
    slot = c.get("block", 4096) * per
    batch, offs, kinds = [], [], []
    for i, x in enumerate(bad_frames):
        g = i % len(good_frames)
        for fr, kind in ((good_frames[g], g), (x, -1)):
            offs.append(len(batch) * slot)
            batch.append(fr)
            kinds.append(kind)
    with _decoder(c["channels"], c["bits"], c.get("rate", 44100), max_frames=len(batch), block=c.get("block", 4096)) as d:
        buf, res, bad = device_decode(d, batch, pcm_offsets=offs, out_bytes=len(batch) * slot)
    k = 0
    for j, kind in enumerate(kinds):
        if kind < 0:
            assert res[j].status == host["status"][k], (c["name"], k, res[j].status, host["status"][k])
            assert set(buf[offs[j]:offs[j] + slot]) == {0xA5}, "a frame with a non-zero status wrote PCM"
            k += 1
        else:
            assert res[j].status == 0
            assert buf[offs[j]:offs[j] + len(good_pcm[kind])] == good_pcm[kind]
    assert bad == len(bad_frames)


def test_statuses_match_the_host_program(tmp_path):
    import test_decode_host as th

    exe = th.host_program(tmp_path)
    # the curated corruptions, on the hand-built frame they are defined for
    b = dc.curated_base()
    cur = dc.curated(b["frame"], b["marks"])
    good_pcm = [dc.oracle_pcm(b["frame"], b["channels"], b["bits"], 44100, b["number"])]
    _status_batch(tmp_path, exe, b, [b["frame"]], good_pcm, [fr for _, fr, _ in cur])
    # 50 of the seeded single-bit flips of every golden, and its frames cut short
    for c in dc.FRAME_CASES:
        frames, _ = dc.golden_frames(c)
        pcm = make_golden.make_pcm(c["name"], c["channels"], c["bits"], c["rate"], c["n_samples"], c["stream_seed"])
        per = c["channels"] * (c["bits"] // 8) * c["block"]
        good_pcm = [pcm[i * per:(i + 1) * per] for i in range(len(frames))]
        bad = [dc.flip(frames[f], bit) for f, bit in dc.random_flips(c, frames)[:50]]
        bad += [x for fr in frames[:2] for x in dc.cuts(fr)]
        _status_batch(tmp_path, exe, c, frames, good_pcm, bad)


# the ragged stream lengths of tests/test_gpu_plan.py
LENGTHS = [0, 1, 3, 4096, 5000, 8192, 4095, 3 * 4096 + 77, 1152, 4097, 6 * 4096, 255, 2 * 4096 + 4095, 64, 12345]


def test_verify_plan():
    import flacgpu

    torch, dev = _torch()
    ch, bits = 2, 16
    fbytes = ch * 2
    offs, pos = [], 0
    for n in LENGTHS:
        offs.append(pos)
        pos = (pos + n * fbytes + 36 + 15) & ~15
    buf = bytearray(pos + 64)
    for s, n in enumerate(LENGTHS):
        buf[offs[s]:offs[s] + n * fbytes] = synth.synth_pcm(n, ch, bits, 44100, stream=s)
    with flacgpu.Encoder(ch, bits, 44100, device=0, max_frames=64) as enc:
        plan = enc.plan(offs, LENGTHS)
        nf = int(plan.n_frames)
        d_pcm = torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).to(dev)
        d_out = torch.zeros(int(plan.out_bound), dtype=torch.uint8, device=dev)
        d_fb = torch.zeros(nf, dtype=torch.int32, device=dev)
        d_off = torch.zeros(nf, dtype=torch.int64, device=dev)
        d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
        d_res = torch.zeros(32 * nf, dtype=torch.uint8, device=dev)
        d_bad = torch.full((1,), 77, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        enc.encode_plan_device(plan, d_pcm.data_ptr(), d_out.data_ptr(), int(plan.out_bound), d_fb.data_ptr(),
                               d_off.data_ptr(), d_tot.data_ptr(), None, st)

        def verify():
            enc.verify_plan_device(plan, d_pcm.data_ptr(), d_out.data_ptr(), d_off.data_ptr(), d_fb.data_ptr(),
                                   d_res.data_ptr(), d_bad.data_ptr(), st)
            enc.sync_check(st)
            return _results(d_res, nf), int(d_bad.item())

        res, bad = verify()
        assert bad == 0 and [r.status for r in res] == [0] * nf
        # one byte of one frame of the bitstream
        s, k = 7, 2
        slot = int(plan.first_frame[s]) + k
        at = int(d_off[slot].item()) + int(d_fb[slot].item()) // 2
        d_out[at] = d_out[at] ^ 0x10
        res, bad = verify()
        assert bad == 1 and [i for i, r in enumerate(res) if r.status] == [slot]
        d_out[at] = d_out[at] ^ 0x10
        # one sample of the PCM
        s, k, i, c = 10, 3, 100, 1
        slot = int(plan.first_frame[s]) + k
        at = offs[s] + ((k * 4096 + i) * ch + c) * 2
        d_pcm[at] = d_pcm[at] ^ 0x01
        res, bad = verify()
        assert bad == 1 and [j for j, r in enumerate(res) if r.status] == [slot]
        assert res[slot].status == dc.STATUS["MISMATCH"] and res[slot].first_bad == i * ch + c
        plan.close()


def test_decode_file():
    import flacgpu

    ch, bits, rate = 2, 16, 44100
    pcm = synth.synth_pcm(3 * 4096 + 555, ch, bits, rate, stream=4)
    with flacgpu.Encoder(ch, bits, rate, device=0, max_frames=64) as enc:
        flac = enc.encode_file(pcm)
        assert flac == oracle_ref.encode_file(pcm, ch, bits, rate)
        got, ok = enc.decode_file(flac)
        assert got == pcm and ok
        bad = bytearray(flac)
        bad[8 + 18 + 5] ^= 0x40  # a byte of the STREAMINFO MD5
        got, ok = enc.decode_file(bytes(bad))
        assert got == pcm and not ok
    with _decoder(ch, bits, rate, max_frames=2) as d:  # chunks of two frames
        got, ok = d.decode_file(flac)
        assert got == pcm and ok
