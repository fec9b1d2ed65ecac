"""Frames of 4097 to 16384 samples on the device decoder (zig-flac_amd/csrc/fg_dec.hip) through a
decode-only context (flacgpu_open_decoder): the frames of bigblock_cases.py, whose expected PCM is
the generator's own samples, and frames of the oracle encoder at blocks 4608 and 16384.

Every frame is valid and has been decoded on the CPU under the sanitizers by
tests/test_bigblock_host.py; nothing here is corrupted.  Contexts hold at most 8 frames a call."""
import ctypes
import hashlib
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import bigblock_cases as bb  # noqa: E402
import decode_cases as dc  # noqa: E402
import frame_grammar as fg  # noqa: E402
import oracle_ref  # noqa: E402
import synth  # noqa: E402
import test_gpu_decode as tgd  # noqa: E402
import test_gpu_frame_grammar as tgf  # noqa: E402
import window_helpers as wh  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = bb.cases()
IDS = [c["name"] for c in CASES]
GUARD = 4099  # odd
CTX_RATE = 12345


def _block(c):
    """The smallest of the three plane sizes that holds the case's largest frame, at its limit."""
    top = max(f["block"] for f in c["frames"])
    return 8192 if top <= 8192 else 16384


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_device_decode_of_every_case(c):
    """The four checks of test_gpu_frame_grammar.test_device_decode_of_every_case."""
    frames = [f["frame"] for f in c["frames"]]
    pcm = fg.case_pcm(c)
    with tgd._decoder(c["channels"], c["bits"], c["rate"], max_frames=8, block=_block(c)) as d:
        got, res = d.decode_frames(b"".join(frames), [len(x) for x in frames])
        tgf._check_results(res, c["frames"], c["rate"])
        assert res[0].bits == c["bits"] and got == pcm
        buf, res, bad = tgd.device_decode(d, frames, out_bytes=len(pcm), guard=GUARD)
        tgf._check_results(res, c["frames"], c["rate"])
        assert bad == 0 and buf[GUARD:GUARD + len(pcm)] == pcm
        assert set(buf[:GUARD]) == {0xA5} and set(buf[GUARD + len(pcm):]) == {0xA5}
        buf, res, bad = tgd.device_decode(d, frames, out_bytes=len(pcm), expect=pcm, guard=GUARD, write=False)
        tgf._check_results(res, c["frames"], c["rate"])
        assert bad == 0 and set(buf) == {0xA5}
        rng = random.Random("flip:" + c["name"])
        j = max(range(len(frames)), key=lambda k: c["frames"][k]["block"])  # a big frame
        e = rng.randrange(c["frames"][j]["block"] * c["channels"])
        at = sum(len(f["pcm"]) for f in c["frames"][:j]) + e * (c["bits"] // 8) + rng.randrange(c["bits"] // 8)
        wrong = bytearray(pcm)
        wrong[at] ^= 1 << rng.randrange(8)
        _, res, bad = tgd.device_decode(d, frames, out_bytes=len(pcm), expect=bytes(wrong), write=False)
        assert bad == 1 and [r.status for r in res] == [dc.STATUS["MISMATCH"] if k == j else 0 for k in range(len(frames))]
        assert res[j].first_bad == e


@pytest.mark.parametrize("max_frames", [1, 3, 0])
def test_mixed_batch_of_big_and_small_frames(max_frames):
    """Every 16-bit stereo frame, of this module's cases and of the grammar's, as one run: segments
    of 64, 128 and 256 samples in one call, in chunks of 1 and 3 frames and in one chunk."""
    frames = [f for c in CASES + list(fg.cases()) if (c["channels"], c["bits"]) == (2, 16) for f in c["frames"]]
    assert sum(f["block"] > 4096 for f in frames) >= 4 and sum(f["block"] <= 4096 for f in frames) >= 10
    data = b"".join(f["frame"] for f in frames)
    pcm = b"".join(f["pcm"] for f in frames)
    with tgd._decoder(2, 16, CTX_RATE, max_frames=max_frames or len(frames), block=8192) as d:
        got, res = d.decode_frames(data, [len(f["frame"]) for f in frames])
    tgf._check_results(res, frames, CTX_RATE)
    assert got == pcm


@pytest.mark.parametrize("name", ["big_eight_by_16", "big_five_by_32"])
def test_more_channels_than_planes(name):
    """8 x 16-bit at 16384 and 5 x 32-bit at 8192: two planes fit, so a checking and a writing pass
    of four / three rounds.  The frame twice, at scattered PCM offsets in reverse order."""
    c = bb.case(name)
    fr = c["frames"][0]
    frames = [fr["frame"], fr["frame"]]
    size = len(fr["pcm"])
    offs = [7 + size + 7, 7]
    at = 7 + size + 7 + size + 7
    with tgd._decoder(c["channels"], c["bits"], c["rate"], max_frames=2, block=_block(c)) as d:
        buf, res, bad = tgd.device_decode(d, frames, pcm_offsets=offs, out_bytes=at, guard=GUARD)
    tgf._check_results(res, [fr, fr], c["rate"])
    want = bytearray(b"\xa5" * (GUARD + at + GUARD))
    for o in offs:
        want[GUARD + o:GUARD + o + size] = fr["pcm"]
    assert bad == 0 and buf == bytes(want)


@pytest.mark.parametrize("block", [4608, 16384])
def test_frames_of_the_oracle_encoder(block):
    """About three frames with a short last one, encoded on the CPU at a block the GPU encoder never writes."""
    n = 2 * block + 1234
    pcm = synth.synth_pcm(n, 2, 16, 44100, stream=block)
    fr, sizes, _ = oracle_ref.encode_stream(pcm, 2, 16, 44100, block)
    ref, _ = oracle_ref.decode_frames(fr, 2, 16, 44100, n)
    assert ref == pcm and len(sizes) == 3
    with tgd._decoder(2, 16, 44100, max_frames=8, block=block) as d:
        got, res = d.decode_frames(fr, sizes)
    assert [r.status for r in res] == [0, 0, 0]
    assert [r.block_size for r in res] == [block, block, 1234] and [r.number for r in res] == [0, 1, 2]
    assert got == pcm


def test_limits():
    import flacgpu
    import flac_bits as fbits

    L = flacgpu.load_library()
    big = bb.case("big_mono_a")["frames"][1]  # 4608 samples
    fr = fbits.frame(0, 16385, 0, 16, lambda w: fbits.sub_constant(w, 5, 16))
    with tgd._decoder(1, 16, 44100, max_frames=4, block=16384) as d:
        _, res = d.decode_frames(fr + big["frame"], [len(fr), len(big["frame"])])
        assert [r.status for r in res] == [dc.STATUS["RANGE"], 0] and res[0].block_size == 16385
    with tgd._decoder(1, 16, 44100, max_frames=4, block=4096) as d:  # flacgpu_open's context
        got, res = d.decode_frames(big["frame"], [len(big["frame"])])
        assert [r.status for r in res] == [dc.STATUS["RANGE"]] and got == b""
    for ch, bits, block in ((2, 16, 16385), (2, 32, 8193), (1, 32, 16384), (9, 16, 8192), (2, 12, 8192)):
        with pytest.raises(flacgpu.FlacGpuError) as e:
            flacgpu.Decoder(ch, bits, 44100, max_frames=4, block_size=block)
        assert e.value.code == -1
    cfg = flacgpu.Config.default(2, 16, 44100)
    cfg.block_size = 4097
    h = ctypes.c_void_p()
    assert L.flacgpu_open(0, ctypes.byref(cfg), 4, ctypes.byref(h)) == -1  # the encoder's limit stays


def test_encode_entry_points_refuse_a_decode_only_context():
    import flacgpu

    c = bb.case("big_mid_side_16")
    frames = [f["frame"] for f in c["frames"]]
    pcm = fg.case_pcm(c)
    with tgd._decoder(2, 16, c["rate"], max_frames=4, block=8192) as d:
        calls = [lambda: d.encode_frames(pcm[:4096]), lambda: d.plan([0], [1024]), lambda: d.encode_file(pcm[:4096]),
                 lambda: d.encode_files([pcm[:4096]]), lambda: d.set_records(True), lambda: d.set_md5_engine(flacgpu.MD5_DEVICE)]
        for k, call in enumerate(calls):
            with pytest.raises(flacgpu.FlacGpuError) as e:
                call()
            assert e.value.code == -1, k
        got, res = d.decode_frames(b"".join(frames), [len(x) for x in frames])  # and it still decodes
        assert got == pcm and [r.status for r in res] == [0, 0]
        assert d.md5(pcm) == hashlib.md5(pcm).digest()  # the host engine


def test_decode_file_and_files():
    """A 4608-block case behind a STREAMINFO block: the single-file and the many-files call, MD5 verdict included."""
    c = bb.case("big_left_side_24")
    flac = tgf._flac_file(c)
    pcm = fg.case_pcm(c)
    bad = bytearray(flac)
    bad[8 + 18 + 3] ^= 0x02  # a byte of the STREAMINFO MD5
    with tgd._decoder(2, 24, c["rate"], max_frames=1, block=8192) as d:
        assert d.decode_file(flac) == (pcm, True)
        assert d.decode_file(bytes(bad)) == (pcm, False)
        res = d.decode_files([flac, bytes(bad), flac[:-9]])
        assert res[0] == (0, pcm, True) and res[1] == (0, pcm, False) and res[2][0] != 0 and not res[2][2]


WINDOWS = {  # (start, count): inside a big frame, across each boundary, everything, and past the end
    "big_mono_b": [(100, 50), (8193 - 3, 10), (8193 + 16383 - 1, 2), (8000, 20000), (0, 1 << 20), (8193 + 16383 + 16000, 9999)],
    "big_variable": [(4607, 2), (4600, 100), (4608 + 64 + 8191, 2), (5000, 9000), (0, 1 << 20)],
}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_windows_inside_and_across_big_frames(name):
    c = bb.case(name)
    wh.grammar_call(c, [(0, s, n) for s, n in WINDOWS[name]], wh.odd_layout, block_size=16384)


def test_flacbank_crops_of_big_frames():
    import flacbank
    import torch

    names = sorted(WINDOWS)
    cs = [bb.case(n) for n in names]
    assert {(c["channels"], c["bits"]) for c in cs} == {(1, 16), (2, 16)}
    for c in cs:
        x = np.frombuffer(fg.case_pcm(c), dtype="<i2").reshape(-1, c["channels"]).astype(np.int32)
        length = 6000
        starts = [s for s, _ in WINDOWS[c["name"]]]
        with flacbank.FlacBank([tgf._flac_file(c)], max_frames=8) as bank:
            assert bank._dec.block_size == max(f["block"] for f in c["frames"])
            for dtype in (torch.int32, torch.float32):
                got, n = bank.crops([0] * len(starts), starts, length, dtype=dtype, planar=False)
                got = got.cpu().numpy()
                for w, s in enumerate(starts):
                    take = max(0, min(length, len(x) - s))
                    assert n[w] == take
                    want = np.zeros((length, c["channels"]), dtype=np.int32)
                    want[:take] = x[s:s + take]
                    if dtype == torch.int32:
                        assert (got[w] == want).all(), (c["name"], w)
                    else:
                        assert (got[w] == want.astype(np.float32) / 32768.0).all(), (c["name"], w)


def test_flacbank_refuses_a_file_that_states_32768():
    import flacbank

    c = bb.case("big_mono_a")
    flac = bytearray(tgf._flac_file(c))
    flac[10:12] = (32768).to_bytes(2, "big")  # STREAMINFO's max_block_size
    with pytest.raises(ValueError, match=r"file 1 states blocks of 32768"):
        flacbank.FlacBank([tgf._flac_file(c), bytes(flac)])
