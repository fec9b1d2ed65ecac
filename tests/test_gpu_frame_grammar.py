"""The device decoder (zig-flac_amd/csrc/fg_dec.hip), the device frame index and the many-streams
decode on frames of the seeded grammar (frame_grammar.py): layouts no encoder here writes, whose
expected PCM is the generator's own samples and no decoder's output.

Every frame is valid and has been decoded on the CPU under the sanitizers by
tests/test_frame_grammar_host.py; nothing here is corrupted."""
import hashlib
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import decode_cases as dc  # noqa: E402
import frame_grammar as fg  # noqa: E402
import test_gpu_decode as tgd  # noqa: E402
import test_gpu_index_streams as tis  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = fg.cases()
IDS = [c["name"] for c in CASES]
GUARD = 4099  # odd: the PCM starts at an address that is no multiple of 16, 4 or 2
CTX_RATE = 12345  # what a context states for rate code 0 where several cases share it
MIXED = [(1, 16), (2, 16), (2, 24), (2, 32)]  # the (channels, bits) pairs with several cases


def _group(ch, bits):
    return [c for c in CASES if (c["channels"], c["bits"]) == (ch, bits)]


def _check_results(res, frames, stream_rate):
    assert [r.status for r in res] == [0] * len(frames)
    assert [r.number for r in res] == [f["number"] for f in frames]
    assert [r.block_size for r in res] == [f["block"] for f in frames]
    assert [r.channel_assign for r in res] == [f["chc"] for f in frames]
    assert [r.sample_rate for r in res] == [stream_rate if f["rate"] is None else f["rate"] for f in frames]
    assert all(r.first_bad == 0 for r in res)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_device_decode_of_every_case(c):
    frames = [f["frame"] for f in c["frames"]]
    pcm = fg.case_pcm(c)
    with tgd._decoder(c["channels"], c["bits"], c["rate"], max_frames=8) as d:
        # the host-buffer entry point
        got, res = d.decode_frames(b"".join(frames), [len(x) for x in frames])
        _check_results(res, c["frames"], c["rate"])
        assert res[0].bits == c["bits"] and got == pcm
        # device buffers: guard bands around an unaligned output
        buf, res, bad = tgd.device_decode(d, frames, out_bytes=len(pcm), guard=GUARD)
        _check_results(res, c["frames"], c["rate"])
        assert bad == 0 and buf[GUARD:GUARD + len(pcm)] == pcm
        assert set(buf[:GUARD]) == {0xA5} and set(buf[GUARD + len(pcm):]) == {0xA5}
        # the verify path: the generator's PCM as the expectation, nothing written
        buf, res, bad = tgd.device_decode(d, frames, out_bytes=len(pcm), expect=pcm, guard=GUARD, write=False)
        _check_results(res, c["frames"], c["rate"])
        assert bad == 0 and set(buf) == {0xA5}
        # one bit of one sample of the expectation
        rng = random.Random("flip:" + c["name"])
        j = rng.randrange(len(frames))
        e = rng.randrange(c["frames"][j]["block"] * c["channels"])  # interleaved sample index within frame j
        at = sum(len(f["pcm"]) for f in c["frames"][:j]) + e * (c["bits"] // 8) + rng.randrange(c["bits"] // 8)
        wrong = bytearray(pcm)
        wrong[at] ^= 1 << rng.randrange(8)
        _, res, bad = tgd.device_decode(d, frames, out_bytes=len(pcm), expect=bytes(wrong), write=False)
        assert bad == 1 and [r.status for r in res] == [dc.STATUS["MISMATCH"] if k == j else 0 for k in range(len(frames))]
        assert res[j].first_bad == e


@pytest.mark.parametrize("ch,bits", MIXED)
def test_mixed_batch_in_chunks(ch, bits):
    """All cases of one (channels, bits) pair as one run of frames of mixed block sizes, subframe
    types and stereo layouts, through the chunk loop with 1 and 3 frames a chunk and in one chunk."""
    group = _group(ch, bits)
    frames = [f for c in group for f in c["frames"]]
    assert len(group) >= 3 and len({f["block"] for f in frames}) >= 6
    data = b"".join(f["frame"] for f in frames)
    pcm = b"".join(f["pcm"] for f in frames)
    for max_frames in (1, 3, len(frames)):
        with tgd._decoder(ch, bits, CTX_RATE, max_frames=max_frames) as d:
            got, res = d.decode_frames(data, [len(f["frame"]) for f in frames])
        _check_results(res, frames, CTX_RATE)
        assert got == pcm, max_frames


@pytest.mark.parametrize("name", ["five_by_32", "eight_by_32"])
def test_more_channels_than_wide_planes(name):
    """5 and 8 channels at 32 bits: the 64-bit planes of four subframes fit at a time, so the frame
    takes a checking pass and a writing pass of two rounds each.  Frames at scattered PCM offsets."""
    c = next(c for c in CASES if c["name"] == name)
    for f in c["frames"]:
        assert {"verbatim", "lpc", "constant"} <= {s["type"] for s in f["subs"]}
    frames = [f["frame"] for f in c["frames"]]
    sizes = [len(f["pcm"]) for f in c["frames"]]
    # the frames' regions in reverse order, 7 bytes of guard before each
    offs, at = [0] * len(frames), 7
    for k in reversed(range(len(frames))):
        offs[k] = at
        at += sizes[k] + 7
    with tgd._decoder(c["channels"], 32, c["rate"], max_frames=4) as d:
        buf, res, bad = tgd.device_decode(d, frames, pcm_offsets=offs, out_bytes=at, guard=GUARD)
    _check_results(res, c["frames"], c["rate"])
    want = bytearray(b"\xa5" * (GUARD + at + GUARD))
    for k, f in enumerate(c["frames"]):
        want[GUARD + offs[k]:GUARD + offs[k] + sizes[k]] = f["pcm"]
    assert bad == 0 and buf == bytes(want)


@pytest.fixture(scope="module")
def ctx():
    import flacgpu

    with flacgpu.Decoder(2, 16, 44100, device=0, max_frames=64) as d:
        yield d


def test_device_index_of_every_case(ctx):
    """flacgpu_flac_index_device per case, then all cases as the streams of one buffer in one
    call: the sizes and offsets of the host index, which the CPU module checked to be the true ones."""
    import flacgpu

    torch, dev = tgd._torch()
    streams = [(c["name"], fg.case_bytes(c), c["bits"], c["rate"]) for c in CASES]
    wanted = [[len(f["frame"]) for f in c["frames"]] for c in CASES]
    assert wanted == [flacgpu.flac_index(s[1], raw_frames=True)[2] for s in streams]
    st = torch.cuda.current_stream(dev).cuda_stream
    for (name, data, bits, rate), want in zip(streams, wanted):
        cap = len(data) // 8 + 1
        d_buf = torch.from_numpy(np.frombuffer(b"\xa5" * 5 + data + b"\xa5" * 16, dtype=np.uint8).copy()).to(dev)
        d_off = torch.full((cap,), -1, dtype=torch.int64, device=dev)
        d_fb = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        d_res = torch.full((16,), 0xA5, dtype=torch.uint8, device=dev)
        ctx.flac_index_device(d_buf.data_ptr() + 5, len(data), d_off.data_ptr(), d_fb.data_ptr(), cap, d_res.data_ptr(),
                              stream_bits=bits, stream_rate=rate, stream=st)
        ctx.sync_check(st)
        r = flacgpu.IndexResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
        assert (r.status, r.n_frames) == (0, len(want)), name
        assert d_fb.cpu().tolist()[:len(want)] == want, name
        assert d_off.cpu().tolist()[:len(want)] == [int(v) for v in np.cumsum([0] + want)[:-1]], name
        assert set(d_fb.cpu().tolist()[len(want):]) <= {-1}, name
    got, offs_t, sizes_t, first, offs = tis.index_streams(ctx, streams)
    tis.check_tables(streams, wanted, got, offs_t, sizes_t, first, offs)


@pytest.mark.parametrize("ch,bits", MIXED)
def test_decode_streams_of_one_buffer(ch, bits):
    """The cases of one (channels, bits) pair as separate streams of one device buffer through
    flacgpu_decode_streams_device, four frames a chunk so that chunks run on from one stream into
    the next: every stream's PCM, counts and MD5, and the bytes between the regions."""
    import flacgpu

    torch, dev = tgd._torch()
    group = _group(ch, bits)
    blob, offs = bytearray(b"\xa5" * 3), []
    for c in group:
        if len(blob) % 2 == 0:
            blob += b"\xa5"
        offs.append(len(blob))
        blob += fg.case_bytes(c)
    blob += b"\xa5" * 16
    pcms = [fg.case_pcm(c) for c in group]
    caps = [len(p) for p in pcms]
    pcm_offs, at = [], 64
    for cap in caps:
        pcm_offs.append(at)
        at = (at + cap + 64 + 3) & ~3  # the device MD5 wants 4-byte aligned regions
    n = len(group)
    d_buf = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
    d_out = torch.full((at,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((32 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_md5 = torch.full((16 * n,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with tgd._decoder(ch, bits, CTX_RATE, max_frames=4) as d:
        d.decode_streams_device(d_buf.data_ptr(), offs, [len(fg.case_bytes(c)) for c in group], d_out.data_ptr(), pcm_offs,
                                caps, d_res.data_ptr(), d_md5=d_md5.data_ptr(), stream_bits=[bits] * n,
                                stream_rates=[c["rate"] for c in group], stream=st)
        d.sync_check(st)
    out = d_out.cpu().numpy().tobytes()
    res = list((flacgpu.StreamResult * n).from_buffer_copy(d_res.cpu().numpy().tobytes()))
    dig = d_md5.cpu().numpy().tobytes()
    want = bytearray(b"\xa5" * at)
    for i, c in enumerate(group):
        want[pcm_offs[i]:pcm_offs[i] + caps[i]] = pcms[i]
        r = res[i]
        assert (r.n_frames, r.index_status, r.bad_frames) == (len(c["frames"]), 0, 0), c["name"]
        assert r.n_samples == sum(f["block"] for f in c["frames"]), c["name"]
        assert (r.first_bad_frame, r.first_bad_status) == (0xFFFFFFFF, 0), c["name"]
        assert out[pcm_offs[i]:pcm_offs[i] + caps[i]] == pcms[i], c["name"]
        assert dig[16 * i:16 * i + 16] == hashlib.md5(pcms[i]).digest(), c["name"]
    assert out == bytes(want)


def _flac_file(c) -> bytes:
    """RFC 9639 8.1 / 8.2: "fLaC", one last metadata block of type 0 and 34 bytes (block size range,
    frame size range, rate 20 bits, channels - 1 3 bits, depth - 1 5 bits, samples 36 bits, the
    MD5 of the interleaved little-endian PCM), then the frames."""
    blocks = [f["block"] for f in c["frames"]]
    sizes = [len(f["frame"]) for f in c["frames"]]
    packed = (c["rate"] << 44) | ((c["channels"] - 1) << 41) | ((c["bits"] - 1) << 36) | sum(blocks)
    si = (min(blocks).to_bytes(2, "big") + max(blocks).to_bytes(2, "big") + min(sizes).to_bytes(3, "big") +
          max(sizes).to_bytes(3, "big") + packed.to_bytes(8, "big") + hashlib.md5(fg.case_pcm(c)).digest())
    assert len(si) == 34
    return b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + si + fg.case_bytes(c)


@pytest.mark.parametrize("name", ["seed30_2x16", "fixed_orders_stereo_24", "eight_by_32"])
def test_whole_file(name):
    c = next(c for c in CASES if c["name"] == name)
    flac = _flac_file(c)
    with tgd._decoder(c["channels"], c["bits"], c["rate"], max_frames=2) as d:  # two frames a chunk
        got, ok = d.decode_file(flac)
        assert got == fg.case_pcm(c) and ok
        bad = bytearray(flac)
        bad[8 + 18 + 3] ^= 0x02  # a byte of the STREAMINFO MD5
        got, ok = d.decode_file(bytes(bad))
        assert got == fg.case_pcm(c) and not ok
