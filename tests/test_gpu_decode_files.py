"""The many-files decode on the GPU: flacgpu_decode_files against flacgpu_decode_file per file
(both MD5 engines, a damaged file, a wrong bit depth, a capacity one byte short, the 32-bit path),
and flacgpu_decode_streams_device directly (regions, guards, results, digests, a region one
frame short).  The context holds 64 frames per call, so tiny files reach the chunk boundaries."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import oracle_ref  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

CH, BITS, RATE, BLOCK, PER = 2, 16, 44100, 256, 4
# frames per file.  In chunks of 64: the first cut falls exactly at the end of file 0, the next
# chunk holds files 1, 2 and the first 60 frames of file 3, the cut after it falls inside file 3.
FRAMES = [64, 1, 3, 70, 0]
SHORT_LAST = {2: 100}  # file 2's last frame has 100 samples
GUARD = 64


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _samples(i):
    n = FRAMES[i] * BLOCK
    return n - (BLOCK - SHORT_LAST[i]) if i in SHORT_LAST else n


@pytest.fixture(scope="module")
def files():
    """[(flac file, its PCM)], made once by the encoder on the GPU (bit-exact with the CPU reference)."""
    import flacgpu

    pcms = [synth.synth_pcm(_samples(i), CH, BITS, RATE, stream=10 + i) if FRAMES[i] else b"" for i in range(len(FRAMES))]
    with flacgpu.Encoder(CH, BITS, RATE, device=0, max_frames=128, block_size=BLOCK) as enc:
        flacs = enc.encode_files(pcms)
    assert flacs[2] == oracle_ref.encode_file(pcms[2], CH, BITS, RATE, block=BLOCK)
    assert [len(flacgpu.flac_index(f)[2]) for f in flacs] == FRAMES
    return list(zip(flacs, pcms))


@pytest.fixture(scope="module")
def ctx():
    import flacgpu

    with flacgpu.Decoder(CH, BITS, RATE, device=0, max_frames=64, block_size=BLOCK) as d:
        yield d


def single(d, flac, cap, guard=GUARD):
    """flacgpu_decode_file on one file -> (status, PCM bytes, md5_ok, guard bytes)."""
    out = ctypes.create_string_buffer(b"\xA5" * (cap + guard + 1), cap + guard + 1)
    ns, ok = ctypes.c_uint64(0), ctypes.c_int(0)
    rc = d.lib.flacgpu_decode_file(d.ctx, bytes(flac), len(flac), out, cap, ctypes.byref(ns), ctypes.byref(ok))
    per = d.channels * d.bytes_per_sample
    return rc, out.raw[: min(ns.value * per, cap)], bool(ok.value), out.raw[cap: cap + guard]


def force_engine(engine):
    import flacgpu

    r = flacgpu.Md5Rates()
    fast, slow = 1e15, 1.0
    for i in range(4):
        r.host_chain[i] = (fast if engine == flacgpu.MD5_HOST else slow) * (i + 1)
    r.device_lane = r.device_chip = slow if engine == flacgpu.MD5_HOST else fast
    r.host_workers = 4
    flacgpu.set_md5_rates(r)
    assert flacgpu.md5_engine_for(4, 1 << 16, 1 << 18) == engine


def check_equal_to_single(d, flacs, caps=None):
    caps = [max(len(p), 1) for _, p in flacs] if caps is None else caps
    got = d.decode_files([f for f, _ in flacs], pcm_caps=caps, guard=GUARD)
    for i, ((flac, _), cap) in enumerate(zip(flacs, caps)):
        want = single(d, flac, cap)
        assert got[i] == want, f"file {i}: status {got[i][0]} vs {want[0]}"
        assert got[i][3] == b"\xA5" * GUARD, f"file {i}: bytes after its capacity were written"
    return got


@pytest.mark.parametrize("engine", ["host", "device"])
def test_decode_files_equals_decode_file(ctx, files, engine):
    import flacgpu

    e = flacgpu.MD5_HOST if engine == "host" else flacgpu.MD5_DEVICE
    ctx.set_timing(True)
    try:
        force_engine(e)
        ctx.reset_timing()
        got = ctx.decode_files([f for f, _ in files], pcm_caps=[max(len(p), 1) for _, p in files], guard=GUARD)
        md5_launches, _ = ctx.kernel_time(flacgpu.K_MD5)
        index_launches, _ = ctx.kernel_time(flacgpu.K_INDEX)
        check_equal_to_single(ctx, files)
    finally:
        ctx.set_timing(False)
        flacgpu.set_md5_rates(None)
    for (st, pcm, ok, guard), (_, want) in zip(got, files):
        assert (st, pcm, ok) == (0, want, True) and guard == b"\xA5" * GUARD
    assert md5_launches == (1 if e == flacgpu.MD5_DEVICE else 0)  # the engine that was asked for ran
    assert index_launches == 1  # all files in one index


def test_one_damaged_file(ctx, files):
    import flacgpu

    first = flacgpu.flac_index(files[2][0])[1]
    bad = bytearray(files[2][0])
    bad[first + 40] ^= 0x10  # inside the first frame of the third file
    flacs = list(files)
    flacs[2] = (bytes(bad), files[2][1])
    got = check_equal_to_single(ctx, flacs)
    assert got[2][0] == -2
    for i in (0, 1, 3, 4):
        assert got[i][:3] == (0, files[i][1], True)


def test_wrong_bit_depth_and_short_capacity(ctx, files):
    import flacgpu

    pcm24 = synth.synth_pcm(300, CH, 24, RATE, stream=3)
    with flacgpu.Encoder(CH, 24, RATE, device=0, max_frames=64, block_size=BLOCK) as enc:
        other = enc.encode_file(pcm24)
    flacs = [files[1], (other, b""), files[2], files[0]]
    caps = [len(files[1][1]), 300 * CH * 3, len(files[2][1]) - 1, len(files[0][1])]
    got = check_equal_to_single(ctx, flacs, caps)
    assert got[1][0] == -2 and got[2][0] == -4  # INVALID_INPUT, OUTPUT_TOO_SMALL
    assert got[0][:3] == (0, files[1][1], True) and got[3][:3] == (0, files[0][1], True)


def test_32_bit_lpc_files():
    import flacgpu

    pcms = [synth.synth_pcm(4096 + 1000 + i, 2, 32, 96000, stream=20 + i) for i in range(2)]
    with flacgpu.Encoder(2, 32, 96000, device=0, max_frames=64, lpc_order=12) as enc:
        flacs = list(zip(enc.encode_files(pcms), pcms))
    assert all(len(flacgpu.flac_index(f)[2]) == 2 for f, _ in flacs)
    with flacgpu.Decoder(2, 32, 96000, device=0, max_frames=64) as d:
        got = check_equal_to_single(d, flacs)
    for (st, pcm, ok, _), (_, want) in zip(got, flacs):
        assert (st, pcm, ok) == (0, want, True)


def test_argument_checks(ctx):
    L = ctx.lib
    ptrs = (ctypes.c_void_p * 1)()
    sz = (ctypes.c_size_t * 1)()
    ns = (ctypes.c_uint64 * 1)()
    st = (ctypes.c_int * 1)()
    assert L.flacgpu_decode_files(ctx.ctx, 1, None, sz, ptrs, sz, ns, None, st) == -2
    assert L.flacgpu_decode_files(ctx.ctx, 1, ptrs, sz, ptrs, sz, ns, None, None) == -2
    assert L.flacgpu_decode_files(ctx.ctx, 0, None, None, None, None, None, None, None) == 0
    buf = ctypes.create_string_buffer(64)
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    f = L.flacgpu_decode_streams_device
    assert f(ctx.ctx, None, 2, u64, u64, None, None, buf, u64, u64, buf, None, None) == -2
    assert f(ctx.ctx, buf, 2, u64, u64, None, None, None, u64, u64, buf, None, None) == -2
    assert f(ctx.ctx, buf, 2, u64, u64, None, None, buf, None, u64, buf, None, None) == -2
    assert f(ctx.ctx, buf, 2, u64, u64, None, None, buf, u64, u64, None, None, None) == -2
    odd = (ctypes.c_uint64 * 2)(0, 9)  # a digest needs 4-byte aligned regions
    assert f(ctx.ctx, buf, 2, u64, u64, None, None, buf, odd, u64, buf, buf, None) == -2


# ---- flacgpu_decode_streams_device directly ------------------------------------------------------
def decode_streams(d, files, short=None):
    """The files' frames at odd offsets of one device buffer through flacgpu_decode_streams_device,
    PCM regions of exact capacity between 0xA5 guards of 64 bytes (stream `short`: one frame less)
    -> (output bytes, [region offset], [region capacity], [StreamResult], [digest])."""
    import flacgpu

    torch, dev = _torch()
    blob, offs, lens = bytearray(b"\xA5" * 3), [], []
    for flac, _ in files:
        first = flacgpu.flac_index(flac)[1]
        if len(blob) % 2 == 0:
            blob += b"\xA5"
        offs.append(len(blob))
        lens.append(len(flac) - first)
        blob += flac[first:]
    blob += b"\xA5" * 16
    caps = [len(p) for _, p in files]
    if short is not None:
        caps[short] -= BLOCK * PER
    pcm_offs, at = [], GUARD
    for c in caps:
        pcm_offs.append(at)
        at += c + GUARD
    n = len(files)
    d_buf = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
    d_out = torch.full((at,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((32 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_md5 = torch.full((16 * n,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    d.decode_streams_device(d_buf.data_ptr(), offs, lens, d_out.data_ptr(), pcm_offs, caps, d_res.data_ptr(),
                            d_md5=d_md5.data_ptr(), stream_bits=[BITS] * n, stream_rates=[RATE] * n, stream=st)
    d.sync_check(st)
    res = list((flacgpu.StreamResult * n).from_buffer_copy(d_res.cpu().numpy().tobytes()))
    dig = d_md5.cpu().numpy().tobytes()
    return d_out.cpu().numpy().tobytes(), pcm_offs, caps, res, [dig[16 * i:16 * i + 16] for i in range(n)]


def _guards_intact(out, pcm_offs, caps):
    at = 0
    for o, c in zip(pcm_offs, caps):
        if set(out[at:o]) != {0xA5}:
            return False
        at = o + c
    return set(out[at:]) == {0xA5}


def test_decode_streams_device(ctx, files):
    import flacgpu

    out, pcm_offs, caps, res, dig = decode_streams(ctx, files)
    assert all(o % 4 == 0 for o in pcm_offs)
    assert _guards_intact(out, pcm_offs, caps)
    for i, (flac, pcm) in enumerate(files):
        _, first, sizes = flacgpu.flac_index(flac)
        host_pcm, frame_res = ctx.decode_frames(flac[first:], sizes)  # the host path, frame by frame
        assert host_pcm == pcm and out[pcm_offs[i]:pcm_offs[i] + caps[i]] == pcm, i
        bad = [k for k, r in enumerate(frame_res) if r.status]
        r = res[i]
        assert (r.n_frames, r.index_status, r.bad_frames) == (len(sizes), 0, len(bad)), i
        assert r.n_samples == sum(fr.block_size for fr in frame_res if fr.status == 0) == _samples(i), i
        assert (r.first_bad_frame, r.first_bad_status) == (0xFFFFFFFF, 0), i
        assert dig[i] == hashlib.md5(pcm).digest(), i


def test_stream_region_one_frame_short(ctx, files):
    short = 3  # 70 frames, decoded in two chunks; file 4 (no frames) and nothing else follows it
    order = [files[1], files[3], files[2], files[0]]
    out, pcm_offs, caps, res, dig = decode_streams(ctx, order, short=1)
    assert _guards_intact(out, pcm_offs, caps)
    r = res[1]
    assert (r.n_frames, r.index_status) == (FRAMES[short], 0)
    assert (r.bad_frames, r.first_bad_frame, r.first_bad_status) == (1, FRAMES[short] - 1, 7)  # the last frame: RANGE
    assert r.n_samples == (FRAMES[short] - 1) * BLOCK
    assert out[pcm_offs[1]:pcm_offs[1] + caps[1]] == order[1][1][:caps[1]]  # the frames that fit are there
    assert dig[1] == bytes(16)
    for i in (0, 2, 3):  # the neighbours: their regions, results and digests as if nothing had happened
        assert out[pcm_offs[i]:pcm_offs[i] + caps[i]] == order[i][1], i
        assert (res[i].bad_frames, res[i].first_bad_frame) == (0, 0xFFFFFFFF), i
        assert dig[i] == hashlib.md5(order[i][1]).digest(), i
