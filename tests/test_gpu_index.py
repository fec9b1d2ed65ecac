"""The device frame index (zig-flac_amd/csrc/fg_index.hip) on the GPU against the host index
flacgpu_flac_index: every stream of index_cases.cases() (all of them cleared by the sanitizer run
of test_index_host.py first), the cap and guard rules, the index feeding the device decoder, and
the whole-file decode built on it."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import decode_cases as dc  # noqa: E402
import index_cases as ic  # noqa: E402
import make_golden  # noqa: E402
import oracle_ref  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 5  # entries past the capacity of both output arrays
CASES = ic.cases()


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    import flacgpu

    with flacgpu.Decoder(2, 16, 44100, device=0, max_frames=64) as d:
        yield d


def device_index(d, data, bits, rate, cap=None, at=3):
    """flacgpu_flac_index_device over `data` placed `at` bytes (odd) into a 0xA5-filled allocation ->
    (status, n_frames, offsets array, sizes array), the arrays cap + GUARD long and 0xA5-filled."""
    import flacgpu

    torch, dev = _torch()
    n = len(data)
    cap = n // 8 + 1 if cap is None else cap
    host = np.full(at + n + 7, 0xA5, dtype=np.uint8)
    host[at:at + n] = np.frombuffer(data, dtype=np.uint8)
    d_buf = torch.from_numpy(host).to(dev)
    d_off = torch.full((8 * (cap + GUARD),), 0xA5, dtype=torch.uint8, device=dev)
    d_fb = torch.full((4 * (cap + GUARD),), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((16,), 0xA5, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    d.flac_index_device(d_buf.data_ptr() + at, n, d_off.data_ptr(), d_fb.data_ptr(), cap, d_res.data_ptr(),
                        stream_bits=bits, stream_rate=rate, stream=st)
    d.sync_check(st)
    res = flacgpu.IndexResult.from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert res.reserved == 0
    return (res.status, res.n_frames, np.frombuffer(d_off.cpu().numpy().tobytes(), dtype=np.uint64),
            np.frombuffer(d_fb.cpu().numpy().tobytes(), dtype=np.uint32))


def _untouched(offs, sizes, start):
    return bool((offs[start:] == 0xA5A5A5A5A5A5A5A5).all() and (sizes[start:] == 0xA5A5A5A5).all())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_index_equals_the_host_index(ctx, case):
    import flacgpu

    name, data, bits, rate = case
    want = ic.host_index(data)
    status, n, offs, sizes = device_index(ctx, data, bits, rate)
    if want is None:
        assert (status, n) == (flacgpu.INDEX_INVALID, 0), name
        assert _untouched(offs, sizes, 0)
        return
    assert (status, n) == (flacgpu.INDEX_OK, len(want)), name
    assert list(sizes[:n]) == want, name
    assert list(offs[:n]) == [int(v) for v in np.cumsum([0] + want)[:-1]], name
    assert _untouched(offs, sizes, n), "entries at and past n_frames were written"


def test_base_alignments(ctx):
    """The same stream at every offset of a 16-byte unit: the first chunk's lead changes with it."""
    c = dc.FRAME_CASES[0]
    _, raw = dc.golden_frames(c)
    for at in (0, 1, 9, 15, 16, 63, 64):
        status, n, offs, sizes = device_index(ctx, raw, c["bits"], c["rate"], at=at)
        assert status == 0 and list(sizes[:n]) == c["frame_bytes"], at


def test_cap_too_small(ctx):
    import flacgpu

    data = b"".join(ic.tiny_frames())
    want = ic.host_index(data)
    status, n, offs, sizes = device_index(ctx, data, 8, 44100, cap=len(want) - 1)
    assert (status, n) == (flacgpu.INDEX_TOO_SMALL, len(want))
    assert _untouched(offs, sizes, len(want) - 1), "written past cap"
    # exactly enough
    status, n, offs, sizes = device_index(ctx, data, 8, 44100, cap=len(want))
    assert (status, n) == (flacgpu.INDEX_OK, len(want)) and list(sizes[:n]) == want and _untouched(offs, sizes, n)
    # an invalid stream stays INVALID whatever the cap
    status, n, offs, sizes = device_index(ctx, data[:-1], 8, 44100, cap=3)
    assert (status, n) == (flacgpu.INDEX_INVALID, 0) and _untouched(offs, sizes, 0)


def test_argument_checks(ctx):
    L = ctx.lib
    buf = ctypes.create_string_buffer(64)
    assert L.flacgpu_flac_index_device(ctx.ctx, None, 8, 16, 0, buf, buf, 1, buf, None) == -2
    assert L.flacgpu_flac_index_device(ctx.ctx, buf, 8, 16, 0, None, buf, 1, buf, None) == -2
    assert L.flacgpu_flac_index_device(ctx.ctx, buf, 8, 16, 0, buf, None, 1, buf, None) == -2
    assert L.flacgpu_flac_index_device(ctx.ctx, buf, 8, 16, 0, buf, buf, 1, None, None) == -2
    assert L.flacgpu_flac_index_device(ctx.ctx, buf, 1 << 32, 16, 0, buf, buf, 1, buf, None) == -2


def test_index_feeds_the_device_decoder():
    import flacgpu

    torch, dev = _torch()
    c = next(c for c in dc.FRAME_CASES if c["name"] == "c1_44k16_stereo")
    _, raw = dc.golden_frames(c)
    pcm = make_golden.make_pcm(c["name"], c["channels"], c["bits"], c["rate"], c["n_samples"], c["stream_seed"])
    ref, _ = oracle_ref.decode_frames(raw, c["channels"], c["bits"], c["rate"], c["n_samples"], first_number=c["first_frame"])
    assert ref == pcm
    cap = len(raw) // 8 + 1
    host = np.full(1 + len(raw) + 16, 0xA5, dtype=np.uint8)
    host[1:1 + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    d_buf = torch.from_numpy(host).to(dev)
    d_off = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_fb = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_ir = torch.zeros(16, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with flacgpu.Decoder(c["channels"], c["bits"], c["rate"], device=0, max_frames=64, block_size=c["block"]) as d:
        d.flac_index_device(d_buf.data_ptr() + 1, len(raw), d_off.data_ptr(), d_fb.data_ptr(), cap, d_ir.data_ptr(),
                            stream_bits=c["bits"], stream_rate=c["rate"], stream=st)
        d.sync_check(st)
        ir = flacgpu.IndexResult.from_buffer_copy(d_ir.cpu().numpy().tobytes())
        assert ir.status == 0 and ir.n_frames == len(c["frame_bytes"])
        n = int(ir.n_frames)
        d_out = torch.full((len(pcm) + 64,), 0xA5, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        d_bad = torch.full((1,), 77, dtype=torch.int32, device=dev)
        d.decode_frames_device(d_buf.data_ptr() + 1, d_off.data_ptr(), d_fb.data_ptr(), n, d_res.data_ptr(),
                               d_bad.data_ptr(), d_pcm_out=d_out.data_ptr(), pcm_cap=len(pcm), stream=st)
        d.sync_check(st)
    out = d_out.cpu().numpy().tobytes()
    assert int(d_bad.item()) == 0 and out[:len(pcm)] == pcm and set(out[len(pcm):]) == {0xA5}


def _with_extra_block(flac: bytes, body: bytes) -> bytes:
    """The file with one more metadata block (PADDING, `body`) after its last one."""
    assert flac[:4] == b"fLaC"
    pos = 4
    while True:
        last, n = flac[pos] & 0x80, int.from_bytes(flac[pos + 1:pos + 4], "big")
        if last:
            break
        pos += 4 + n
    out = bytearray(flac)
    out[pos] &= 0x7F
    end = pos + 4 + n
    return bytes(out[:end]) + bytes([0x81]) + len(body).to_bytes(3, "big") + body + bytes(out[end:])


def test_decode_file_through_the_device_index():
    import flacgpu

    ch, bits, rate = 2, 16, 44100
    pcm = synth.synth_pcm(3 * 4096 + 555, ch, bits, rate, stream=4)  # the file of test_gpu_decode.test_decode_file
    flac = oracle_ref.encode_file(pcm, ch, bits, rate)
    odd = _with_extra_block(flac, bytes(7))
    assert flacgpu.flac_index(odd)[1] == flacgpu.flac_index(flac)[1] + 11
    for max_frames in (2, 64):
        with flacgpu.Decoder(ch, bits, rate, device=0, max_frames=max_frames) as d:
            d.set_timing(True)
            got, ok = d.decode_file(flac)
            assert got == pcm and ok
            launches, ms = d.kernel_time(flacgpu.K_INDEX)
            assert launches >= 1 and ms > 0
            got, ok = d.decode_file(odd)  # the frames start at an odd offset of the file
            assert got == pcm and ok
            bad = bytearray(flac)
            bad[8 + 18 + 5] ^= 0x40  # a byte of the STREAMINFO MD5
            got, ok = d.decode_file(bytes(bad))
            assert got == pcm and not ok
            # a corrupted frame byte: refused as before, by the C entry point itself
            first = flacgpu.flac_index(flac)[1]
            bad = bytearray(flac)
            bad[first + 1000] ^= 0x04
            out = ctypes.create_string_buffer(len(pcm) + 4096 * ch * 2)
            ns, md5_ok = ctypes.c_uint64(0), ctypes.c_int(0)
            rc = d.lib.flacgpu_decode_file(d.ctx, bytes(bad), len(bad), out, len(out), ctypes.byref(ns), ctypes.byref(md5_ok))
            assert rc == -2
