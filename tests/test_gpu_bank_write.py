"""The write side of a bank on the GPU: flacgpu_pcm_from_elements_device (k_elements_pcm),
FlacBank.from_tensors and FlacBank.file_bytes.

Everything compares bytes and bit patterns for equality; there is no tolerance.  The kernel is
compared with the host statement of its rule (flacgpu_pcm_from_elements_host, itself compared with
numpy in tests/test_quantize_host.py) over a guarded buffer; the banks with their own input, with
Encoder.encode_file of the same PCM (a path pinned to the oracle elsewhere), with the independent
verifier decoder (oracle/flac_decode.c) and with hashlib's MD5."""
import ctypes
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fuzz_blocks  # noqa: E402
import oracle_ref  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

I32, F32, F16, BF16 = range(4)
GUARD = 64
LENGTHS = (1, 2, 3, 4, 5, 255, 4095, 4097, 10000)


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _dtype(fmt):
    import torch

    return {I32: torch.int32, F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[fmt]


def _golden(name):
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        return f.read()


def _file(channels, bits, frames, rate, block=4096):
    """Golden bare frames with a STREAMINFO in front: a file."""
    import flacgpu

    return flacgpu.header_bytes(flacgpu.StreamInfo.new(rate, channels, bits, 0, block), True) + _golden(frames)


# ---- the kernel against the host statement -------------------------------------------------------
def _values(rng, count, fmt, bits):
    """`count` elements of fmt as a CPU torch tensor: ordinary values, ties, out-of-range values, NaN."""
    import torch

    if fmt == I32:
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        v = rng.integers(lo, hi + 1, count)
        wide = rng.integers(-(1 << 31), 1 << 31, count)
        v = np.where(rng.random(count) < 0.1, wide, v)
        return torch.from_numpy(v.astype(np.int32))
    unit = 2.0 ** -(bits - 1)
    v = rng.random(count) * 2.4 - 1.2
    ties = (rng.integers(-(1 << min(bits - 1, 20)), 1 << min(bits - 1, 20), count) + 0.5) * unit
    pick = rng.random(count)
    v = np.where(pick < 0.2, ties, v)
    special = np.array([1.0, -1.0, np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0 - unit, -1.0 - unit, 3.4e38, 1e-40])
    v = np.where(pick > 0.95, special[rng.integers(0, len(special), count)], v)
    return torch.from_numpy(v.astype(np.float32)).to(_dtype(fmt))


def _patterns(x):
    """A CPU torch tensor's elements as a numpy array of their bit patterns."""
    import torch

    return x.view(torch.int32 if x.element_size() == 4 else torch.int16).numpy().view(np.uint32 if x.element_size() == 4 else np.uint16)


@pytest.fixture(scope="module")
def encoders():
    import flacgpu

    made = {}

    def get(C, bits, rate=44100):
        if (C, bits, rate) not in made:
            made[(C, bits, rate)] = flacgpu.Encoder(C, bits, rate, device=0, max_frames=4)
        return made[(C, bits, rate)]

    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("fmt", [I32, F32, F16, BF16])
@pytest.mark.parametrize("C,bits", [(1, 8), (2, 16), (3, 24), (8, 32), (1, 24)])
def test_kernel_equals_the_host_statement(encoders, C, bits, fmt, planar):
    import flacgpu

    torch, dev = _torch()
    enc = encoders(C, bits)
    rng = np.random.default_rng([C, bits, fmt, int(planar)])
    B, esz = bits // 8, flacgpu.ELEMENT_BYTES[fmt]
    keep, addrs, strides, offs, want, want_clipped, at = [], [], [], [], [], [], 0
    for s, T in enumerate(LENGTHS):
        lead = (1, 3)[s % 2]  # the view starts 1 or 3 elements into its allocation
        stride = T + (0, 5, 2)[s % 3] if planar else T
        count = C * stride if planar else T * C
        host = _values(rng, count, fmt, bits)
        alloc = torch.zeros(lead + count, dtype=_dtype(fmt), device=dev)
        alloc[lead:] = host.to(dev)
        keep.append(alloc)
        addrs.append(alloc.data_ptr() + lead * esz)
        strides.append(stride)
        p = _patterns(host).reshape((C, stride) if planar else (T, C))
        pcm, clipped = flacgpu.pcm_from_elements_host(p, bits, fmt, planar=planar, samples=T, plane_stride=stride if planar else None)
        assert len(pcm) == (T * C * B + 3) // 4 * 4 and pcm[T * C * B:] == bytes(len(pcm) - T * C * B)
        offs.append(at)
        at += len(pcm)
        want.append(pcm)
        want_clipped.append(clipped)
    if fmt != I32 or bits < 32:
        assert sum(want_clipped) > 0
    buf = torch.full((GUARD + at + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_clip = torch.full((len(LENGTHS),), -7, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    enc.pcm_from_elements_device(addrs, list(LENGTHS), strides if planar else None, fmt, flacgpu.DELIVER_PLANAR if planar else 0,
                                 buf.data_ptr() + GUARD, offs, at, d_clip.data_ptr(), stream=st)
    enc.sync_check(st)
    got = buf.cpu().numpy().tobytes()
    assert got[:GUARD] == b"\xA5" * GUARD and got[GUARD + at:] == b"\xA5" * GUARD
    for s, T in enumerate(LENGTHS):
        assert got[GUARD + offs[s]:GUARD + offs[s] + len(want[s])] == want[s], (s, T)
    assert got[GUARD:GUARD + at] == b"".join(want)
    assert d_clip.cpu().tolist() == want_clipped


def test_device_call_refuses_on_a_context(encoders):
    """The refusals that need a context to be reached: a decode-only one, and the checks behind it."""
    import flacgpu

    torch, dev = _torch()
    enc = encoders(2, 16)
    x = torch.zeros(64, dtype=torch.float32, device=dev)
    buf = torch.full((256,), 0xA5, dtype=torch.uint8, device=dev)
    clip = torch.zeros(2, dtype=torch.int64, device=dev)
    good = ([x.data_ptr(), x.data_ptr()], [8, 8], [8, 8], F32, 1, buf.data_ptr(), [0, 32], 64, clip.data_ptr())
    enc.pcm_from_elements_device(*good)
    enc.sync_check()
    for i, bad in ((6, [0, 30]), (6, [0, 28]), (7, 63), (2, [8, 7]), (3, 4), (4, 2), (0, [x.data_ptr(), 0])):
        args = list(good)
        args[i] = bad
        with pytest.raises(flacgpu.FlacGpuError) as e:
            enc.pcm_from_elements_device(*args)
        assert e.value.code == -2, (i, bad)
    with flacgpu.Decoder(2, 16, 44100, device=0, max_frames=4, block_size=8192) as d:  # decode-only
        with pytest.raises(flacgpu.FlacGpuError) as e:
            d.pcm_from_elements_device(*good)
        assert e.value.code == -2
    assert buf.cpu().numpy().tobytes()[64:] == b"\xA5" * 192


# ---- integer round trip and file identity ---------------------------------------------------------
def _int_streams(C, bits, block, seed):
    """int64 [T, C] streams of one sample, a block less one, a block, and three blocks and a tail."""
    rng = np.random.default_rng(seed)
    out = []
    for k, T in enumerate((1, block - 1, block, 3 * block + 37)):
        parts, left = [], T
        while left:
            n = min(left, block)
            parts.append(fuzz_blocks.block(rng, n, C, bits, fuzz_blocks.ALL_KINDS[(k + len(parts)) % len(fuzz_blocks.ALL_KINDS)]))
            left -= n
        out.append(np.concatenate(parts, axis=0))
    return out


@pytest.mark.parametrize("C,bits,rate,block,prediction", [(2, 16, 44100, 4096, 0), (2, 24, 96000, 4096, 0), (1, 8, 22050, 4096, 0),
                                                           (8, 32, 192000, 4096, 0), (2, 16, 44100, 1152, 0),
                                                           (2, 16, 48000, 4096, 8)])
def test_integers_come_back_and_files_are_the_encoders(C, bits, rate, block, prediction):
    import flacbank
    import flacgpu

    torch, dev = _torch()
    streams = _int_streams(C, bits, block, [C, bits, block, prediction])
    tensors = [torch.from_numpy(np.ascontiguousarray(x.T).astype(np.int32)) for x in streams]  # [C, T], on the CPU: moved
    tensors[2] = tensors[2].to(dev)
    with flacbank.FlacBank.from_tensors(tensors, rate, bits=bits, block_size=block, prediction=prediction, max_frames=64) as b, \
            flacgpu.Encoder(C, bits, rate, device=0, max_frames=16, block_size=block, lpc_order=prediction) as enc:
        assert b.samples == [len(x) for x in streams] and b.clipped == [0] * 4
        assert (b.channels, b.bits, b.sample_rates) == (C, bits, [rate] * 4)
        for i, x in enumerate(streams):
            got, n = b.crops([i], [0], len(x), dtype=torch.int32)
            assert n == [len(x)] and (got[0].cpu().numpy() == x.T).all(), i
            pcm = synth.to_pcm_bytes(x, bits)
            flac = b.file_bytes(i)
            assert flac == enc.encode_file(pcm), i
            dec, sizes = oracle_ref.decode_frames(flac[73:], C, bits, rate, len(x))  # the independent decoder
            assert dec == pcm and len(sizes) == (len(x) + block - 1) // block
            assert flac[26:42] == hashlib.md5(pcm).digest()  # the MD5 in STREAMINFO
        assert b.compressed_bytes == sum(len(b.file_bytes(i)) - 73 for i in range(4))


def test_interleaved_and_batched_inputs():
    """[T, C] tensors with planar=False and one [N, C, T] tensor give the banks the [C, T] list gives."""
    import flacbank

    torch, dev = _torch()
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-30000, 30000, (3, 2, 5000)).astype(np.int32)).to(dev)
    with flacbank.FlacBank.from_tensors(list(x), 44100, max_frames=64) as a, \
            flacbank.FlacBank.from_tensors(x, 44100, max_frames=64) as b, \
            flacbank.FlacBank.from_tensors(x.transpose(1, 2).contiguous(), 44100, planar=False, max_frames=64) as c, \
            flacbank.FlacBank.from_tensors([x[i].transpose(0, 1) for i in range(3)], 44100, planar=False, max_frames=64) as d, \
            flacbank.FlacBank.from_tensors([x[i, :, 100:4900] for i in range(3)], 44100, max_frames=64) as e:
        files = [a.file_bytes(i) for i in range(3)]
        for other in (b, c, d):  # d's sources are not contiguous as [T, C]: they are copied
            assert [other.file_bytes(i) for i in range(3)] == files
        got, n = e.crops([0, 1, 2], [0, 0, 0], 4800, dtype=torch.int32)  # planes 5000 apart: a plane stride
        assert n == [4800] * 3 and torch.equal(got, x[:, :, 100:4900])


# ---- float round trip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits,rate", [("c1_44k16_stereo.flac", 16, 44100), ("c3_96k24_stereo.flac", 24, 96000)])
def test_float_crops_come_back_bit_for_bit(name, bits, rate):
    import flacbank

    torch, dev = _torch()
    with flacbank.FlacBank([_file(2, bits, name, rate)], max_frames=64) as src:
        T = src.samples[0]
        x, n = src.crops([0], [0], T)
        assert n == [T] and x.dtype == torch.float32
        with flacbank.FlacBank.from_tensors([x[0], x[0, :, 1000:3001]], rate, bits=bits, max_frames=64) as b:
            assert b.clipped == [0, 0] and b.samples == [T, 2001]
            y, n = b.crops([0], [0], T)
            assert n == [T] and torch.equal(y.view(torch.int32), x.view(torch.int32))
            z, _ = b.crops([1], [0], 2001)
            assert torch.equal(z.view(torch.int32), x[:, :, 1000:3001].contiguous().view(torch.int32))
            assert b.file_bytes(0)[73:] == _golden(name)  # the same samples, the same encoder: the golden frames


def test_clipped_counts_the_elements_the_clamp_changed():
    import flacbank

    torch, _ = _torch()
    x = torch.tensor([[1.0, 0.5, 1.0, -1.5, float("nan"), 0.25, -1.0]], dtype=torch.float32)
    quiet = torch.tensor([[0.5, -0.5, 0.999]], dtype=torch.float32)
    with flacbank.FlacBank.from_tensors([quiet, x], 8000, bits=16, max_frames=4) as b:
        assert b.clipped == [0, 4]
        got, _ = b.crops([1], [0], 7, dtype=torch.int32)
        assert got[0, 0].tolist() == [32767, 16384, 32767, -32768, 0, 8192, -32768]


# ---- the bank is a bank --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_banks():
    import flacbank

    torch, dev = _torch()
    rng = np.random.default_rng(11)
    t = np.arange(9000)
    x = [(8000 * np.sin(t[:n] * f) + rng.integers(-200, 200, n)).astype(np.int32) for n, f in ((9000, 0.05), (5000, 0.3))]
    tensors = [torch.from_numpy(np.stack([v, -v // 2])).to(dev) for v in x]
    b = flacbank.FlacBank.from_tensors(tensors, 44100, max_frames=64)
    again = flacbank.FlacBank([b.file_bytes(i) for i in range(2)], max_frames=64)
    yield b, again
    b.close()
    again.close()


def test_a_bank_of_its_own_files_returns_the_same(two_banks):
    torch, _ = _torch()
    b, again = two_banks
    assert again.samples == b.samples and again.sample_rates == b.sample_rates and again.clipped is None
    files_, starts = [0, 1, 0, 1], [0, 100, 8000, 4990]
    for kw in (dict(), dict(dtype=torch.int32), dict(rate=48000), dict(dtype=torch.bfloat16, planar=False)):
        (x, n), (y, m) = b.crops(files_, starts, 2000, **kw), again.crops(files_, starts, 2000, **kw)
        assert n == m and torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                                      y.view(torch.int16 if y.element_size() == 2 else torch.int32)), kw
    (x, n), (y, m) = b.features(files_, starts, 4, 64, 16), again.features(files_, starts, 4, 64, 16)
    assert n == m and x.shape == (4, 2, 33, 4) and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert [again.file_bytes(i) for i in range(2)] == [b.file_bytes(i) for i in range(2)]


def test_two_rates_in_one_call():
    import flacbank
    import flacgpu

    torch, dev = _torch()
    rng = np.random.default_rng(12)
    x = [rng.integers(-20000, 20000, (1, n)).astype(np.int32) for n in (6000, 5000, 300)]
    rates = [44100, 48000, 44100]
    with flacbank.FlacBank.from_tensors([torch.from_numpy(v) for v in x], rates, max_frames=64) as b:
        assert b.sample_rates == rates and b.samples == [6000, 5000, 300]
        assert b.samples_at(48000) == [(6000 * 160 + 146) // 147, 5000, (300 * 160 + 146) // 147]
        got, n = b.crops([0, 1, 2], [1000, 1000, 0], 400, rate=48000)
        assert n == [400, 400, (300 * 160 + 146) // 147]
        f = [v[0].astype(np.float32) * np.float32(2.0 ** -15) for v in x]
        assert (got[1, 0].cpu().numpy().view(np.uint32) == f[1][1000:1400].view(np.uint32)).all()  # at its own rate
        for w, i, start in ((0, 0, 1000), (2, 2, 0)):
            want = flacgpu.resample_f32_host(f[i], 44100, 48000, start, 400)
            assert (got[w, 0, :len(want)].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all(), w
        for i in range(3):  # the rate is in every file's STREAMINFO and frame headers
            si, _, _ = flacgpu.flac_index(b.file_bytes(i))
            assert int(si.sample_rate) == rates[i] and int(si.interchannel_samples) == x[i].shape[1]


def test_groups_cut_by_the_scratch_budget_give_the_same_files(monkeypatch):
    import flacbank
    import flacgpu

    torch, dev = _torch()
    rng = np.random.default_rng(13)
    lengths = [100, 120, 20000, 90, 110]
    tensors = [torch.from_numpy(rng.integers(-9000, 9000, (2, n)).astype(np.int32)).to(dev) for n in lengths]
    cfg = flacgpu.Config.default(2, 16, 44100)
    image = (flacgpu.load_library().flacgpu_frame_bound_bytes(ctypes.byref(cfg)) + 16 + 15) // 16 * 16
    budget = 2 * (120 * 4 + image)  # two short tensors fit, the long one (five frames) does not fit alone
    assert 20000 * 4 + 5 * image > budget
    calls = []
    real = flacgpu.Encoder.pcm_from_elements_device

    def counted(self, d_src, *a, **k):
        calls.append(len(d_src))
        return real(self, d_src, *a, **k)

    monkeypatch.setattr(flacgpu.Encoder, "pcm_from_elements_device", counted)
    with flacbank.FlacBank.from_tensors(tensors, 44100, max_frames=64) as one:
        assert calls == [5]
        whole = [one.file_bytes(i) for i in range(5)]
    del calls[:]
    with flacbank.FlacBank.from_tensors(tensors, 44100, max_frames=64, scratch_bytes=budget) as cut:
        assert calls == [2, 1, 2]
        assert [cut.file_bytes(i) for i in range(5)] == whole
        got, n = cut.crops([2, 4], [19000, 0], 110, dtype=torch.int32)
        assert n == [110, 110] and torch.equal(got[0], tensors[2][:, 19000:19110]) and torch.equal(got[1], tensors[4])


def test_from_tensors_runs_on_the_callers_stream():
    """The source is filled by a kernel queued on a non-default stream right before the build, with no
    synchronisation of the test's own in between: the bank holds the filled values."""
    import flacbank

    torch, dev = _torch()
    rng = np.random.default_rng(14)
    vals = torch.from_numpy(rng.integers(-30000, 30000, (2, 50000)).astype(np.int32)).to(dev)
    x = torch.zeros_like(vals)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        x.add_(vals)
        b = flacbank.FlacBank.from_tensors([x], 44100, max_frames=64)
        got, n = b.crops([0], [0], 50000, dtype=torch.int32)
    s.synchronize()
    assert n == [50000] and torch.equal(got[0], vals)
    b.close()


# ---- banks built from files ---------------------------------------------------------------------------
def test_file_bytes_of_a_bank_built_from_files_are_the_files():
    import flacbank

    files = [_golden("c1_44k16_stereo_file.flac"), _file(2, 16, "c1_44k16_stereo.flac", 44100), _file(2, 16, "specials.flac", 44100)]
    with flacbank.FlacBank(files, max_frames=64) as b:
        assert b.clipped is None
        assert [b.file_bytes(i) for i in range(3)] == files
        with pytest.raises(ValueError):
            b.file_bytes(3)
    with pytest.raises(ValueError, match="closed"):
        b.file_bytes(0)
