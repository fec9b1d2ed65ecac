"""Sample windows delivered as tensor elements on the GPU: flacgpu_decode_windows_device_as and
FlacBank.

Everything compares bit patterns for equality; there is no tolerance.  The expected elements
are the generators' own PCM (synth.synth_pcm for the encoded files, frame_grammar.case_pcm for the
grammar streams) turned into integers here with numpy (3-byte samples sign-extended by hand) and
converted by numpy (f32, f16) or torch on the CPU (bf16); they are never an output of the decoder.
Every output buffer is filled with 0xA5 before the call and compared whole, so a stray write
anywhere fails.  The files are those of test_gpu_windows.py: stereo 16-bit, blocks of 256,
[64, 1, 3, 70, 0] frames, decoded by a context that holds 64 frames per call.

Mutation counts (each mutant of k_window_elements<false> / its host side fails tests here): DESIGN.md 7b."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import flac_bits  # noqa: E402
import frame_grammar as fg  # noqa: E402
import synth  # noqa: E402
from window_helpers import (BITS, BLOCK, CH, FRAMES, GUARD, NONE, PER, RATE, Resident, _bare, _blocks, _samples,  # noqa: E402,F401
                            _torch, cover)
from window_helpers import ctx, files, resident  # noqa: E402,F401  (fixtures: the five stereo 16-bit files)

pytestmark = pytest.mark.gpu

DEC_RANGE = 7
U64 = (1 << 64) - 1
I32, F32, F16, BF16 = range(4)
PLANAR, PAD = 1, 2
ESZ = {I32: 4, F32: 4, F16: 2, BF16: 2}
FORMAT_NAMES = {I32: "i32", F32: "f32", F16: "f16", BF16: "bf16"}


# ---- the expectation: PCM bytes -> integers -> elements, by numpy and torch-CPU only ------------
def ints(pcm, channels, bits):
    """Interleaved little-endian PCM bytes -> int32 [samples, channels]."""
    B = bits // 8
    raw = np.frombuffer(pcm, dtype=np.uint8).reshape(-1, B).astype(np.uint32)
    v = np.zeros(len(raw), dtype=np.uint32)
    for k in range(B):
        v |= raw[:, k] << np.uint32(8 * k)
    if B < 4:  # sign-extend by hand
        v = np.where(v & np.uint32(1 << (bits - 1)), v | np.uint32((0xFFFFFFFF << bits) & 0xFFFFFFFF), v)
    return v.astype(np.uint32).view(np.int32).reshape(-1, channels)


def elements(x, bits, fmt):
    """int32 array -> the elements' bit patterns (uint32 or uint16), same shape."""
    import torch

    if fmt == I32:
        return x.view(np.uint32)
    f32 = x.astype(np.float32) * np.float32(2.0 ** -(bits - 1))
    if fmt == F32:
        return f32.view(np.uint32)
    if fmt == F16:
        return f32.astype(np.float16).view(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(f32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def need(take, count, flags):
    return count if flags & (PLANAR | PAD) else take


def layout(sizes, fmt):
    """Regions of the given element counts, one after another with gaps, so that the byte address
    of region w takes every multiple of the element size mod 16 in turn -> ([offset], bytes)."""
    per16 = 16 // ESZ[fmt]
    offs, at = [], 1
    for w, n in enumerate(sizes):
        at += (w % per16 - at) % per16
        offs.append(at)
        at += n + 3
    return offs, ((at * ESZ[fmt] + 64) // 16) * 16


def check_delivery(out, res, windows, blocks_of, ints_of, channels, bits, fmt, flags, offsets, caps, expect_status=None):
    """Every result and every element of the output buffer, for windows whose expected status is
    OK but for those in expect_status {window: (status, first_bad_frame, first_bad_status)}."""
    expect_status = expect_status or {}
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    C = channels
    for w, ((s, start, count), r) in enumerate(zip(windows, res)):
        first, frames, take = cover(blocks_of[s], start, count)
        if w in expect_status:
            st, bad, bad_st = expect_status[w]
            assert (r.status, r.n_samples, r.first_bad_frame, r.first_bad_status) == (st, 0, bad, bad_st), w
            continue
        assert (r.status, r.n_samples, r.n_frames, r.first_bad_frame, r.first_bad_status) == (0, take, frames, NONE, 0), w
        if frames:
            assert r.first_frame == first, w
        assert need(take, count, flags) * C <= caps[w]
        el = elements(ints_of[s][start:start + take], bits, fmt)  # [take, C]
        o = offsets[w]
        if flags & PLANAR:
            for c in range(C):
                want[o + c * count:o + c * count + take] = el[:, c]
                if flags & PAD:
                    want[o + c * count + take:o + (c + 1) * count] = 0
        else:
            want[o:o + take * C] = el.reshape(-1)
            if flags & PAD:
                want[o + take * C:o + count * C] = 0
    got = np.frombuffer(out, dtype=dt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]  # elements, and 0xA5 everywhere else


# ---- the stereo files ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def file_ints(files):
    """The files' samples as int32 [samples, channels]: computed once, shared, never changed."""
    out = {i: ints(pcm, CH, BITS) for i, (_, pcm) in enumerate(files)}
    for v in out.values():
        v.setflags(write=False)
    return out


def forty_windows():
    w = [
        (0, 300, 50),                 # inside one frame
        (0, 512, 256),                # exactly one frame
        (0, 767, 2),                  # the last sample of a frame and the first of the next
        (0, 0, _samples(0)),          # a whole file
        (2, 500, 1000),               # clipped by the end of the file with the short last frame
        (2, _samples(2), 10),         # at the end
        (2, _samples(2) + 88, 10),    # past the end
        (2, 5, 0),                    # no samples
        (3, 1000, 5000), (3, 3000, 5000), (3, 4000, 9000),  # three overlapping windows
        (4, 0, 100),                  # the file with no frames
        (1, 0, 256), (1, 255, 1), (1, 0, (1 << 64) - 1), (2, 511, (1 << 64) - 1),
    ]
    rng = random.Random("windows")
    while len(w) < 40:
        s = rng.choice((0, 1, 2, 3))
        start = rng.randrange(_samples(s))
        w.append((s, start, rng.choice((1, 2, 255, 256, 257, 700))))
    return w


@pytest.mark.parametrize("pad", [False, True], ids=["nopad", "pad"])
@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("fmt", [I32, F32, F16, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_forty_windows(resident, file_ints, fmt, planar, pad):
    flags = (PLANAR if planar else 0) | (PAD if pad else 0)
    windows = forty_windows()
    blocks_of = {i: _blocks(i) for i in range(len(FRAMES))}
    takes = [cover(blocks_of[s], start, count) for s, start, count in windows]
    assert sum(t[1] for t in takes) > 128  # the cut of the covering frames crosses two chunk boundaries
    # a capacity of exactly what the window needs; the two windows of 2^64 - 1 samples get what they deliver
    huge = [w for w, (_, _, count) in enumerate(windows) if count == U64]
    assert huge == [14, 15]
    sizes = [CH * (t[2] if w in huge else need(t[2], windows[w][2], flags)) for w, t in enumerate(takes)]
    offs, size = layout(sizes, fmt)
    assert {(o * ESZ[fmt]) % 16 for o in offs} == set(range(0, 16, ESZ[fmt]))  # every destination alignment
    out, res = resident.deliver(windows, fmt, flags, offs, sizes, size)
    # under PLANAR or PAD the layout is the stated count's, which no capacity holds: TOO_SMALL;
    # interleaved without padding they are delivered clipped
    expect = {w: (3, NONE, 0) for w in huge} if flags else {}
    assert [r.status for r in res] == [3 if w in expect else 0 for w in range(len(windows))]
    check_delivery(out, res, windows, blocks_of, file_ints, CH, BITS, fmt, flags, offs, sizes, expect_status=expect)
    # the clipped window, the windows at and past the end, without samples and of the empty file
    assert [r.n_samples for r in res[4:8]] == [112, 0, 0, 0] and res[11].n_samples == 0 and res[11].n_frames == 0
    if pad:  # padded windows with no samples are all zeros (check_delivery compared them; here: that they exist)
        dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
        got = np.frombuffer(out, dtype=dt)
        for w in (5, 6, 11):
            assert windows[w][2] > 0 and (got[offs[w]:offs[w] + CH * windows[w][2]] == 0).all()


def test_capacity_one_element_short_and_bad_index_write_nothing(ctx, resident, files, file_ints):
    """PAD set: a TOO_SMALL window (one element short) and a BAD_INDEX window (a stream with no
    frame at offset 0), each between two good neighbours, write nothing; the results are the
    byte call's."""
    blocks_of = {i: _blocks(i) for i in range(5)}
    windows = [(0, 100, 300), (3, 4000, 600), (1, 3, 200)]
    for flags in (PAD, PAD | PLANAR):
        sizes = [300 * CH, 600 * CH - 1, 200 * CH]
        offs, size = layout(sizes, F32)
        out, res = resident.deliver(windows, F32, flags, offs, sizes, size)
        assert [r.status for r in res] == [0, 3, 0]
        check_delivery(out, res, windows, blocks_of, file_ints, CH, BITS, F32, flags, offs, sizes, expect_status={1: (3, NONE, 0)})
    _, ref = resident.decode(windows, [0, 2048, 8192], [300 * PER, 600 * PER - 1, 200 * PER], 16384)
    assert [_fields(r) for r in res] == [_fields(r) for r in ref]
    # one element more fits
    sizes = [300 * CH, 600 * CH, 200 * CH]
    offs, size = layout(sizes, F32)
    out, res = resident.deliver(windows, F32, PAD | PLANAR, offs, sizes, size)
    check_delivery(out, res, windows, blocks_of, file_ints, CH, BITS, F32, PAD | PLANAR, offs, sizes)

    bad = b"\x00" * 7 + _bare(files[1][0])  # no frame at offset 0
    r = Resident(ctx, [(_bare(files[1][0]), BITS, RATE), (bad, BITS, RATE), (_bare(files[2][0]), BITS, RATE)])
    assert r.index == [(0, 1), (1, 0), (0, 3)]
    windows = [(0, 10, 100), (1, 0, 100), (2, 300, 600)]
    sizes = [100 * CH, 100 * CH, 600 * CH]
    offs, size = layout(sizes, BF16)
    out, res = r.deliver(windows, BF16, PAD | PLANAR, offs, sizes, size)
    check_delivery(out, res, windows, {0: _blocks(1), 1: [], 2: _blocks(2)}, {0: file_ints[1], 2: file_ints[2]}, CH, BITS, BF16,
                   PAD | PLANAR, offs, sizes, expect_status={1: (1, NONE, 0)})
    _, ref = r.decode(windows, [0, 1024, 2048], [100 * PER, 100 * PER, 600 * PER], 8192)
    assert [_fields(x) for x in res] == [_fields(x) for x in ref]


def _fields(r):
    return (r.n_samples, r.first_frame, r.n_frames, r.status, r.first_bad_frame, r.first_bad_status)


# ---- the grammar streams ---------------------------------------------------------------------------
def _case(name):
    return next(c for c in fg.cases() if c["name"] == name)


def _grammar_deliver(c, windows, fmt, flags, block_size=4096, expect_status=None, offsets=None, compare_with_bytes=False):
    """The grammar case as the one stream of a context of its own; windows [(0, start, count)]."""
    import flacgpu

    C, bits = c["channels"], c["bits"]
    blocks = [f["block"] for f in c["frames"]]
    x = ints(fg.case_pcm(c), C, bits)
    with flacgpu.Decoder(C, bits, c["rate"], device=0, max_frames=64, block_size=block_size) as d:
        r = Resident(d, [(fg.case_bytes(c), bits, c["rate"])])
        assert r.index == [(0, len(blocks))] and r.totals == [sum(blocks)]
        sizes = [C * need(cover(blocks, s, n)[2], n, flags) for _, s, n in windows]
        offs, size = offsets(sizes) if offsets else layout(sizes, fmt)
        out, res = r.deliver(windows, fmt, flags, offs, sizes, size)
        if compare_with_bytes:
            per = C * bits // 8
            caps = [n * per for _, _, n in windows]
            _, ref = r.decode(windows, [sum(caps[:w]) for w in range(len(caps))], caps, sum(caps) + 16)
            assert [_fields(a) for a in res] == [_fields(b) for b in ref]
    if expect_status is None:
        assert [v.status for v in res] == [0] * len(windows)
    check_delivery(out, res, windows, {0: blocks}, {0: x}, C, bits, fmt, flags, offs, sizes, expect_status=expect_status)
    return res, x


@pytest.mark.parametrize("fmt,flags", [(F32, 0), (BF16, PLANAR | PAD)], ids=["f32", "bf16"])
def test_alignment_sweep_mono_8_bit(fmt, flags):
    """per = 1: a window for every (source mod 16, destination element within 16 bytes) pair at
    eleven lengths, in one call.  The source starts `skip` bytes into 16-byte aligned scratch and
    skip = start here (frame 0), so start mod 16 is the source alignment; the longest windows run
    on into frame 1."""
    c = _case("seed3_1x8")
    assert [f["block"] for f in c["frames"]][:2] == [1152, 1024]
    windows, dst = [], []
    for sa in range(16):
        for da in range(16 // ESZ[fmt]):
            for n in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 47):
                start = 1104 + sa
                assert start % 16 == sa
                windows.append((0, start, n))
                dst.append(64 * len(dst) + da)
    assert len(windows) == 16 * (16 // ESZ[fmt]) * 11 and any(s + n > 1152 for _, s, n in windows)
    _grammar_deliver(c, windows, fmt, flags, offsets=lambda sizes: (dst, (64 * len(dst) + 64) * ESZ[fmt]))


@pytest.mark.parametrize("flags", [0, PLANAR | PAD], ids=["interleaved", "planar_pad"])
@pytest.mark.parametrize("fmt", [I32, F32, F16], ids=lambda f: FORMAT_NAMES[f])
def test_24_bit_mono(fmt, flags):
    c = _case("waste_and_unary")  # blocks 128, 192, 1152, 256, 100; per = 3: two tiles for the whole stream
    windows = [(0, 0, 1828), (0, 127, 2), (0, 5, 7), (0, 319, 1153), (0, 1700, 500), (0, 1471, 2), (0, 1828, 3)]
    res, x = _grammar_deliver(c, windows, fmt, flags)
    assert res[4].n_samples == 128 and res[6].n_samples == 0
    assert x.min() < -(1 << 16) and x.max() > (1 << 16)  # samples that need their third byte


@pytest.mark.parametrize("flags", [0, PLANAR | PAD], ids=["interleaved", "planar_pad"])
@pytest.mark.parametrize("fmt", [F32, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_eight_channels_32_bit(fmt, flags):
    """per = 32, the two-round reconstruct; planar planes of length 1, 2, 100 (18 of them samples) and 5113."""
    c = _case("eight_by_32")  # blocks 1000, 4096, 17
    windows = [(0, 999, 2), (0, 0, 5113), (0, 5095, 100), (0, 1003, 10), (0, 3, 1)]
    res, x = _grammar_deliver(c, windows, fmt, flags)
    assert res[2].n_samples == 18
    big = x[np.abs(x.astype(np.int64)) >= (1 << 24)]
    assert (big.astype(np.float32).astype(np.float64) != big.astype(np.float64)).sum() > 100  # inexact int -> f32


def _odd_channel_cases():
    """Grammar cases with an odd channel count above 1, picked by that field: the first, and the one
    with the most bytes per sample."""
    odd = [c for c in fg.cases() if c["channels"] > 1 and c["channels"] % 2 == 1]
    assert odd
    widest = max(odd, key=lambda c: c["channels"] * c["bits"])
    return [odd[0]] + ([widest] if widest is not odd[0] else [])


@pytest.mark.parametrize("flags", [0, PLANAR, PLANAR | PAD], ids=["interleaved", "planar", "planar_pad"])
def test_odd_channel_counts(flags):
    for c in _odd_channel_cases():
        total = sum(f["block"] for f in c["frames"])
        odd_len = next(n for n in (total - 2, total - 3, total - 4, total - 5) if n % 4 and n % 8 and n > 8)
        windows = [(0, 0, 1), (0, 1, odd_len), (0, total // 2, 1), (0, 3, 7), (0, 0, total), (0, total - 1, 6)]
        for fmt in (F32, F16):
            _grammar_deliver(c, windows, fmt, flags)


def test_bad_frame_writes_nothing_with_pad():
    """The third frame (1152 samples) is above the context's block size of 256: the windows that
    touch it are BAD_FRAME and write nothing, padding included; their neighbours are delivered.
    The results are the byte call's."""
    c = _case("waste_and_unary")
    assert [f["block"] for f in c["frames"]] == [128, 192, 1152, 256, 100]
    windows = [(0, 100, 220), (0, 300, 100), (0, 1482, 300), (0, 320, 1), (0, 1472, 356), (0, 1471, 1), (0, 100, 220)]
    bad = {1: (2, 2, DEC_RANGE), 3: (2, 2, DEC_RANGE), 5: (2, 2, DEC_RANGE)}
    for flags in (PAD, PAD | PLANAR):
        res, _ = _grammar_deliver(c, windows, F32, flags, block_size=256, expect_status=bad, compare_with_bytes=True)
        assert [r.status for r in res] == [0, 2, 0, 2, 0, 2, 0]


# ---- FlacBank ----------------------------------------------------------------------------------------
def _torch_dtypes():
    import torch

    return {I32: torch.int32, F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}


def _bits_of(x, fmt):
    """A tensor's bit patterns as a numpy array."""
    import torch

    return x.cpu().contiguous().view(torch.int32 if ESZ[fmt] == 4 else torch.int16).numpy().view(
        np.uint32 if ESZ[fmt] == 4 else np.uint16)


CROPS = [(0, 300), (2, 600), (3, 4000), (1, 250), (4, 0), (2, 668), (3, 17919 - 300), (0, 16383)]
LENGTH = 300


def _expected_crops(file_ints, fmt, planar):
    want = np.zeros((len(CROPS), LENGTH, CH), dtype=np.uint32 if ESZ[fmt] == 4 else np.uint16)
    n = []
    for w, (f, start) in enumerate(CROPS):
        el = elements(file_ints[f][start:start + LENGTH], BITS, fmt)
        want[w, :len(el)] = el
        n.append(len(el))
    return (want.transpose(0, 2, 1) if planar else want), n


@pytest.fixture(scope="module")
def bank(files):
    import flacbank

    with flacbank.FlacBank([f for f, _ in files], device=0, max_frames=64) as b:
        yield b


def test_flacbank_properties(bank, files):
    import flacgpu

    assert (bank.channels, bank.bits, bank.sample_rates) == (CH, BITS, [RATE] * len(FRAMES))
    assert bank.samples == [_samples(i) for i in range(len(FRAMES))]
    assert bank.samples == [flacgpu.flac_index(f)[0].interchannel_samples for f, _ in files]  # STREAMINFO's
    assert bank.compressed_bytes == sum(len(_bare(f)) for f, _ in files)


@pytest.mark.parametrize("pad", [True, False], ids=["pad", "memset"])
@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [I32, F32, F16, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_flacbank_crops(bank, file_ints, fmt, planar, pad):
    x, n = bank.crops([c[0] for c in CROPS], [c[1] for c in CROPS], LENGTH, dtype=_torch_dtypes()[fmt], planar=planar, pad=pad)
    want, want_n = _expected_crops(file_ints, fmt, planar)
    assert n == want_n and want_n[1] == 12 and want_n[3] == 6 and want_n[4] == 0 and want_n[5] == 0 and want_n[7] == 1
    assert tuple(x.shape) == ((len(CROPS), CH, LENGTH) if planar else (len(CROPS), LENGTH, CH))
    assert x.dtype == _torch_dtypes()[fmt] and x.is_contiguous()
    assert (_bits_of(x, fmt) == want).all()


def test_flacbank_out_is_reused(bank, file_ints):
    torch, dev = _torch()
    files_, starts = [c[0] for c in CROPS], [c[1] for c in CROPS]
    buf = torch.full((len(CROPS), CH, LENGTH), 7.0, dtype=torch.float32, device=dev)
    x, n, statuses = bank.crops(files_, starts, LENGTH, out=buf, strict=False)
    assert x is buf and statuses == [0] * len(CROPS)
    assert (_bits_of(buf, F32) == _expected_crops(file_ints, F32, True)[0]).all()
    buf.fill_(7.0)
    x, _ = bank.crops(files_, starts, LENGTH, out=buf, pad=False)  # the memset form clears the old contents too
    assert x is buf and (_bits_of(buf, F32) == _expected_crops(file_ints, F32, True)[0]).all()
    for wrong in (torch.empty((len(CROPS), LENGTH, CH), dtype=torch.float32, device=dev),
                  torch.empty((len(CROPS), CH, LENGTH), dtype=torch.float16, device=dev),
                  torch.empty((len(CROPS), CH, LENGTH), dtype=torch.float32),
                  torch.empty((len(CROPS), CH, 2 * LENGTH), dtype=torch.float32, device=dev)[:, :, ::2]):
        with pytest.raises(ValueError):
            bank.crops(files_, starts, LENGTH, out=wrong)
    with pytest.raises(ValueError):
        bank.crops(files_, starts, LENGTH, dtype=torch.float64)


def test_flacbank_runs_on_the_callers_stream(bank, file_ints):
    """Under torch.cuda.stream(s) the crops and a consumer queued on s right after them, with no
    synchronisation of the test's own in between: the consumer sees the delivered samples."""
    torch, dev = _torch()
    files_, starts = [0, 3, 2, 3], [0, 2000, 10, 9000]
    length = 8000  # several tiles a crop
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        x, n = bank.crops(files_, starts, length)
        y = x.float() * 2
    s.synchronize()
    assert n == [8000, 8000, 602, 8000]
    want = np.zeros((4, CH, length), dtype=np.float32)
    for w, (f, st) in enumerate(zip(files_, starts)):
        v = file_ints[f][st:st + length].astype(np.float32) * np.float32(2.0 ** -15)
        want[w, :, :len(v)] = v.T
    assert (y.cpu().numpy().view(np.uint32) == (want * np.float32(2)).view(np.uint32)).all()


def _break_first_frame(flac):
    """The file with the first subframe of its first frame given a reserved type and the frame's
    CRC-16 made right again: the index and the positions accept it, no decoder can decode it."""
    import flacgpu

    _, first, sizes = flacgpu.flac_index(flac)
    frame = bytearray(flac[first:first + sizes[0]])
    assert flac_bits.crc8(bytes(frame[:5])) == frame[5]  # sync, two code bytes, frame number 0, CRC-8: the header is 6 bytes
    frame[6] = 0x04  # subframe type 000010: reserved
    frame[-2:] = flac_bits.crc16(bytes(frame[:-2])).to_bytes(2, "big")
    return flac[:first] + bytes(frame) + flac[first + sizes[0]:]


def test_flacbank_strict_names_the_crop_of_a_damaged_file(files):
    import flacbank
    import flacgpu

    damaged = _break_first_frame(files[3][0])
    with flacbank.FlacBank([files[0][0], damaged, files[2][0]], device=0, max_frames=64) as b:
        assert b.samples == [_samples(0), _samples(3), _samples(2)]
        with pytest.raises(flacgpu.FlacGpuError, match=r"crop 1 \(file 1, start 200\) is BAD_FRAME, frame 0"):
            b.crops([0, 1, 2], [5, 200, 7], 100)
        x, n, statuses = b.crops([0, 1, 1, 2], [5, 200, 256, 7], 100, strict=False)
        assert statuses == [0, flacgpu.WINDOW_BAD_FRAME, 0, 0] and n == [100, 0, 100, 100]
        want = np.zeros((4, CH, 100), dtype=np.uint32)
        for w, (f, st) in enumerate([(0, 5), (None, 0), (3, 256), (2, 7)]):
            if f is not None:
                want[w] = elements(ints(files[f][1], CH, BITS)[st:st + 100], BITS, F32).T
        assert (_bits_of(x[[0, 2, 3]], F32) == want[[0, 2, 3]]).all()  # a crop that is not OK is left as allocated


def test_flacbank_splits_more_crops_than_one_call_takes(files, file_ints):
    import flacbank

    W = 65535 + 3
    with flacbank.FlacBank([files[1][0]], device=0, max_frames=4096) as b:
        starts = [(7 * w) % 255 for w in range(W)]
        x, n = b.crops([0] * W, starts, 2, dtype=_torch_dtypes()[I32])
    assert n == [2] * W
    src = file_ints[1]
    idx = np.array(starts)
    want = np.stack([src[idx], src[idx + 1]], axis=2)  # [W, C, 2]
    assert (x.cpu().numpy() == want).all()
