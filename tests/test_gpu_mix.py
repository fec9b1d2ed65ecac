"""Sample windows delivered with a channel mix on the GPU: flacgpu_decode_windows_device_mix
(k_window_elements<true>) and FlacMixBank.

Everything compares bit patterns for equality; there is no tolerance.  The expected elements are
the generators' own PCM (synth.synth_pcm, the PCM this file builds, frame_grammar.case_pcm) turned
into integers with numpy and mixed here: a mask of one channel is that channel's element
(test_gpu_deliver.elements), a mask of m = 2, 4, 8 channels is

    s.astype(np.int64).sum -> .astype(np.float32) * np.float32(2.0 ** -(bits - 1 + log2 m))

narrowed by numpy (f16) or torch on the CPU (bf16), a mask of none is 0; they are never an output
of the decoder.  Every output buffer is filled with 0xA5 before the call and compared whole, so a
stray write anywhere fails.  Blocks of 256 (the golden 3-channel file: 4096), files of at most 70
frames, contexts of 64 frames per call.

Mutation counts (each mutant of k_window_elements<true> / its host side fails tests here): DESIGN.md 7b."""
import json
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_grammar as fg  # noqa: E402
import oracle_ref  # noqa: E402
import synth  # noqa: E402
import test_gpu_deliver as tgd  # noqa: E402
from test_gpu_deliver import BF16, ESZ, F16, F32, FORMAT_NAMES, I32, PAD, PLANAR, elements, file_ints, ints, layout, need  # noqa: E402,F401
from window_helpers import BITS, BLOCK, CH, FRAMES, NONE, RATE, Resident, cover  # noqa: E402
from window_helpers import ctx, files, resident  # noqa: E402,F401  (fixtures: the five stereo 16-bit files)

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
DEC_RANGE = 7
ALL_FLAGS = [0, PLANAR, PAD, PLANAR | PAD]
FLAG_IDS = ["interleaved", "planar", "interleaved_pad", "planar_pad"]


# ---- the expectation -------------------------------------------------------------------------------
def mix_elements(x, bits, fmt, masks):
    """int32 [samples, C] -> the mixed elements' bit patterns [samples, K] by numpy and torch-CPU."""
    import torch

    out = np.zeros((len(x), len(masks)), dtype=np.uint32 if ESZ[fmt] == 4 else np.uint16)
    for k, mask in enumerate(masks):
        chans = [c for c in range(8) if mask >> c & 1]
        assert all(c < x.shape[1] for c in chans)
        m = len(chans)
        if m == 0:
            continue
        if m == 1:
            out[:, k] = elements(np.ascontiguousarray(x[:, chans[0]]), bits, fmt)
            continue
        assert fmt != I32 and m in (2, 4, 8)
        s = x[:, chans].astype(np.int64).sum(axis=1)
        f32 = s.astype(np.float32) * np.float32(2.0 ** -(bits - 1 + {2: 1, 4: 2, 8: 3}[m]))
        if fmt == F32:
            out[:, k] = f32.view(np.uint32)
        elif fmt == F16:
            out[:, k] = f32.astype(np.float16).view(np.uint16)
        else:
            out[:, k] = torch.from_numpy(np.ascontiguousarray(f32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return out


def mix_call(r, windows, fmt, flags, masks, offsets, caps, size):
    """One flacgpu_decode_windows_device_mix call on the Resident r into a 0xA5-filled buffer of
    `size` bytes -> (the buffer's bytes, [WindowResult]); offsets and caps in elements."""
    return r._call(windows, size, lambda out, res: r.d.decode_windows_device_mix(
        *r._tables(), windows, fmt, flags, masks, out, offsets, caps, res, stream=r.st))


def check_mix(out, res, windows, blocks_of, ints_of, bits, fmt, flags, masks, offsets, caps, expect_status=None):
    """test_gpu_deliver.check_delivery with K = len(masks) output channels."""
    expect_status = expect_status or {}
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    K = len(masks)
    for w, ((s, start, count), r) in enumerate(zip(windows, res)):
        first, frames, take = cover(blocks_of[s], start, count)
        if w in expect_status:
            st, bad, bad_st = expect_status[w]
            assert (r.status, r.n_samples, r.first_bad_frame, r.first_bad_status) == (st, 0, bad, bad_st), w
            continue
        assert (r.status, r.n_samples, r.n_frames, r.first_bad_frame, r.first_bad_status) == (0, take, frames, NONE, 0), w
        if frames:
            assert r.first_frame == first, w
        assert need(take, count, flags) * K <= caps[w]
        el = mix_elements(ints_of[s][start:start + take], bits, fmt, masks)  # [take, K]
        o = offsets[w]
        if flags & PLANAR:
            for k in range(K):
                want[o + k * count:o + k * count + take] = el[:, k]
                if flags & PAD:
                    want[o + k * count + take:o + (k + 1) * count] = 0
        else:
            want[o:o + take * K] = el.reshape(-1)
            if flags & PAD:
                want[o + take * K:o + count * K] = 0
    got = np.frombuffer(out, dtype=dt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]  # elements, and 0xA5 everywhere else


def run_mix(r, windows, blocks_of, ints_of, bits, fmt, flags, masks, expect_status=None, short=None):
    """The windows with exactly the capacity each needs (short: {window: elements less}), at every
    destination alignment in turn, checked whole -> the results."""
    K = len(masks)
    sizes = [K * need(cover(blocks_of[s], start, count)[2], count, flags) - (short or {}).get(w, 0)
             for w, (s, start, count) in enumerate(windows)]
    offs, size = layout(sizes, fmt)
    out, res = mix_call(r, windows, fmt, flags, masks, offs, sizes, size)
    check_mix(out, res, windows, blocks_of, ints_of, bits, fmt, flags, masks, offs, sizes, expect_status=expect_status)
    return res


def stereo_windows():
    """tgd.forty_windows without the two of 2^64 - 1 samples: inside one frame, across frame
    boundaries, a whole file, across the short last frame, clipped, at and past the end, of count 0,
    overlapping, of the file without frames, and the seeded ones."""
    w = [x for x in tgd.forty_windows() if x[2] != U64]
    assert len(w) == 38 and (2, 5, 0) in w and (2, tgd._samples(2) + 88, 10) in w and (2, 500, 1000) in w
    return w


def stereo_blocks():
    return {i: tgd._blocks(i) for i in range(len(FRAMES))}


# ---- identity: the bytes of _as ------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("fmt", [I32, F32, F16, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_identity_is_the_as_call(resident, fmt, flags):
    windows = tgd.forty_windows()
    blocks_of = stereo_blocks()
    takes = [cover(blocks_of[s], start, count) for s, start, count in windows]
    assert sum(t[1] for t in takes) > 128  # the covering frames cross two chunk boundaries
    sizes = [CH * (t[2] if windows[w][2] == U64 else need(t[2], windows[w][2], flags)) for w, t in enumerate(takes)]
    offs, size = layout(sizes, fmt)
    assert {(o * ESZ[fmt]) % 16 for o in offs} == set(range(0, 16, ESZ[fmt]))  # every destination alignment
    ref_out, ref_res = resident.deliver(windows, fmt, flags, offs, sizes, size)
    out, res = mix_call(resident, windows, fmt, flags, [1, 2], offs, sizes, size)
    assert [tgd._fields(a) for a in res] == [tgd._fields(b) for b in ref_res]
    assert sum(r.status == 0 and r.n_samples > 0 for r in res) >= 30
    assert out == ref_out and out != b"\xA5" * len(out)


# ---- stereo 16-bit to mono ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("fmt", [F32, F16, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_stereo_to_mono(resident, file_ints, fmt, flags):
    windows = stereo_windows()
    res = run_mix(resident, windows, stereo_blocks(), file_ints, BITS, fmt, flags, [3])
    assert [r.n_samples for r in res[4:8]] == [112, 0, 0, 0] and res[11].n_frames == 0
    if fmt == F32 and flags == 0:  # the mean is not one of its channels: the two differ somewhere in every file
        for i in (0, 1, 2, 3):
            x = file_ints[i]
            assert (x[:, 0] != x[:, 1]).any()


def test_other_shapes_of_stereo(resident, file_ints):
    """Stereo to three channels with a silent one, and the swap, I32 included."""
    windows = stereo_windows()
    for fmt, flags, masks in ((F32, PLANAR | PAD, [1, 2, 0]), (F16, 0, [1, 2, 0]), (BF16, PAD, [0, 3, 2]),
                              (I32, PLANAR | PAD, [2, 1]), (I32, 0, [2, 1]), (F32, PLANAR, [2, 1]), (I32, PAD, [2, 0, 2])):
        run_mix(resident, windows, stereo_blocks(), file_ints, BITS, fmt, flags, masks)


# ---- sources made here: PCM chosen by the test, encoded by the CPU oracle encoder ---------------------------
def _pcm_with(n, channels, bits, stream, rows=()):
    """synth's samples with `rows` (tuples of one sample each channel) laid over samples 300 on:
    across the boundary of frames 1 and 2."""
    x = synth.synth_samples(n, channels, bits, RATE, stream=stream)
    for i, row in enumerate(rows):
        x[300 + i] = row
    return synth.to_pcm_bytes(x, bits)


def _directed_rows(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rows = [(lo, lo), (hi, hi), (lo, hi), (hi, lo), (hi, hi - 1), (lo + 1, lo), (0, 0), (1, 0), (-1, 0), (1, 1)]
    if bits == 32:
        # sums on and next to the ties of the int64 -> f32 rounding: 2^k + half an ulp, and that with an odd significand
        for k in range(24, 32):
            half = 1 << (k - 24)
            for s in ((1 << k) + half, (1 << k) + 3 * half, (1 << k) + half + 1, (1 << k) + half - 1, 1 << k):
                for sign in (1, -1):
                    a = sign * s // 2
                    rows.append((a, sign * s - a))
        rows.append((lo, lo))  # -2^32
    return [r for r in rows if all(lo <= v <= hi for v in r)]


MADE = {  # name -> (channels, bits, samples, synth stream, directed rows)
    "mono16": (1, 16, 5 * BLOCK + 100, 40, ()),
    "mono24": (1, 24, 3 * BLOCK + 77, 41, ()),
    "stereo24": (2, 24, 6 * BLOCK + 31, 42, _directed_rows(24)),
    "stereo32": (2, 32, 4 * BLOCK + 200, 43, _directed_rows(32)),
    "eight16": (8, 16, 5 * BLOCK + 9, 44, ([-32768] * 8, [32767] * 8)),
    # the limits, and sums past 2^24 that the f32 conversion rounds: 2^25 - 1, the tie -2^25 - 1, 6 * 2^23 - 1
    "eight24": (8, 24, 3 * BLOCK + 130, 45, ([-(1 << 23)] * 8, [(1 << 23) - 1] * 8, [(1 << 23) - 1] * 4 + [3, 0, 0, 0],
                                            [-(1 << 23)] * 4 + [0, -1, 0, 0], [(1 << 23) - 1] * 6 + [5, 0])),
}


@pytest.fixture(scope="module")
def made():
    """{name: (flac file, int32 [samples, channels], blocks)}: made once, shared, never changed."""
    out = {}
    for name, (ch, bits, n, stream, rows) in MADE.items():
        pcm = _pcm_with(n, ch, bits, stream, rows)
        flac = oracle_ref.encode_file(pcm, ch, bits, RATE, block=BLOCK)
        x = ints(pcm, ch, bits)
        x.setflags(write=False)
        blocks = [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else [])
        out[name] = (flac, x, blocks)
    return out


def _made_windows(n):
    return [(0, 0, n), (0, 290, 150), (0, 255, 2), (0, 300, 97), (0, n - 50, 200), (0, n + 5, 30), (0, 7, 0), (0, 511, 258)]


def _run_made(made, name, cases):
    import flacgpu

    ch, bits, n = MADE[name][:3]
    flac, x, blocks = made[name]
    assert flacgpu.flac_index(flac)[0].interchannel_samples == n == sum(blocks)
    with flacgpu.Decoder(ch, bits, RATE, device=0, max_frames=64, block_size=BLOCK) as d:
        r = Resident(d, [(tgd._bare(flac), bits, RATE)])
        assert r.index == [(0, len(blocks))] and r.totals == [n]
        for fmt, flags, masks in cases:
            res = run_mix(r, _made_windows(n), {0: blocks}, {0: x}, bits, fmt, flags, masks)
            assert [v.n_samples for v in res[4:7]] == [50, 0, 0]
    return x


def test_mono_to_two_channels(made):
    _run_made(made, "mono16", [(F32, PLANAR | PAD, [1, 1]), (BF16, 0, [1, 1]), (I32, PAD, [1, 1]), (F16, PLANAR, [1, 0, 1])])


def test_24_bit_stereo_to_mono(made):
    x = _run_made(made, "stereo24", [(F32, PLANAR | PAD, [3]), (F32, 0, [3]), (F16, PAD, [3]), (BF16, PLANAR, [3])])
    s = x.astype(np.int64).sum(axis=1)
    # two 24-bit samples reach -2^24 (both at the minimum) and at most 2^24 - 2
    assert s.min() == -(1 << 24) and s.max() == (1 << 24) - 2 and {-(1 << 24), (1 << 24) - 2} <= set(s[290:440].tolist())


def test_32_bit_stereo_to_mono(made):
    x = _run_made(made, "stereo32", [(F32, PLANAR | PAD, [3]), (F32, 0, [3]), (F16, PLANAR, [3]), (BF16, PAD, [3]),
                                     (I32, 0, [2, 1])])
    s = x.astype(np.int64).sum(axis=1)
    inexact = s.astype(np.float32).astype(np.float64) != s.astype(np.float64)
    assert inexact.sum() > 100 and s.min() == -(1 << 32)
    have = set(s[300:440].tolist())
    for k in range(24, 32):  # exact ties, above an even and an odd significand
        half = 1 << (k - 24)
        assert {(1 << k) + half, (1 << k) + 3 * half, -(1 << k) - half} <= have, k
    assert (np.abs(s) > (1 << 31)).any()  # sums no int32 holds


def test_eight_channels_16_bit(made):
    x = _run_made(made, "eight16", [(F32, PLANAR | PAD, [0xFF]), (BF16, 0, [0xFF]), (F32, 0, [0x0F, 0xF0]),
                                    (F16, PLANAR | PAD, [0x0F, 0xF0]), (F32, PLANAR, [0xFF, 0x81, 0x10, 0])])
    s = x.astype(np.int64).sum(axis=1)
    assert s.min() == -8 * 32768 and s.max() == 8 * 32767


def test_eight_channels_24_bit_to_mono(made):
    """per = 24: 170 samples a tile, so the whole-stream window takes six."""
    x = _run_made(made, "eight24", [(F32, PLANAR | PAD, [0xFF]), (F32, 0, [0xFF]), (BF16, PAD, [0xFF]), (F16, PLANAR, [0xFF, 0xF0])])
    s = x.astype(np.int64).sum(axis=1)
    assert s.min() == -(1 << 26) and s.max() == 8 * ((1 << 23) - 1)
    assert {(1 << 25) - 1, -(1 << 25) - 1, 6 * (1 << 23) - 1} <= set(s[300:305].tolist())
    assert (s.astype(np.float32).astype(np.float64) != s.astype(np.float64)).sum() >= 3  # sums whose conversion rounds


def test_golden_three_channels_8_bit():
    import hashlib

    import flacgpu

    with open(os.path.join(HERE, "golden", "manifest.json")) as f:
        case = next(c for c in json.load(f)["cases"] if c["name"] == "3ch_8bit")
    n = case["n_samples"]
    pcm = synth.synth_pcm(n, 3, 8, case["rate"], stream=case["stream_seed"])
    assert hashlib.sha256(pcm).hexdigest() == case["pcm_sha256"] and (case["channels"], case["bits"]) == (3, 8)
    with open(os.path.join(HERE, "golden", "3ch_8bit.flac"), "rb") as f:
        frames = f.read()
    x, blocks = ints(pcm, 3, 8), [4096, n - 4096]
    with flacgpu.Decoder(3, 8, case["rate"], device=0, max_frames=64, block_size=4096) as d:
        r = Resident(d, [(frames, 8, case["rate"])])
        assert r.index == [(0, 2)] and r.totals == [n]
        windows = [(0, 0, n), (0, 4090, 20), (0, 4100, 100), (0, 17, 1365), (0, 1365, 1366)]  # a tile is 1365 samples
        for fmt, flags in ((F32, PLANAR | PAD), (F16, 0), (BF16, PLANAR), (F32, PAD)):
            res = run_mix(r, windows, {0: blocks}, {0: x}, 8, fmt, flags, [0b011, 0b100])
            assert res[2].n_samples == 20


# ---- statuses ------------------------------------------------------------------------------------------
def test_too_small_is_by_the_output_channels(resident, file_ints):
    """Stereo to mono: count elements hold a window (2 * count would be the source's); one less is
    TOO_SMALL and writes nothing, between two good neighbours.  Stereo to three: 2 * count is too small."""
    windows = [(0, 100, 300), (3, 4000, 600), (1, 3, 200)]
    for flags in (PAD, PAD | PLANAR, 0):
        res = run_mix(resident, windows, stereo_blocks(), file_ints, BITS, F32, flags, [3], short={1: 1},
                      expect_status={1: (3, NONE, 0)})
        assert [r.status for r in res] == [0, 3, 0]
        res = run_mix(resident, windows, stereo_blocks(), file_ints, BITS, F32, flags, [3])
        assert [r.status for r in res] == [0, 0, 0]
    res = run_mix(resident, windows, stereo_blocks(), file_ints, BITS, BF16, PLANAR, [1, 2, 0], short={1: 600},
                  expect_status={1: (3, NONE, 0)})
    assert [r.status for r in res] == [0, 3, 0]


def test_bad_frame_writes_nothing_and_harms_no_neighbour():
    """tgd.test_bad_frame_writes_nothing_with_pad with a mix: the third frame of the 24-bit mono
    grammar stream is above the context's block size."""
    import flacgpu

    c = tgd._case("waste_and_unary")
    blocks = [f["block"] for f in c["frames"]]
    assert blocks == [128, 192, 1152, 256, 100] and (c["channels"], c["bits"]) == (1, 24)
    x = ints(fg.case_pcm(c), 1, 24)
    windows = [(0, 100, 220), (0, 300, 100), (0, 1482, 300), (0, 320, 1), (0, 1472, 356), (0, 1471, 1), (0, 100, 220)]
    bad = {1: (2, 2, DEC_RANGE), 3: (2, 2, DEC_RANGE), 5: (2, 2, DEC_RANGE)}
    with flacgpu.Decoder(1, 24, c["rate"], device=0, max_frames=64, block_size=256) as d:
        r = Resident(d, [(fg.case_bytes(c), 24, c["rate"])])
        for flags in (PAD, PAD | PLANAR):
            res = run_mix(r, windows, {0: blocks}, {0: x}, 24, F32, flags, [1, 1], expect_status=bad)
            assert [v.status for v in res] == [0, 2, 0, 2, 0, 2, 0]


def test_invalid_mixes_are_refused_by_a_context(ctx, resident):
    """On a stereo context: the call returns INVALID_INPUT and the buffer keeps its 0xA5."""
    import flacgpu

    windows = [(0, 0, 10)]
    for fmt, masks in ((F32, [4]), (F32, [1, 2, 8]), (F32, [0xFF]), (I32, [3]), (I32, [1, 3]), (F32, []), (F32, [1] * 9)):
        with pytest.raises(flacgpu.FlacGpuError) as e:
            mix_call(resident, windows, fmt, PAD, masks, [0], [100], 1024)
        assert e.value.code == -2, masks
    out, res = mix_call(resident, windows, F32, PAD, [3, 3, 3, 3, 3, 3, 3, 3], [0], [80], 1024)  # eight output channels
    assert res[0].status == 0 and out[:320] != b"\xA5" * 320 and out[320:] == b"\xA5" * (1024 - 320)


# ---- FlacMixBank ---------------------------------------------------------------------------------------------
LENGTH = 300


def _bank_sources(files, file_ints, made, names):
    """[(flac, ints, bits)] of the named sources: 'sN' is stereo 16-bit file N of the fixture."""
    out = []
    for name in names:
        if name[0] == "s" and name[1:].isdigit():
            out.append((files[int(name[1:])][0], file_ints[int(name[1:])], 16))
        else:
            out.append((made[name][0], made[name][1], MADE[name][1]))
    return out


def _default_masks(C, K):
    return [1 << k for k in range(K)] if C == K else ([1] * K if C == 1 else [(1 << C) - 1])


def _expected_crops(src, crops, K, fmt, planar, masks_of=None):
    want = np.zeros((len(crops), LENGTH, K), dtype=np.uint32 if ESZ[fmt] == 4 else np.uint16)
    n = []
    for w, (f, start) in enumerate(crops):
        _, x, bits = src[f]
        C = x.shape[1]
        el = mix_elements(x[start:start + LENGTH], bits, fmt, (masks_of or {}).get(C) or _default_masks(C, K))
        want[w, :len(el)] = el
        n.append(len(el))
    return (want.transpose(0, 2, 1) if planar else want), n


def _shuffled_crops(src, seed):
    """Per file: a crop inside, one across frames, one clipped by the end and one past it; shuffled."""
    crops = []
    for f, (_, x, _) in enumerate(src):
        n = len(x)
        crops += [(f, 10), (f, 200), (f, max(n - 120, 0)), (f, n + 3)]
    random.Random(seed).shuffle(crops)
    return crops


@pytest.fixture(scope="module")
def mono_bank(files, file_ints, made):
    import flacbank

    src = _bank_sources(files, file_ints, made, ["mono16", "s2", "stereo24", "eight16", "s1", "s3"])
    with flacbank.FlacMixBank([s[0] for s in src], channels=1, device=0, max_frames=64) as b:
        yield b, src


def test_mixbank_properties(mono_bank):
    b, src = mono_bank
    assert len(b) == 6 and b.channels == 1 and b.bits == [16, 24]
    assert b.file_channels == [1, 2, 2, 8, 2, 2] and b.file_bits == [16, 16, 24, 16, 16, 16]
    assert b.samples == [len(s[1]) for s in src] and b.sample_rates == [RATE] * 6
    assert len(b._groups) == 4  # (1, 16), (2, 16), (2, 24), (8, 16)


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [F32, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_mixbank_to_mono(mono_bank, fmt, planar):
    b, src = mono_bank
    crops = _shuffled_crops(src, "mono")
    x, n = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar)
    want, want_n = _expected_crops(src, crops, 1, fmt, planar)
    assert n == want_n and 120 in n and 0 in n and LENGTH in n
    assert tuple(x.shape) == ((len(crops), 1, LENGTH) if planar else (len(crops), LENGTH, 1)) and x.is_contiguous()
    assert (tgd._bits_of(x, fmt) == want).all()
    # the memset form gives the same tensor
    y, n2 = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar, pad=False)
    assert n2 == want_n and (tgd._bits_of(y, fmt) == want).all()


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [F32, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_mixbank_to_stereo(files, file_ints, made, fmt, planar):
    import flacbank

    src = _bank_sources(files, file_ints, made, ["stereo24", "mono16", "s2", "mono24", "s1"])
    crops = _shuffled_crops(src, "stereo")
    with flacbank.FlacMixBank([s[0] for s in src], channels=2, device=0, max_frames=64) as b:
        assert len(b._groups) == 4 and b.file_channels == [2, 1, 2, 1, 2] and b.file_bits == [24, 16, 16, 24, 16]
        x, n = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar)
    want, want_n = _expected_crops(src, crops, 2, fmt, planar)
    assert n == want_n and (tgd._bits_of(x, fmt) == want).all()


def test_mixbank_channel_map(files, file_ints, made):
    """A map: eight channels to front and back halves, stereo swapped."""
    import flacbank

    src = _bank_sources(files, file_ints, made, ["eight16", "s2", "eight24"])
    crops = _shuffled_crops(src, "map")
    masks_of = {8: [0x0F, 0xF0], 2: [2, 1]}
    with flacbank.FlacMixBank([s[0] for s in src], channels=2, device=0, max_frames=64, channel_map=masks_of) as b:
        x, n = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH)
    want, want_n = _expected_crops(src, crops, 2, F32, True, masks_of=masks_of)
    assert n == want_n and (tgd._bits_of(x, F32) == want).all()


def test_mixbank_out_is_reused(mono_bank):
    torch, dev = tgd._torch()
    b, src = mono_bank
    crops = _shuffled_crops(src, "out")
    f, s = [c[0] for c in crops], [c[1] for c in crops]
    want = _expected_crops(src, crops, 1, F32, True)[0]
    buf = torch.full((len(crops), 1, LENGTH), 7.0, dtype=torch.float32, device=dev)
    x, n, statuses = b.crops(f, s, LENGTH, out=buf, strict=False)
    assert x is buf and statuses == [0] * len(crops) and (tgd._bits_of(buf, F32) == want).all()
    buf.fill_(7.0)
    x, _ = b.crops(f, s, LENGTH, out=buf, pad=False)
    assert x is buf and (tgd._bits_of(buf, F32) == want).all()
    for wrong in (torch.empty((len(crops), LENGTH, 1), dtype=torch.float32, device=dev),
                  torch.empty((len(crops), 1, LENGTH), dtype=torch.float16, device=dev),
                  torch.empty((len(crops), 1, LENGTH), dtype=torch.float32),
                  torch.empty((len(crops), 2, LENGTH), dtype=torch.float32, device=dev)):
        with pytest.raises(ValueError):
            b.crops(f, s, LENGTH, out=wrong)
    with pytest.raises(ValueError):
        b.crops(f, s, LENGTH, dtype=torch.float64)
    with pytest.raises(ValueError):
        b.crops([6], [0], LENGTH)


def test_mixbank_a_damaged_file_harms_only_its_own_crops(files, file_ints, made):
    import flacbank
    import flacgpu

    src = _bank_sources(files, file_ints, made, ["mono16", "s3", "stereo24", "s2"])
    damaged = tgd._break_first_frame(src[1][0])
    crops = [(0, 10), (1, 100), (2, 5), (1, 256), (3, 0), (1, 200), (0, 300)]  # file 1: frame 0, frame 1 on, frames 0 and 1
    with flacbank.FlacMixBank([src[0][0], damaged, src[2][0], src[3][0]], channels=1, device=0, max_frames=64) as b:
        assert b.samples == [len(s[1]) for s in src]
        with pytest.raises(flacgpu.FlacGpuError, match=r"crop 1 \(file 1, start 100\) is BAD_FRAME, frame 0"):
            b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH)
        x, n, statuses = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH, strict=False)
    B = flacgpu.WINDOW_BAD_FRAME
    assert statuses == [0, B, 0, 0, 0, B, 0] and n == [LENGTH, 0, LENGTH, LENGTH, LENGTH, 0, LENGTH]
    want, _ = _expected_crops(src, crops, 1, F32, True)
    ok = [0, 2, 3, 4, 6]
    assert (tgd._bits_of(x[ok], F32) == want[ok]).all()  # a crop that is not OK is left as allocated


def test_mixbank_int32(mono_bank, files, file_ints, made):
    import flacbank

    torch, _ = tgd._torch()
    b, _ = mono_bank
    with pytest.raises(ValueError, match="different scales"):  # 16 and 24 bits in one bank
        b.crops([0], [0], LENGTH, dtype=torch.int32)
    src = _bank_sources(files, file_ints, made, ["s2", "mono16", "s1"])
    crops = _shuffled_crops(src, "int")
    with flacbank.FlacMixBank([s[0] for s in src], channels=2, device=0, max_frames=64) as one_depth:
        x, n = one_depth.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH, dtype=torch.int32, planar=False)
    want, want_n = _expected_crops(src, crops, 2, I32, False)
    assert n == want_n and x.dtype == torch.int32 and (tgd._bits_of(x, I32) == want).all()
    with flacbank.FlacMixBank([src[0][0], src[1][0]], channels=1, device=0, max_frames=64) as means:  # stereo to mono is a mean
        with pytest.raises(ValueError, match="int32 cannot deliver"):
            means.crops([0], [0], LENGTH, dtype=torch.int32)
