"""Sample windows delivered at another sample rate on the GPU:
flacgpu_decode_windows_device_resample (k_window_resample), FlacBank.crops(rate=) and
FlacMixBank(sample_rate=).

The expected elements never come from the decoder: the generator's PCM is turned into F32 elements
and mixes by numpy (test_gpu_mix.mix_elements), each output channel then goes through the host
statement of the rule, flacgpu.resample_f32_host (itself checked against float64 under a derived
bound by tests/test_resample_host.py), and is narrowed by numpy (f16) or torch on the CPU (bf16).
Every output buffer is filled with 0xA5 before the call and compared whole, bit for bit.  One test
compares the device's F32 outputs with tests/resample_ref.py's float64 values directly, so the
device does not depend on the host rule alone.

Sources: a handful of files of 2 to 12 frames, blocks of 192, 4096 and 16384, so that a filter's
reach crosses several frames; 16-bit stereo and mono at 44100, 48000 and 16000, one 24-bit, one
8-bit, one 32-bit and one big-block file, encoded by the CPU oracle encoder."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import flac_bits  # noqa: E402
import oracle_ref  # noqa: E402
import resample_ref as ref  # noqa: E402
import synth  # noqa: E402
import test_gpu_deliver as tgd  # noqa: E402
from test_gpu_deliver import BF16, ESZ, F16, F32, FORMAT_NAMES, I32, PAD, PLANAR, ints, layout, need  # noqa: E402
from test_gpu_mix import mix_elements  # noqa: E402
from window_helpers import NONE, Resident, cover  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_FLAGS = [0, PLANAR, PAD, PLANAR | PAD]
FLAG_IDS = ["interleaved", "planar", "interleaved_pad", "planar_pad"]
SIX = [(44100, 48000), (48000, 44100), (48000, 16000), (16000, 32000), (44100, 16000), (96000, 8000)]  # 160/147 .. 1/12
SIX_IDS = ["160_147", "147_160", "1_3", "2_1", "160_441", "1_12"]

# name -> (group, channels, bits, rate, block, samples, synth stream); a group is one decode context
SOURCES = {
    "s44": ("st16", 2, 16, 44100, 192, 11 * 192 + 100, 70),
    "s48": ("st16", 2, 16, 48000, 4096, 2 * 4096 + 900, 71),
    "s16": ("st16", 2, 16, 16000, 192, 8 * 192 + 50, 72),
    "m44": ("mo16", 1, 16, 44100, 4096, 2 * 4096 + 333, 73),
    "m16": ("mo16", 1, 16, 16000, 192, 5 * 192 + 7, 74),
    "m96": ("mo16", 1, 16, 96000, 16384, 16384 + 700, 75),  # the big-block file
    "t48": ("st24", 2, 24, 48000, 192, 6 * 192 + 31, 76),
    "e44": ("mo8", 1, 8, 44100, 192, 7 * 192 + 5, 77),
    "w44": ("st32", 2, 32, 44100, 192, 4 * 192 + 120, 78),
}
GROUPS = {"st16": (2, 16, 4096), "mo16": (1, 16, 16384), "st24": (2, 24, 192), "mo8": (1, 8, 192), "st32": (2, 32, 192)}


def _members(group):
    return [n for n, s in SOURCES.items() if s[0] == group]


@pytest.fixture(scope="module")
def sources():
    """{name: (flac file, int32 [samples, channels], blocks)}: made once, shared, never changed."""
    out = {}
    for name, (_, ch, bits, rate, block, n, stream) in SOURCES.items():
        pcm = synth.synth_pcm(n, ch, bits, rate, stream=stream)
        flac = oracle_ref.encode_file(pcm, ch, bits, rate, block=block)
        x = ints(pcm, ch, bits)
        x.setflags(write=False)
        out[name] = (flac, x, [block] * (n // block) + ([n % block] if n % block else []))
    return out


@pytest.fixture(scope="module")
def residents(sources):
    """{group: Resident of the group's files, in SOURCES order} on a decode context each."""
    import flacgpu

    with contextlib.ExitStack() as stack:
        out = {}
        for g, (ch, bits, block) in GROUPS.items():
            d = stack.enter_context(flacgpu.Decoder(ch, bits, 44100, device=0, max_frames=8, block_size=block))
            names = _members(g)
            r = Resident(d, [(tgd._bare(sources[n][0]), bits, SOURCES[n][3]) for n in names])
            assert r.index == [(0, len(sources[n][2])) for n in names] and r.totals == [SOURCES[n][5] for n in names]
            out[g] = r
        yield out


# ---- the expectation -------------------------------------------------------------------------------
_WHOLE = {}


def whole_f32(sources, name, masks, src, dst):
    """The whole stream resampled: float32 [out_total, K], by the host rule channel by channel."""
    import flacgpu

    key = (name, tuple(masks), src, dst)
    if key not in _WHOLE:
        x, bits = sources[name][1], SOURCES[name][2]
        planes = mix_elements(x, bits, F32, masks).view(np.float32)  # [samples, K]
        y = np.stack([flacgpu.resample_f32_host(np.ascontiguousarray(planes[:, k]), src, dst) for k in range(len(masks))], axis=1)
        y.setflags(write=False)
        _WHOLE[key] = y
    return _WHOLE[key]


def narrow(y, fmt):
    import torch

    if fmt == F32:
        return y.view(np.uint32)
    if fmt == F16:
        return y.astype(np.float16).view(np.uint16)
    y = np.array(y, dtype=np.float32)  # a copy: the cached streams are read-only
    return torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def identity(group):
    return [1 << c for c in range(GROUPS[group][0])]


def resample_call(r, windows, fmt, flags, masks, src, dst, offsets, caps, size):
    return r._call(windows, size, lambda out, res: r.d.decode_windows_device_resample(
        *r._tables(), windows, fmt, flags, masks, src, dst, out, offsets, caps, res, stream=r.st))


def run(residents, sources, group, windows, fmt, flags, masks, src, dst, expect_status=None, short=None, given_masks=True):
    """One call: the windows [(file of the group, start, count)] in output samples, each with exactly
    the capacity it needs (short: {window: elements less}), at every destination alignment in turn;
    every result and the whole buffer checked -> the results."""
    r, names = residents[group], _members(group)
    eff = masks if masks is not None else identity(group)
    K = len(eff)
    L, M, Hw, T = ref.ratio(src, dst)
    takes = [ref.delivered(SOURCES[names[s]][5], L, M, start, count) for s, start, count in windows]
    sizes = [K * need(takes[w], windows[w][2], flags) - (short or {}).get(w, 0) for w in range(len(windows))]
    offs, size = layout(sizes, fmt)
    out, res = resample_call(r, windows, fmt, flags, masks if given_masks else None, src, dst, offs, sizes, size)
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    for w, ((s, start, count), v) in enumerate(zip(windows, res)):
        name, take = names[s], takes[w]
        lo, hi = ref.source_range(SOURCES[name][5], L, M, Hw, start, take)
        first, frames, span = cover(sources[name][2], lo, hi - lo)
        assert span == hi - lo
        if expect_status and w in expect_status:
            st, bad, bad_st = expect_status[w]
            assert (v.status, v.n_samples, v.first_bad_frame, v.first_bad_status) == (st, 0, bad, bad_st), w
            continue
        assert (v.status, v.n_samples, v.n_frames, v.first_bad_frame, v.first_bad_status) == (0, take, frames, NONE, 0), w
        if frames:
            assert v.first_frame == first, w
        el = narrow(np.ascontiguousarray(whole_f32(sources, name, eff, src, dst)[start:start + take]), fmt)  # [take, K]
        o = offs[w]
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
    return res


def usual_windows(s, out_n):
    """Of stream s with out_n output samples: from 0, the whole stream, across the end (clipped),
    interior ones across frames and tiles, count 0, past the end, two that overlap."""
    return [(s, 0, 37), (s, 0, out_n), (s, out_n - 41, 100), (s, out_n // 3, out_n // 2), (s, 7, 0), (s, out_n + 5, 30),
            (s, out_n, 1), (s, 100, 300), (s, 250, 301), (s, out_n - 1, 1)]


# ---- the six ratios --------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SIX, ids=SIX_IDS)
def test_six_ratios(residents, sources, src, dst):
    group, name = {44100: ("st16", "s44"), 48000: ("st16", "s48"), 16000: ("mo16", "m16"), 96000: ("mo16", "m96")}[src]
    assert SOURCES[name][3] == src
    s = _members(group).index(name)
    L, M, Hw, T = ref.ratio(src, dst)
    out_n = ref.out_total(SOURCES[name][5], L, M)
    windows = usual_windows(s, out_n)
    for flags in (PLANAR | PAD, 0):
        res = run(residents, sources, group, windows, F32, flags, identity(group), src, dst)
        assert [v.n_samples for v in res[:3]] == [37, out_n, 41] and [v.n_samples for v in res[4:7]] == [0, 0, 0]
        assert res[1].n_frames == len(sources[name][2]) and res[9].n_samples == 1
    if (src, dst) == (44100, 48000):
        assert out_n > 2 * 1024 and res[3].n_frames > 3  # more than two tiles, a reach across several frames
    if (src, dst) == (96000, 8000):
        assert T == 576 and res[7].n_frames == 1 and res[1].n_frames == 2


# ---- formats, layouts, odd offsets -------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("fmt", [F32, F16, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_formats_and_layouts(residents, sources, fmt, flags):
    L, M, _, _ = ref.ratio(44100, 48000)
    out_n = ref.out_total(SOURCES["s44"][5], L, M)
    windows = usual_windows(0, out_n) + [(2, 11, 95), (0, 1000, 1030)]  # another stream of the context between them
    n_align = 16 // ESZ[fmt]
    assert len(windows) >= n_align  # layout() gives window w the alignment w mod (16 / element size): heads and tails of every length
    run(residents, sources, "st16", windows, fmt, flags, identity("st16"), 44100, 48000)


# ---- mixes --------------------------------------------------------------------------------------------
def test_null_masks_are_the_identity(residents, sources):
    windows = [(0, 5, 700), (1, 9000, 2000), (0, 0, 50)]
    run(residents, sources, "st16", windows, F32, PLANAR | PAD, None, 44100, 48000, given_masks=False)
    run(residents, sources, "st16", windows, BF16, 0, [1, 2], 44100, 48000)


def test_stereo_to_mono_mean(residents, sources):
    L, M, _, _ = ref.ratio(48000, 44100)
    out_n = ref.out_total(SOURCES["s48"][5], L, M)
    for fmt, flags in ((F32, PLANAR | PAD), (F16, 0), (BF16, PAD)):
        run(residents, sources, "st16", usual_windows(1, out_n), fmt, flags, [3], 48000, 44100)
    x = sources["s48"][1]
    assert (x[:, 0] != x[:, 1]).any()


def test_mono_to_two_channels_and_other_shapes(residents, sources):
    L, M, _, _ = ref.ratio(16000, 32000)
    out_n = ref.out_total(SOURCES["m16"][5], L, M)
    for fmt, flags, masks in ((F32, PLANAR | PAD, [1, 1]), (BF16, 0, [1, 1]), (F16, PLANAR, [1, 0, 1])):
        run(residents, sources, "mo16", usual_windows(1, out_n), fmt, flags, masks, 16000, 32000)
    run(residents, sources, "st16", [(2, 0, 400), (2, 3000, 500)], F32, 0, [2, 1, 0, 3], 16000, 32000)  # swap, silence, mean


# ---- depths and the big block ------------------------------------------------------------------------
@pytest.mark.parametrize("name,src,dst,masks", [("t48", 48000, 44100, [3]), ("t48", 48000, 16000, [1, 2]), ("e44", 44100, 48000, [1]),
                                                ("w44", 44100, 48000, [3]), ("w44", 44100, 16000, [2, 1]),
                                                ("m96", 96000, 48000, [1]), ("m96", 96000, 44100, [1, 1])],
                         ids=["24bit_mean", "24bit_down", "8bit", "32bit_mean", "32bit_down", "bigblock_1_2", "bigblock_147_320"])
def test_depths_and_big_blocks(residents, sources, name, src, dst, masks):
    group = SOURCES[name][0]
    s = _members(group).index(name)
    L, M, _, _ = ref.ratio(src, dst)
    out_n = ref.out_total(SOURCES[name][5], L, M)
    for fmt, flags in ((F32, PLANAR | PAD), (F16, 0)):
        run(residents, sources, group, usual_windows(s, out_n), fmt, flags, masks, src, dst)


# ---- statuses ------------------------------------------------------------------------------------------
def test_too_small_is_by_the_output_count(residents, sources):
    windows = [(0, 100, 300), (1, 4000, 600), (0, 2300, 400)]  # the last is clipped
    for flags in (PAD, PAD | PLANAR, 0):
        res = run(residents, sources, "st16", windows, F32, flags, [3], 44100, 48000, short={1: 1}, expect_status={1: (3, NONE, 0)})
        assert [v.status for v in res] == [0, 3, 0]
        res = run(residents, sources, "st16", windows, F32, flags, [3], 44100, 48000)
        assert [v.status for v in res] == [0, 0, 0]
    res = run(residents, sources, "st16", windows, BF16, PLANAR, [1, 2, 0], 44100, 48000, short={2: 1}, expect_status={2: (3, NONE, 0)})
    assert [v.status for v in res] == [0, 0, 3]


def _break_frame(flac, k):
    """tgd._break_first_frame for frame k < 128 of a file of fixed 192-sample blocks (6-byte headers)."""
    import flacgpu

    _, first, sizes = flacgpu.flac_index(flac)
    at = first + sum(sizes[:k])
    frame = bytearray(flac[at:at + sizes[k]])
    assert flac_bits.crc8(bytes(frame[:5])) == frame[5] and frame[4] == k
    frame[6] = 0x04  # subframe type 000010: reserved
    frame[-2:] = flac_bits.crc16(bytes(frame[:-2])).to_bytes(2, "big")
    return flac[:at] + bytes(frame) + flac[at + sizes[k]:]


def test_a_frame_damaged_in_the_reach_only_is_bad_frame(sources):
    """Frame 5 of the 192-block stereo file is damaged.  At 160/147 a window whose output samples
    all sit in frames 6 and 7, but whose filter reaches back into frame 5, is BAD_FRAME and writes
    nothing; one further on and one of another file are intact."""
    import flacgpu

    damaged = _break_frame(sources["s44"][0], 5)
    L, M, Hw, T = ref.ratio(44100, 48000)
    # outputs whose centre sample is at or after source sample 6 * 192 + 2, within Hw - 1 of frame 5
    start = -(-(6 * 192 + 2) * L // M)
    lo, hi = ref.source_range(SOURCES["s44"][5], L, M, Hw, start, 100)
    assert 5 * 192 <= lo < 6 * 192 <= start * M // L and hi < 8 * 192
    far = -(-(6 * 192 + Hw + 5) * L // M)  # the reach ends after frame 5
    assert ref.source_range(SOURCES["s44"][5], L, M, Hw, far, 100)[0] >= 6 * 192
    windows = [(0, start, 100), (0, far, 100), (1, 500, 700), (0, 0, 50), (0, start - 300, 200)]
    with flacgpu.Decoder(2, 16, 44100, device=0, max_frames=8, block_size=4096) as d:
        r = Resident(d, [(tgd._bare(damaged), 16, 44100), (tgd._bare(sources["s48"][0]), 16, 48000)])
        clean = Resident(d, [(tgd._bare(sources["s44"][0]), 16, 44100), (tgd._bare(sources["s48"][0]), 16, 48000)])
        sizes = [2 * 100, 2 * 100, 2 * 700, 2 * 50, 2 * 200]
        offs, size = layout(sizes, F32)
        for flags in (PAD, PLANAR | PAD):
            out, res = resample_call(r, windows, F32, flags, [1, 2], 44100, 48000, offs, sizes, size)
            ref_out, ref_res = resample_call(clean, windows, F32, flags, [1, 2], 44100, 48000, offs, sizes, size)
            assert [v.status for v in ref_res] == [0] * 5 and [v.status for v in res] == [2, 0, 0, 0, 2]
            for w in (0, 4):
                assert (res[w].n_samples, res[w].first_bad_frame) == (0, 5) and res[w].first_bad_status != 0
            got, want = np.frombuffer(out, dtype=np.uint32).copy(), np.frombuffer(ref_out, dtype=np.uint32).copy()
            for w in (0, 4):  # the damaged windows write nothing, not even padding
                assert (got[offs[w]:offs[w] + sizes[w]] == 0xA5A5A5A5).all()
                want[offs[w]:offs[w] + sizes[w]] = 0xA5A5A5A5
            assert (got == want).all()


# ---- position independence -----------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst,name", [(44100, 48000, "s44"), (48000, 16000, "s48")], ids=["160_147", "1_3"])
def test_position_independence(residents, sources, src, dst, name):
    """The whole resampled stream as one window equals the concatenation of many windows with odd
    boundaries, bit for bit."""
    r, s = residents["st16"], _members("st16").index(name)
    L, M, _, _ = ref.ratio(src, dst)
    out_n = ref.out_total(SOURCES[name][5], L, M)
    cuts, at, step = [0], 0, 1
    while at < out_n:
        at = min(at + step, out_n)
        cuts.append(at)
        step = (step * 7 + 3) % 211 + 1
    pieces = [(s, a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert len(pieces) > 20 and any(p[2] % 2 for p in pieces)
    one, res1 = resample_call(r, [(s, 0, out_n)], F32, 0, [1, 2], src, dst, [0], [2 * out_n], 8 * out_n)
    offs = [2 * p[1] for p in pieces]
    many, res2 = resample_call(r, pieces, F32, 0, [1, 2], src, dst, offs, [2 * p[2] for p in pieces], 8 * out_n)
    assert res1[0].n_samples == out_n and [v.n_samples for v in res2] == [p[2] for p in pieces]
    assert one == many and one != b"\xA5" * len(one)


# ---- independence from the host rule ---------------------------------------------------------------------
@pytest.mark.parametrize("src,dst,name", [(44100, 48000, "s44"), (44100, 16000, "s44")], ids=["up", "down"])
def test_f32_outputs_against_float64(residents, sources, src, dst, name):
    import flacgpu

    r, s = residents["st16"], _members("st16").index(name)
    L, M, Hw, T, = ref.ratio(src, dst)
    out_n = ref.out_total(SOURCES[name][5], L, M)
    out, res = resample_call(r, [(s, 0, out_n)], F32, PLANAR, [1, 2], src, dst, [0], [2 * out_n], 8 * out_n)
    assert res[0].status == 0 and res[0].n_samples == out_n
    got = np.frombuffer(out, dtype=np.float32).reshape(2, out_n)
    table = flacgpu.resample_filter(src, dst)[3]
    x = mix_elements(sources[name][1], 16, F32, [1, 2]).view(np.float32)
    for ch in range(2):
        y64, bound = ref.resample64(np.ascontiguousarray(x[:, ch]), src, dst, 0, out_n, table)
        bad = np.nonzero(np.abs(got[ch].astype(np.float64) - y64) > bound)[0]
        assert len(bad) == 0, (ch, [(int(i), float(got[ch][i]), float(y64[i])) for i in bad[:5]])


# ---- refusals that need a context -------------------------------------------------------------------------
def test_refusals_on_a_context(residents):
    import flacgpu

    r = residents["st16"]
    w = [(0, 0, 10)]
    for fmt, masks, src, dst in ((F32, [1, 2], 44100, 44100), (I32, [1, 2], 44100, 48000), (F32, [1, 2], 192000, 8000),
                                 (F32, [4], 44100, 48000), (F32, [], 44100, 48000), (F32, [1] * 9, 44100, 48000),
                                 (F32, [1, 2], 0, 48000), (4, [1, 2], 44100, 48000)):
        with pytest.raises(flacgpu.FlacGpuError) as e:
            resample_call(r, w, fmt, PAD, masks, src, dst, [0], [100], 1024)
        assert e.value.code == -2, (fmt, masks, src, dst)
    with pytest.raises(flacgpu.FlacGpuError):
        resample_call(r, w, F32, 4, [1, 2], 44100, 48000, [0], [100], 1024)  # an unknown flag


# ---- FlacBank.crops(rate=) and FlacMixBank(sample_rate=) ---------------------------------------------------
LENGTH = 300


def _expected_crops(sources, names, crops, K, fmt, planar, rate, masks_of):
    want = np.zeros((len(crops), LENGTH, K), dtype=np.uint32 if ESZ[fmt] == 4 else np.uint16)
    n = []
    for w, (f, start) in enumerate(crops):
        name = names[f]
        C, bits, src = SOURCES[name][1], SOURCES[name][2], SOURCES[name][3]
        masks = masks_of[C]
        if src == rate:
            el = mix_elements(sources[name][1][start:start + LENGTH], bits, fmt, masks)
        else:
            el = narrow(np.ascontiguousarray(whole_f32(sources, name, masks, src, rate)[start:start + LENGTH]), fmt)
        want[w, :len(el)] = el
        n.append(len(el))
    return (want.transpose(0, 2, 1) if planar else want), n


def _crops_of(names, rate):
    crops = []
    for f, name in enumerate(names):
        src = SOURCES[name][3]
        out_n = SOURCES[name][5] if src == rate else ref.out_total(SOURCES[name][5], *ref.ratio(src, rate)[:2])
        crops += [(f, 10), (f, out_n // 2), (f, max(out_n - 120, 0)), (f, out_n + 3)]
    return crops[::2] + crops[1::2]  # the files' crops interleaved


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [F32, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_flacbank_crops_at_a_rate(sources, fmt, planar):
    import flacbank

    torch, _ = tgd._torch()
    names = ["s44", "s48", "s16"]
    crops = _crops_of(names, 48000)
    f, s = [c[0] for c in crops], [c[1] for c in crops]
    with flacbank.FlacBank([sources[n][0] for n in names], device=0, max_frames=8) as b:
        assert b.sample_rates == [44100, 48000, 16000]
        assert b.samples_at(48000) == [ref.out_total(SOURCES["s44"][5], 160, 147), SOURCES["s48"][5], 3 * SOURCES["s16"][5]]
        x, n = b.crops(f, s, LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar, rate=48000)
        want, want_n = _expected_crops(sources, names, crops, 2, fmt, planar, 48000, {2: [1, 2]})
        assert n == want_n and 120 in n and 0 in n and LENGTH in n
        assert (tgd._bits_of(x, fmt) == want).all()
        # files already at the rate: today's output, bit for bit
        own = [(w, c) for w, c in enumerate(crops) if c[0] == 1]
        y, n_own = b.crops([1] * len(own), [c[1] for _, c in own], LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar)
        assert n_own == [n[w] for w, _ in own]
        assert (tgd._bits_of(y, fmt) == tgd._bits_of(x, fmt)[[w for w, _ in own]]).all()
        with pytest.raises(ValueError, match="int32"):
            b.crops(f, s, LENGTH, dtype=torch.int32, rate=48000)
        with pytest.raises(ValueError, match=r"file 2 is at 16000 Hz"):
            b.crops([2], [0], LENGTH, rate=44101)  # 16000 -> 44101 has no common factor: L = 44101
        with pytest.raises(ValueError, match=r"file 0 is at 44100 Hz"):
            b.samples_at(44101)


def test_flacmixbank_with_a_sample_rate(sources):
    """A mixed-rate, mixed-format bank in one crops call, against the per-file expectation."""
    import flacbank

    torch, _ = tgd._torch()
    names = ["m44", "s48", "t48", "s16", "e44", "w44", "m16"]
    files = [sources[n][0] for n in names]
    crops = _crops_of(names, 48000)
    f, s = [c[0] for c in crops], [c[1] for c in crops]
    masks_of = {1: [1], 2: [3]}
    with flacbank.FlacMixBank(files, channels=1, device=0, max_frames=8, sample_rate=48000) as b:
        assert b.sample_rate == 48000 and b.samples == [SOURCES[n][5] for n in names]
        assert b.out_samples == [SOURCES[n][5] if SOURCES[n][3] == 48000 else
                                 ref.out_total(SOURCES[n][5], *ref.ratio(SOURCES[n][3], 48000)[:2]) for n in names]
        for fmt, planar in ((F16, False), (F32, True)):
            x, n = b.crops(f, s, LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar)
            want, want_n = _expected_crops(sources, names, crops, 1, fmt, planar, 48000, masks_of)
            assert n == want_n and (tgd._bits_of(x, fmt) == want).all()
        with pytest.raises(ValueError, match="int32"):
            b.crops(f, s, LENGTH, dtype=torch.int32)
    # the same files at their own rate through a bank without the keyword: today's output for those at 48000
    with flacbank.FlacMixBank(files, channels=1, device=0, max_frames=8) as plain:
        assert not hasattr(plain, "out_samples") and plain.sample_rate is None
        own = [(w, c) for w, c in enumerate(crops) if SOURCES[names[c[0]]][3] == 48000]
        y, _ = plain.crops([c[0] for _, c in own], [c[1] for _, c in own], LENGTH)
        assert len(own) == 8 and (tgd._bits_of(y, F32) == tgd._bits_of(x, F32)[[w for w, _ in own]]).all()
