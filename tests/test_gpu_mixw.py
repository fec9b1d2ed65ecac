"""Sample windows delivered with a weighted channel mix on the GPU: flacgpu_decode_windows_device_to
(k_window_elements<MIX_WEIGHTS>, k_window_resample<MIX_WEIGHTS>, stage 1 of the features) and
FlacMixBank with weight matrices and downmix=.

Everything compares bit patterns for equality; there is no tolerance.  The expected elements are
the generators' own PCM (synth.synth_pcm, the PCM test_gpu_mix builds, frame_grammar.case_pcm)
turned into integers with numpy and mixed by tests/mixw_ref.py (the fused multiply-add chain in
float64 with the double rounding corrected), narrowed by numpy (f16) or torch on the CPU (bf16);
they are never an output of the decoder.  Resampled and framed expectations are the library's host
statements of those rules (flacgpu_resample_f32_host, flacgpu_features_f32_host) over the mixw_ref
planes.  Every output buffer is filled with 0xA5 before the call and compared whole, so a stray
write anywhere fails.  Blocks of 256, files of at most 70 frames, contexts of 64 frames per call."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import frame_grammar as fg  # noqa: E402
import mixw_ref  # noqa: E402
import oracle_ref  # noqa: E402
import resample_ref as rref  # noqa: E402
import test_gpu_deliver as tgd  # noqa: E402
import test_gpu_mix as tgm  # noqa: E402
from test_gpu_resample import SIX  # noqa: E402
from test_gpu_deliver import BF16, ESZ, F16, F32, FORMAT_NAMES, I32, PAD, PLANAR, file_ints, ints, layout, need  # noqa: E402,F401
from window_helpers import BITS, BLOCK, NONE, RATE, Resident, cover  # noqa: E402
from window_helpers import ctx, files, resident  # noqa: E402,F401  (fixtures: the five stereo 16-bit files)

pytestmark = pytest.mark.gpu

ALL_FLAGS = tgm.ALL_FLAGS
FLAG_IDS = tgm.FLAG_IDS
DEC_RANGE = 7
MID_SIDE = np.array([[0.5, 0.5], [0.5, -0.5]], dtype=np.float32)


def itu(C, K):
    import flacbank

    return flacbank.downmix_matrix(C, K, "itu")


def mean(C):
    import flacbank

    return flacbank.downmix_matrix(C, 1, "mean")


def dense(K, C, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.05, 1.0, size=(K, C)) * rng.choice([-1.0, 1.0], size=(K, C))).astype(np.float32)


# ---- the expectation -------------------------------------------------------------------------------
def mixw_elements(x, bits, fmt, W):
    """int32 [samples, C] -> the weighted elements' bit patterns [samples, K] by mixw_ref."""
    return mixw_ref.narrow(mixw_ref.mix(x, bits, W))[{F32: 0, F16: 1, BF16: 2}[fmt]]


def to_call(r, windows, fmt, flags, offsets, caps, size, **how):
    """One flacgpu_decode_windows_device_to call on the Resident r into a 0xA5-filled buffer of
    `size` bytes -> (the buffer's bytes, [WindowResult]); offsets and caps in elements."""
    return r._call(windows, size, lambda out, res: r.d.decode_windows_device_to(
        *r._tables(), windows, fmt, flags, out, offsets, caps, res, stream=r.st, **how))


def check_mixw(out, res, windows, blocks_of, ints_of, bits, fmt, flags, W, offsets, caps, expect_status=None):
    """test_gpu_mix.check_mix with the weighted expectation."""
    expect_status = expect_status or {}
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    K = len(W)
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
        el = mixw_elements(ints_of[s][start:start + take], bits, fmt, W)  # [take, K]
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


def run_mixw(r, windows, blocks_of, ints_of, bits, fmt, flags, W, expect_status=None, short=None):
    """The windows with exactly the capacity each needs (short: {window: elements less}), at every
    destination alignment in turn, checked whole -> the results."""
    K = len(W)
    sizes = [K * need(cover(blocks_of[s], start, count)[2], count, flags) - (short or {}).get(w, 0)
             for w, (s, start, count) in enumerate(windows)]
    offs, size = layout(sizes, fmt)
    assert len(sizes) < 4 or {(o * ESZ[fmt]) % 16 for o in offs} == set(range(0, 16, ESZ[fmt]))  # every destination alignment
    out, res = to_call(r, windows, fmt, flags, offs, sizes, size, channel_weights=W)
    check_mixw(out, res, windows, blocks_of, ints_of, bits, fmt, flags, W, offs, sizes, expect_status=expect_status)
    return res


# ---- identity weights: the bytes of _as; {0.5, 0.5}: the bytes of _mix with mask 3 -------------------
@pytest.mark.parametrize("flags", ALL_FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("fmt", [F32, F16, BF16], ids=lambda f: FORMAT_NAMES[f])
def test_identity_and_half_sum_are_the_existing_calls(resident, fmt, flags):
    windows = tgm.stereo_windows()
    blocks_of = tgm.stereo_blocks()
    takes = [cover(blocks_of[s], start, count)[2] for s, start, count in windows]
    for K, W, masks in ((2, np.eye(2, dtype=np.float32), None), (1, [[0.5, 0.5]], [3])):
        sizes = [K * need(t, windows[w][2], flags) for w, t in enumerate(takes)]
        offs, size = layout(sizes, fmt)
        if masks is None:
            ref_out, ref_res = resident.deliver(windows, fmt, flags, offs, sizes, size)
            same_out, same_res = to_call(resident, windows, fmt, flags, offs, sizes, size)  # no weights: _as itself
            assert same_out == ref_out and [tgd._fields(a) for a in same_res] == [tgd._fields(b) for b in ref_res]
        else:
            ref_out, ref_res = tgm.mix_call(resident, windows, fmt, flags, masks, offs, sizes, size)
            same_out, _ = to_call(resident, windows, fmt, flags, offs, sizes, size, channel_masks=masks)  # _mix itself
            assert same_out == ref_out
        out, res = to_call(resident, windows, fmt, flags, offs, sizes, size, channel_weights=W)
        assert [tgd._fields(a) for a in res] == [tgd._fields(b) for b in ref_res]
        assert sum(r.status == 0 and r.n_samples > 0 for r in res) >= 30
        assert out == ref_out and out != b"\xA5" * len(out)


# ---- sources made here: PCM chosen by the test, encoded by the CPU oracle encoder -----------------------
def _limits(ch, bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return ([lo] * ch, [hi] * ch, [lo, hi] * (ch // 2) + [lo] * (ch % 2), [0] * ch, [5] * ch)


MADE = {  # name -> (channels, bits, samples, synth stream, directed rows)
    "mono16": (1, 16, 5 * BLOCK + 100, 60, ()),
    "three16": (3, 16, 5 * BLOCK + 100, 61, _limits(3, 16)),
    "six16": (6, 16, 5 * BLOCK + 9, 62, _limits(6, 16)),
    "six24": (6, 24, 3 * BLOCK + 130, 63, _limits(6, 24)),
    "eight24": (8, 24, 3 * BLOCK + 130, 64, _limits(8, 24)),  # per = 24: a tile is 170 samples, the whole stream several
    "stereo32": (2, 32, 4 * BLOCK + 200, 65, tgm._directed_rows(32)),
}


@pytest.fixture(scope="module")
def made():
    """{name: (flac file, int32 [samples, channels], blocks)}: made once, shared, never changed."""
    out = {}
    for name, (ch, bits, n, stream, rows) in MADE.items():
        pcm = tgm._pcm_with(n, ch, bits, stream, rows)
        flac = oracle_ref.encode_file(pcm, ch, bits, RATE, block=BLOCK)
        x = ints(pcm, ch, bits)
        x.setflags(write=False)
        blocks = [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else [])
        out[name] = (flac, x, blocks)
    return out


@pytest.fixture(scope="module")
def made_res(made):
    """{name: Resident of the made source on a context of its own}, open for the module."""
    import flacgpu

    out, open_ = {}, []
    try:
        for name, (flac, x, blocks) in made.items():
            ch, bits, n = MADE[name][:3]
            d = flacgpu.Decoder(ch, bits, RATE, device=0, max_frames=64, block_size=BLOCK)
            open_.append(d)
            r = Resident(d, [(tgd._bare(flac), bits, RATE)])
            assert r.index == [(0, len(blocks))] and r.totals == [n]
            out[name] = r
        yield out
    finally:
        for d in open_:
            d.close()


def _run_made(made, made_res, name, cases):
    n = MADE[name][2]
    _, x, blocks = made[name]
    for fmt, flags, W in cases:
        res = run_mixw(made_res[name], tgm._made_windows(n), {0: blocks}, {0: x}, MADE[name][1], fmt, flags, W)
        assert [v.n_samples for v in res[4:7]] == [50, 0, 0]
    return x


def test_six_channels_to_stereo_and_mono_itu(made, made_res):
    for name in ("six16", "six24"):
        _run_made(made, made_res, name, [(F32, PLANAR | PAD, itu(6, 2)), (F32, 0, itu(6, 2)), (F16, PAD, itu(6, 2)),
                                         (BF16, PLANAR, itu(6, 2)), (F32, PLANAR, itu(6, 1)), (BF16, 0, itu(6, 1)),
                                         (F16, PLANAR | PAD, itu(6, 1)), (F32, PAD, itu(6, 1))])


def test_three_channels_to_mono_mean(made, made_res):
    _run_made(made, made_res, "three16", [(F32, PLANAR | PAD, mean(3)), (F32, 0, mean(3)), (F16, PLANAR, mean(3)),
                                          (BF16, PAD, mean(3))])


def test_mid_side_of_32_bit_stereo(made, made_res):
    x = _run_made(made, made_res, "stereo32", [(F32, PLANAR | PAD, MID_SIDE), (F32, 0, MID_SIDE), (F16, PLANAR, MID_SIDE),
                                               (BF16, PAD, MID_SIDE)])
    f = x.astype(np.float32).astype(np.float64) != x.astype(np.float64)
    assert f.sum() > 100  # samples whose own conversion to float rounds


def test_eight_channels_24_bit_dense(made, made_res):
    """per = 24: 170 samples a tile, so the whole-stream window takes several; 8 x 8 seeded weights."""
    W = dense(8, 8, 88)
    _run_made(made, made_res, "eight24", [(F32, PLANAR | PAD, W), (F32, 0, W), (BF16, PAD, W), (F16, PLANAR, W)])


def test_zero_columns_and_a_zero_row(made, made_res):
    """Channels 1 and 3 are under zero weights in every row (they are passed over), row 1 is all
    zero (of both signs): bit pattern 0 everywhere."""
    W = dense(3, 6, 5)
    W[:, 1] = 0.0
    W[:, 3] = -0.0
    W[1, :] = [0.0, -0.0, 0.0, 0.0, -0.0, 0.0]
    n = MADE["six16"][2]
    _, x, blocks = made["six16"]
    for fmt, flags in ((F32, PLANAR | PAD), (F32, 0), (BF16, PLANAR), (F16, PAD)):
        run_mixw(made_res["six16"], tgm._made_windows(n), {0: blocks}, {0: x}, 16, fmt, flags, W)
    sizes = [3 * n]
    out, res = to_call(made_res["six16"], [(0, 0, n)], F32, PLANAR, [0], sizes, 4 * 3 * n + 64, channel_weights=W)
    planes = np.frombuffer(out, dtype=np.uint32)[:3 * n].reshape(3, n)
    assert res[0].n_samples == n and (planes[1] == 0).all() and (planes[0] != 0).any() and (planes[2] != 0).any()


# ---- statuses ------------------------------------------------------------------------------------------
def test_too_small_is_by_the_output_channels(resident, file_ints):
    windows = [(0, 100, 300), (3, 4000, 600), (1, 3, 200)]
    for flags in (PAD, PAD | PLANAR, 0):
        for W in (np.array([[0.25, 0.75]], dtype=np.float32), dense(3, 2, 9)):
            res = run_mixw(resident, windows, tgm.stereo_blocks(), file_ints, BITS, F32, flags, W, short={1: 1},
                           expect_status={1: (3, NONE, 0)})
            assert [r.status for r in res] == [0, 3, 0]
            res = run_mixw(resident, windows, tgm.stereo_blocks(), file_ints, BITS, F32, flags, W)
            assert [r.status for r in res] == [0, 0, 0]


def test_bad_frame_writes_nothing_and_harms_no_neighbour():
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
            res = run_mixw(r, windows, {0: blocks}, {0: x}, 24, F32, flags, [[1.0], [-0.5]], expect_status=bad)
            assert [v.status for v in res] == [0, 2, 0, 2, 0, 2, 0]


def test_invalid_weights_are_refused_by_a_context(resident):
    """On a stereo context: the call returns INVALID_INPUT and the buffer keeps its 0xA5."""
    import flacgpu

    torch, dev = tgd._torch()
    windows = [(0, 0, 10)]
    cases = [(F32, [[1.0, 0.5, 0.5]], {}), (F32, [[float("nan"), 1.0]], {}), (F32, [[1.0, float("-inf")]], {}), (F32, [[2.0 ** 33, 1.0]], {}),
             (F32, [[1e-40, 1.0]], {}), (I32, [[1.0, 0.0], [0.0, 1.0]], {}), (F32, [[1.0, 1.0]] * 9, {}),
             (F32, [[0.5, 0.5]], {"channel_masks": [3]}), (F32, [[0.5, 0.5]], {"src_rate": 44100, "dst_rate": 44100}),
             (F32, [[0.5, 0.5]], {"n_fft": 64, "hop": 16, "flags": PLANAR})]
    for fmt, W, how in cases:
        flags = how.pop("flags", PAD)
        d_out = torch.full((1024,), 0xA5, dtype=torch.uint8, device=dev)
        d_res = torch.full((32,), 0xA5, dtype=torch.uint8, device=dev)
        with pytest.raises(flacgpu.FlacGpuError) as e:
            resident.d.decode_windows_device_to(*resident._tables(), windows, fmt, flags, d_out.data_ptr(), [0], [100],
                                                d_res.data_ptr(), channel_weights=W, stream=resident.st, **how)
        assert e.value.code == -2, (W, how)
        resident.d.sync_check(resident.st)
        assert d_out.cpu().numpy().tobytes() == b"\xA5" * 1024 and d_res.cpu().numpy().tobytes() == b"\xA5" * 32
    out, res = to_call(resident, windows, F32, PAD, [0], [80], 1024, channel_weights=[[0.5, 0.5]] * 8)  # eight output channels
    assert res[0].status == 0 and out[:320] != b"\xA5" * 320 and out[320:] == b"\xA5" * (1024 - 320)


# ---- through the resampler ---------------------------------------------------------------------------
def _tile(L, M, T, K):
    """resample::tile_plan's tile, written out: the largest tile of at most 1024 output samples whose
    K skewed planes fit 64 KiB."""
    words = 65536 // 4 // K
    for tile in range(1024, 0, -1):
        span = (tile - 1) * M // L + 1 + T
        if (span - 1) + ((span - 1) >> 5) + 1 <= words:
            return tile
    raise AssertionError


@pytest.mark.parametrize("fmt,flags", [(F32, PLANAR | PAD), (F32, 0), (BF16, PAD), (F16, PLANAR)],
                         ids=["f32_planar_pad", "f32_interleaved", "bf16_pad", "f16_planar"])
def test_six_to_stereo_through_the_resampler(made, made_res, fmt, flags):
    import flacgpu

    src, dst = 44100, 48000
    assert (src, dst) in SIX and src == RATE
    W = itu(6, 2)
    _, x, blocks = made["six16"]
    n = len(x)
    L, M, Hw, T = rref.ratio(src, dst)
    out_n = rref.out_total(n, L, M)
    tile = _tile(L, M, T, 2)
    assert tile < out_n  # the stream takes more than one tile
    planes = mixw_ref.mix(x, 16, W)
    whole = np.stack([flacgpu.resample_f32_host(np.ascontiguousarray(planes[:, k]), src, dst) for k in range(2)], axis=1)
    assert whole.shape == (out_n, 2)
    windows = [(0, 0, 37), (0, tile - 30, 70), (0, out_n - 41, 100), (0, 0, out_n), (0, 7, 0), (0, out_n + 5, 30)]
    takes = [rref.delivered(n, L, M, start, count) for _, start, count in windows]
    sizes = [2 * need(t, windows[w][2], flags) for w, t in enumerate(takes)]
    offs, size = layout(sizes, fmt)
    out, res = to_call(made_res["six16"], windows, fmt, flags, offs, sizes, size, channel_weights=W, src_rate=src, dst_rate=dst)
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    for w, ((_, start, count), v) in enumerate(zip(windows, res)):
        take = takes[w]
        lo, hi = rref.source_range(n, L, M, Hw, start, take)
        first, frames, _ = cover(blocks, lo, hi - lo)
        assert (v.status, v.n_samples, v.n_frames, v.first_bad_frame) == (0, take, frames, NONE), w
        if frames:
            assert v.first_frame == first, w
        el = mixw_ref.narrow(np.ascontiguousarray(whole[start:start + take]))[{F32: 0, F16: 1, BF16: 2}[fmt]]
        o = offs[w]
        if flags & PLANAR:
            for k in range(2):
                want[o + k * count:o + k * count + take] = el[:, k]
                if flags & PAD:
                    want[o + k * count + take:o + (k + 1) * count] = 0
        else:
            want[o:o + take * 2] = el.reshape(-1)
            if flags & PAD:
                want[o + take * 2:o + count * 2] = 0
    got = np.frombuffer(out, dtype=dt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    assert takes[1] == 70 and takes[2] == 41


# ---- features ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(0, 0), (44100, 16000)], ids=["own_rate", "to_16000"])
def test_three_to_mono_features(made, made_res, src, dst):
    import flacbank
    import flacgpu

    n_fft, hop = 64, 16
    F = flacbank.mel_filters(dst or RATE, n_fft, 8)
    W = mean(3)
    _, x, blocks = made["three16"]
    plane = np.ascontiguousarray(mixw_ref.mix(x, 16, W)[:, 0])
    if src:
        plane = flacgpu.resample_f32_host(plane, src, dst)
    total = len(plane)
    windows = [(0, 0, 5), (0, 17, 3), (0, max(total - 3 * hop, 0), 8), (0, total, 2), (0, 200, 40), (0, 100, 0)]
    sizes = [8 * fr for _, _, fr in windows]
    offs, size = layout(sizes, F32)
    out, res = to_call(made_res["three16"], windows, F32, 0, offs, sizes, size, channel_weights=W, src_rate=src, dst_rate=dst,
                       n_fft=n_fft, hop=hop, filters=F)
    want = np.frombuffer(b"\xA5" * len(out), dtype=np.uint32).copy()
    for w, ((_, start, frames), v) in enumerate(zip(windows, res)):
        y, n = flacgpu.features_f32_host(plane, n_fft, hop, start, frames, F)
        assert (v.status, v.n_samples, v.first_bad_frame) == (0, n, NONE), w
        want[offs[w]:offs[w] + 8 * frames] = y.view(np.uint32).reshape(-1)
    got = np.frombuffer(out, dtype=np.uint32)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
    assert res[2].n_samples == 3 and res[3].n_samples == 0 and (got[offs[4]:offs[4] + 320] != 0).any()


# ---- FlacMixBank ---------------------------------------------------------------------------------------------
LENGTH = 300
BANK = ["mono16", "s2", "three16", "six16", "six24", "eight24", "s1"]  # 1, 2, 3, 6 and 8 channels, 16 and 24 bits


def _bank_sources(files, file_ints, made, names):
    """[(flac, ints, bits)] of the named sources: 'sN' is stereo 16-bit file N of the fixture."""
    out = []
    for name in names:
        if name[0] == "s" and name[1:].isdigit():
            out.append((files[int(name[1:])][0], file_ints[int(name[1:])], 16))
        else:
            out.append((made[name][0], made[name][1], MADE[name][1]))
    return out


def _policy(C, K, downmix, channel_map=None):
    """("masks", masks) or ("weights", W) as FlacMixBank's documented policy gives them."""
    import flacbank

    if channel_map and C in channel_map:
        m = channel_map[C]
        return ("weights", np.asarray(m, dtype=np.float32)) if np.ndim(m) == 2 else ("masks", list(m))
    if C == K or C == 1 or (K == 1 and C in (2, 4, 8)):
        return "masks", tgm._default_masks(C, K)
    return "weights", flacbank.downmix_matrix(C, K, downmix)


def _expected_crops(src, crops, K, fmt, planar, downmix, channel_map=None):
    want = np.zeros((len(crops), LENGTH, K), dtype=np.uint32 if ESZ[fmt] == 4 else np.uint16)
    n = []
    for w, (f, start) in enumerate(crops):
        _, x, bits = src[f]
        form, mix = _policy(x.shape[1], K, downmix, channel_map)
        part = x[start:start + LENGTH]
        el = tgm.mix_elements(part, bits, fmt, mix) if form == "masks" else mixw_elements(part, bits, fmt, mix)
        want[w, :len(el)] = el
        n.append(len(el))
    return (want.transpose(0, 2, 1) if planar else want), n


@pytest.fixture(scope="module")
def banks(files, file_ints, made):
    import flacbank

    src = _bank_sources(files, file_ints, made, BANK)
    with flacbank.FlacMixBank([s[0] for s in src], channels=2, device=0, max_frames=64, downmix="itu") as stereo:
        with flacbank.FlacMixBank([s[0] for s in src], channels=1, device=0, max_frames=64, downmix="mean") as mono:
            yield {2: (stereo, "itu"), 1: (mono, "mean")}, src


@pytest.mark.parametrize("planar", [True, False], ids=["planar", "interleaved"])
@pytest.mark.parametrize("fmt", [F32, BF16], ids=lambda f: FORMAT_NAMES[f])
@pytest.mark.parametrize("K", [2, 1], ids=["stereo_itu", "mono_mean"])
def test_mixbank_downmix(banks, K, fmt, planar):
    by_k, src = banks
    b, kind = by_k[K]
    assert b.file_channels == [1, 2, 3, 6, 6, 8, 2] and b.bits == [16, 24] and len(b._groups) == 6
    assert all(isinstance(g, tuple) and len(g) == 2 for g in b._groups)  # the entries stay pairs
    crops = tgm._shuffled_crops(src, f"mixw{K}")
    x, n = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH, dtype=tgd._torch_dtypes()[fmt], planar=planar)
    want, want_n = _expected_crops(src, crops, K, fmt, planar, kind)
    assert n == want_n and 120 in n and 0 in n and LENGTH in n
    assert tuple(x.shape) == ((len(crops), K, LENGTH) if planar else (len(crops), LENGTH, K)) and x.is_contiguous()
    assert (tgd._bits_of(x, fmt) == want).all()


def test_mixbank_features_and_int32(banks):
    import flacgpu

    torch, _ = tgd._torch()
    by_k, src = banks
    b, _ = by_k[1]
    n_fft, hop, frames = 64, 16, 6
    f, s = [3, 0, 5, 2, 1], [0, 100, 300, len(src[2][1]) - 40, 50]
    x, n = b.features(f, s, frames, n_fft, hop)
    assert tuple(x.shape) == (5, 1, 33, frames) and n[3] == 3
    got = x.cpu().numpy()
    for w, (fi, si) in enumerate(zip(f, s)):
        _, xi, bits = src[fi]
        form, mix = _policy(xi.shape[1], 1, "mean")
        el = tgm.mix_elements(xi, bits, F32, mix) if form == "masks" else mixw_elements(xi, bits, F32, mix)
        y, nw = flacgpu.features_f32_host(np.ascontiguousarray(el[:, 0].view(np.float32)), n_fft, hop, si, frames)
        assert n[w] == nw and (got[w, 0].view(np.uint32) == y.view(np.uint32)).all(), w
    with pytest.raises(ValueError, match="mixed by weights"):
        b.crops([0], [0], LENGTH, dtype=torch.int32)


def test_mixbank_mid_side_map_and_masks_only(files, file_ints, made):
    """channel_map={2: mid/side rows}; and a bank of masks only delivers as before."""
    import flacbank

    src = _bank_sources(files, file_ints, made, ["s2", "mono16", "s1", "stereo32"])
    crops = tgm._shuffled_crops(src, "ms")
    cmap = {2: [[0.5, 0.5], [0.5, -0.5]]}
    with flacbank.FlacMixBank([s[0] for s in src], channels=2, device=0, max_frames=64, channel_map=cmap) as b:
        assert len(b._groups) == 3
        x, n = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH)
    want, want_n = _expected_crops(src, crops, 2, F32, True, None, channel_map=cmap)
    assert n == want_n and (tgd._bits_of(x, F32) == want).all()
    with_masks_only = {2: [2, 1]}
    with flacbank.FlacMixBank([s[0] for s in src], channels=2, device=0, max_frames=64, channel_map=with_masks_only) as b:
        assert all(isinstance(m, list) for _, m in b._groups)
        x, n = b.crops([c[0] for c in crops], [c[1] for c in crops], LENGTH)
    want, want_n = tgm._expected_crops(src, crops, 2, F32, True, masks_of=with_masks_only)
    assert n == want_n and (tgd._bits_of(x, F32) == want).all()
