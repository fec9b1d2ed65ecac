"""Sample windows delivered as short-time power spectra and filter-bank rows on the GPU:
flacgpu_decode_windows_device_features (k_features on the f32-input MFMA), FlacBank.features and
FlacMixBank.features.

The expected values are never the code under test: a stream's whole F32 signal comes from the
existing window calls (flacgpu_decode_windows_device_mix, or _resample where the rates differ), each
channel then goes through the host statement of the rule, flacgpu.features_f32_host (itself checked
against float64 under a derived bound by tests/test_features_host.py), and is narrowed by numpy
(f16) or torch on the CPU (bf16).  Every output buffer is filled with 0xA5 before the call and
compared whole, bit for bit, so the guard elements around every window's region are checked too.
One test compares the device's F32 output with tests/features_ref.py's float64 values directly.

The bit-for-bit comparison is also what decides whether v_mfma_f32_16x16x4_f32 accumulates as a
k-ordered chain of fused multiply-adds: it does, every case below passes on gfx950.

Sources: files of 2 to 4 frames of 4096 at 16 and 24 bits, and one big-block file."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import features_ref as fref  # noqa: E402
import oracle_ref  # noqa: E402
import resample_ref as rref  # noqa: E402
import synth  # noqa: E402
import test_gpu_deliver as tgd  # noqa: E402
from test_gpu_deliver import BF16, ESZ, F16, F32, PAD, PLANAR, layout  # noqa: E402
from test_gpu_resample import _break_frame  # noqa: E402
from window_helpers import NONE, Resident, cover  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (group, channels, bits, rate, block, samples, synth stream); a group is one decode context
SOURCES = {
    "a16": ("st16", 2, 16, 16000, 4096, 3 * 4096 + 500, 90),
    "b44": ("st16", 2, 16, 44100, 4096, 2 * 4096 + 77, 91),
    "c48": ("st16", 2, 16, 48000, 4096, 2 * 4096 + 900, 92),
    "m16": ("mo16", 1, 16, 16000, 4096, 2 * 4096 + 333, 93),
    "big": ("mo16", 1, 16, 16000, 16384, 16384 + 700, 94),
    "t24": ("st24", 2, 24, 16000, 4096, 4096 + 1000, 95),
}
GROUPS = {"st16": (2, 16, 4096), "mo16": (1, 16, 16384), "st24": (2, 24, 4096)}
GEOMETRY = {(64, 16, 0): 32, (34, 7, 1): 32, (400, 160, 80): 32, (512, 128, 0): 32, (2048, 512, 128): 8, (2048, 2048, 0): 4}


def _members(group):
    return [n for n, s in SOURCES.items() if s[0] == group]


@pytest.fixture(scope="module")
def sources():
    """{name: (flac file, blocks)}: made once, shared, never changed."""
    out = {}
    for name, (_, ch, bits, rate, block, n, stream) in SOURCES.items():
        pcm = synth.synth_pcm(n, ch, bits, rate, stream=stream)
        out[name] = (oracle_ref.encode_file(pcm, ch, bits, rate, block=block), [block] * (n // block) + ([n % block] if n % block else []))
    return out


@pytest.fixture(scope="module")
def residents(sources):
    import flacgpu

    with contextlib.ExitStack() as stack:
        out = {}
        for g, (ch, bits, block) in GROUPS.items():
            d = stack.enter_context(flacgpu.Decoder(ch, bits, 16000, device=0, max_frames=8, block_size=block))
            names = _members(g)
            r = Resident(d, [(tgd._bare(sources[n][0]), bits, SOURCES[n][3]) for n in names])
            assert r.totals == [SOURCES[n][5] for n in names]
            out[g] = r
        yield out


def filters_for(n_fft, rows, seed=0):
    """A filter bank of `rows` rows: overlapping bands with zeros elsewhere (mel_filters where it has the shape)."""
    import flacbank

    B = n_fft // 2 + 1
    if rows == 0:
        return None
    if rows >= 8 and seed == 0:
        return flacbank.mel_filters(16000, n_fft, rows)
    rng = np.random.RandomState(seed + rows)
    F = np.zeros((rows, B), dtype=np.float32)
    for r in range(rows):
        lo = (r * B) // (rows + 1)
        F[r, lo:min(B, lo + max(3, (2 * B) // (rows + 1)))] = rng.uniform(0.1, 1.0, min(B, lo + max(3, (2 * B) // (rows + 1))) - lo)
    return F


# ---- the expectation -------------------------------------------------------------------------------
_WHOLE = {}


def out_total(name, src, dst):
    n = SOURCES[name][5]
    return n if not src else rref.out_total(n, *rref.ratio(src, dst)[:2])


def whole_f32(residents, name, masks, src, dst):
    """The stream's whole delivered signal, float32 [K, total]: from the existing window calls."""
    key = (name, None if masks is None else tuple(masks), src, dst)
    if key not in _WHOLE:
        group = SOURCES[name][0]
        r, s = residents[group], _members(group).index(name)
        eff = masks if masks is not None else [1 << c for c in range(GROUPS[group][0])]
        K, total = len(eff), out_total(name, src, dst)
        w = [(s, 0, total)]
        if src:
            out, res = r._call(w, 4 * K * total + 64, lambda o, rs: r.d.decode_windows_device_resample(
                *r._tables(), w, F32, PLANAR | PAD, eff, src, dst, o, [0], [K * total], rs, stream=r.st))
        else:
            out, res = r._call(w, 4 * K * total + 64, lambda o, rs: r.d.decode_windows_device_mix(
                *r._tables(), w, F32, PLANAR | PAD, eff, o, [0], [K * total], rs, stream=r.st))
        assert res[0].status == 0 and res[0].n_samples == total
        x = np.frombuffer(out, dtype=np.float32)[:K * total].reshape(K, total).copy()
        x.setflags(write=False)
        _WHOLE[key] = x
    return _WHOLE[key]


def narrow(y, fmt):
    import torch

    if fmt == F32:
        return y.view(np.uint32)
    if fmt == F16:
        with np.errstate(over="ignore"):
            return y.astype(np.float16).view(np.uint16)
    return torch.from_numpy(np.array(y, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def expected(residents, name, masks, src, dst, n_fft, hop, F, start, frames):
    """([K, rows, frames] float32, n) by the host rule over the whole signal."""
    import flacgpu

    x = whole_f32(residents, name, masks, src, dst)
    ys, n = [], 0
    for k in range(x.shape[0]):
        y, n = flacgpu.features_f32_host(np.ascontiguousarray(x[k]), n_fft, hop, start, frames, F)
        ys.append(y)
    return np.stack(ys), n


def feat_call(r, windows, fmt, masks, src, dst, n_fft, hop, F, offs, caps, size):
    return r._call(windows, size, lambda out, res: r.d.decode_windows_device_features(
        *r._tables(), windows, fmt, masks, src, dst, n_fft, hop, F, out, offs, caps, res, stream=r.st))


def run(residents, sources, group, windows, n_fft, hop, F, fmt=F32, masks=None, src=0, dst=0, short=None, expect_status=None):
    """One call: the windows [(file of the group, start, frames)], each with exactly the capacity it
    needs (short: {window: elements less}) at every destination alignment in turn; every result and
    the whole buffer checked -> the results."""
    r, names = residents[group], _members(group)
    K = len(masks) if masks is not None else GROUPS[group][0]
    rows = F.shape[0] if F is not None else n_fft // 2 + 1
    sizes = [K * rows * fr - (short or {}).get(w, 0) for w, (_, _, fr) in enumerate(windows)]
    offs, size = layout(sizes, fmt)
    out, res = feat_call(r, windows, fmt, masks, src, dst, n_fft, hop, F, offs, sizes, size)
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    for w, ((s, start, frames), v) in enumerate(zip(windows, res)):
        name = names[s]
        if expect_status and w in expect_status:
            st, bad = expect_status[w]
            assert (v.status, v.n_samples, v.first_bad_frame) == (st, 0, bad), (w, v.status, v.n_samples, v.first_bad_frame)
            continue
        y, n = expected(residents, name, masks, src, dst, n_fft, hop, F, start, frames)
        assert (v.status, v.n_samples, v.first_bad_frame, v.first_bad_status) == (0, n, NONE, 0), (w, v.status, v.n_samples, n)
        if not src:  # the covering frames of [start - N / 2, start + (frames - 1) H + N / 2) inside the stream
            total = SOURCES[name][5]
            lo, hi = max(0, start - n_fft // 2), min(total, start + (frames - 1) * hop + n_fft // 2) if frames else 0
            if hi > lo:
                first, nfr, _ = cover(sources[name][1], lo, hi - lo)
                assert (v.first_frame, v.n_frames) == (first, nfr), w
            else:
                assert v.n_frames == 0, w
        want[offs[w]:offs[w] + K * rows * frames] = narrow(np.ascontiguousarray(y), fmt).reshape(-1)
    got = np.frombuffer(out, dtype=dt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
    return res


def usual_windows(s, other, total, other_total, n_fft, hop, tile):
    """Of file s with `total` samples (and one of file `other`): from 0, a start inside the first
    half window, frames that run past the end, starts at and past the end, one frame, one frame over
    a tile, two tiles and one, two that overlap, and the window in the second file."""
    last = max(total - 3 * hop, 0)
    return [(s, 0, 5), (s, n_fft // 4 + 1, 3), (s, last, 8), (s, total, 2), (s, total + 2 * n_fft, 2), (s, 1000, 1),
            (s, 37, tile + 1), (s, 0, 2 * tile + 1), (s, 2000, 4), (s, 2000 + hop, 4), (other, other_total // 3, 3), (s, 500, 0)]


# ---- 1. bit for bit, F32 ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,rows", list(GEOMETRY), ids=[f"{k[0]}_{k[1]}_{k[2]}" for k in GEOMETRY])
def test_f32_bit_for_bit(residents, sources, n_fft, hop, rows):
    big = n_fft == 2048
    masks = [3] if big else None  # the mono mean where the host rule is slow: half the expectation
    F = filters_for(n_fft, rows)
    total, other = SOURCES["a16"][5], SOURCES["c48"][5]
    windows = usual_windows(0, 2, total, other, n_fft, hop, GEOMETRY[(n_fft, hop, rows)])
    res = run(residents, sources, "st16", windows, n_fft, hop, F, masks=masks)
    assert [v.n_samples for v in res[:6]] == [5, 3, 3, 0, 0, 1] and res[11].n_samples == 0
    assert res[7].n_samples == min(2 * GEOMETRY[(n_fft, hop, rows)] + 1, -(-total // hop))
    if not big:  # and a window of the big-block file in another context
        run(residents, sources, "mo16", [(1, 16384 - 10, 3), (0, 5, 2), (1, 0, 2)], n_fft, hop, F)


# ---- 2. narrowed formats ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("n_fft,hop,rows", [(400, 160, 80), (64, 16, 0)], ids=["400_160_80", "64_16_0"])
def test_narrowed_formats(residents, sources, fmt, n_fft, hop, rows):
    total = SOURCES["a16"][5]
    windows = usual_windows(0, 2, total, SOURCES["c48"][5], n_fft, hop, 32)
    assert len(windows) >= 8  # layout() gives window w the alignment w mod 8: heads and tails of every length
    run(residents, sources, "st16", windows, n_fft, hop, filters_for(n_fft, rows), fmt=fmt)


def test_f16_rounds_large_power_to_infinity(residents, sources):
    """A full-scale bank of ones over 1025 bins passes 65504: F16 says infinity, BF16 and F32 the value."""
    F = np.full((2, 1025), 64.0, dtype=np.float32)
    for fmt in (F16, BF16):
        run(residents, sources, "st16", [(0, 3000, 6)], 2048, 512, F, fmt=fmt, masks=[1])
    y, _ = expected(residents, "a16", [1], 0, 0, 2048, 512, F, 3000, 6)
    assert y.max() > 65520.0 and (narrow(y, F16) == 0x7C00).any()


# ---- 3. mixes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,s,masks", [("st16", 0, [3]), ("st16", 0, [1, 2]), ("mo16", 0, [1, 1]), ("st16", 1, None),
                                           ("st24", 0, [2, 0, 3])], ids=["mono_mean", "identity", "mono_to_two", "null", "24bit_swap_silence_mean"])
def test_mixes(residents, sources, group, s, masks):
    name = _members(group)[s]
    total = SOURCES[name][5]
    windows = [(s, 0, 7), (s, 123, 40), (s, total - 500, 9), (s, total + 1000, 2)]
    run(residents, sources, group, windows, 400, 160, filters_for(400, 80), masks=masks)
    run(residents, sources, group, windows[:2], 64, 16, None, masks=masks, fmt=BF16)


# ---- 4. rates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,src", [("b44", 44100), ("c48", 48000)], ids=["441_160", "3_1"])
def test_rates(residents, sources, name, src):
    s = _members("st16").index(name)
    total = out_total(name, src, 16000)
    windows = [(s, 0, 6), (s, 77, 35), (s, total - 400, 6), (s, total, 2), (s, total + 900, 1), (s, 1000, 1)]
    res = run(residents, sources, "st16", windows, 400, 160, filters_for(400, 80), src=src, dst=16000)
    assert [v.n_samples for v in res] == [6, min(35, -(-(total - 77) // 160)), 3, 0, 0, 1]
    run(residents, sources, "st16", windows[:3], 400, 160, filters_for(400, 80), src=src, dst=16000, masks=[3], fmt=F16)


# ---- 5. position independence -----------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst,s", [(0, 0, 0), (44100, 16000, 1)], ids=["own_rate", "resampled"])
def test_position_independence(residents, src, dst, s):
    r = residents["st16"]
    n_fft, hop, frames, start, F = 400, 160, 40, 333, filters_for(400, 80)
    rows, K = 80, 2
    one, res1 = feat_call(r, [(s, start, frames)], F32, None, src, dst, n_fft, hop, F, [0], [K * rows * frames], 4 * K * rows * frames)
    whole = np.frombuffer(one, dtype=np.uint32).reshape(K, rows, frames)
    assert res1[0].status == 0 and res1[0].n_samples > 0
    for j in (1, 7, 33, 39):
        fr = frames - j
        part, res2 = feat_call(r, [(s, start + j * hop, fr)], F32, None, src, dst, n_fft, hop, F, [0], [K * rows * fr], 4 * K * rows * fr)
        assert res2[0].status == 0
        assert (np.frombuffer(part, dtype=np.uint32).reshape(K, rows, fr) == whole[:, :, j:]).all(), j
    assert len(set(whole.reshape(-1).tolist())) > 1000


# ---- 6. damage and capacity ---------------------------------------------------------------------------------
def test_a_frame_damaged_in_the_reach_only_is_bad_frame(sources):
    """Frame 1 of the first file is damaged.  A window whose frame centres all sit in frame 2, but
    whose first frame reaches 100 samples back into frame 1, is BAD_FRAME and writes nothing; one
    that starts exactly half a window after the frame's end, and one of another file, are intact."""
    import flacgpu

    damaged = _break_frame(sources["a16"][0], 1)
    n_fft, hop, rows = 400, 160, 80
    F = filters_for(n_fft, rows)
    windows = [(0, 8192 + 100, 4), (0, 8192 + 200, 4), (1, 500, 5), (0, 0, 3), (0, 8192 - 700, 3)]
    with flacgpu.Decoder(2, 16, 16000, device=0, max_frames=8, block_size=4096) as d:
        r = Resident(d, [(tgd._bare(damaged), 16, 16000), (tgd._bare(sources["c48"][0]), 16, 48000)])
        clean = Resident(d, [(tgd._bare(sources["a16"][0]), 16, 16000), (tgd._bare(sources["c48"][0]), 16, 48000)])
        sizes = [2 * rows * w[2] for w in windows]
        offs, size = layout(sizes, F32)
        out, res = feat_call(r, windows, F32, None, 0, 0, n_fft, hop, F, offs, sizes, size)
        ref_out, ref_res = feat_call(clean, windows, F32, None, 0, 0, n_fft, hop, F, offs, sizes, size)
        assert [v.status for v in ref_res] == [0] * 5 and [v.status for v in res] == [2, 0, 0, 0, 2]
        for w in (0, 4):
            assert (res[w].n_samples, res[w].first_bad_frame) == (0, 1) and res[w].first_bad_status != 0
        got, want = np.frombuffer(out, dtype=np.uint32).copy(), np.frombuffer(ref_out, dtype=np.uint32).copy()
        for w in (0, 4):  # the damaged windows write nothing
            assert (got[offs[w]:offs[w] + sizes[w]] == 0xA5A5A5A5).all()
            want[offs[w]:offs[w] + sizes[w]] = 0xA5A5A5A5
        assert (got == want).all() and (want != 0xA5A5A5A5).sum() == sum(sizes[w] for w in (1, 2, 3))


def test_too_small_writes_nothing(residents, sources):
    windows = [(0, 100, 10), (1, 4000, 6), (0, 2300, 40)]
    F = filters_for(400, 80)
    res = run(residents, sources, "st16", windows, 400, 160, F, short={1: 1}, expect_status={1: (3, NONE)})
    assert [v.status for v in res] == [0, 3, 0]
    res = run(residents, sources, "st16", windows, 400, 160, F, fmt=BF16, masks=[3], short={2: 1, 0: 800}, expect_status={2: (3, NONE), 0: (3, NONE)})
    assert [v.status for v in res] == [3, 0, 3]
    res = run(residents, sources, "st16", windows, 400, 160, F)
    assert [v.status for v in res] == [0, 0, 0]


# ---- 7. float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,rows,src", [(400, 160, 80, 0), (512, 128, 0, 0), (400, 160, 80, 48000)],
                         ids=["400_160_80", "512_128_0", "400_160_80_resampled"])
def test_f32_output_against_float64(residents, n_fft, hop, rows, src):
    name = "c48" if src else "a16"
    dst = 16000 if src else 0
    r, s = residents["st16"], _members("st16").index(name)
    F = filters_for(n_fft, rows)
    R, frames, start = (rows or n_fft // 2 + 1), 30, 50
    out, res = feat_call(r, [(s, start, frames)], F32, None, src, dst, n_fft, hop, F, [0], [2 * R * frames], 8 * R * frames)
    assert res[0].status == 0
    got = np.frombuffer(out, dtype=np.float32).reshape(2, R, frames)
    x = whole_f32(residents, name, None, src, dst)
    for k in range(2):
        y64, bound, n = fref.features64(x[k], n_fft, hop, start, frames, F)
        err = np.abs(got[k].astype(np.float64) - y64)
        print(f"channel {k}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert n == res[0].n_samples and (err <= bound).all() and bound.max() < y64.max() / 256.0


# ---- 8. the table caches ------------------------------------------------------------------------------------------
def test_alternating_filter_banks_and_n_fft(residents, sources):
    Fa, Fb = filters_for(400, 80), filters_for(400, 80, seed=5)
    assert Fa.shape == Fb.shape and (Fa != Fb).any()
    w = [(0, 700, 9), (2, 100, 4)]
    for F in (Fa, Fb, Fa, Fb):
        run(residents, sources, "st16", w, 400, 160, F)
    for n_fft, hop in ((64, 16), (512, 128), (64, 16), (512, 128), (400, 160)):
        run(residents, sources, "st16", w, n_fft, hop, None, masks=[3])
    for k in range(20):  # more banks than the context keeps: the oldest are dropped and come back
        run(residents, sources, "st16", w[:1], 64, 16, filters_for(64, 3, seed=k % 18 + 1), masks=[1])


# ---- refusals that need a context ------------------------------------------------------------------------------
def test_refusals_on_a_context(residents):
    import flacgpu

    r = residents["st16"]
    lib, ctx = r.d.lib, r.d.ctx
    import ctypes

    ft = flacgpu.Features(64, 16, 0)
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    t = r._tables()
    torch, dev = tgd._torch()
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)

    def call(fmt=F32, K=0, masks=None, src=0, dst=0, ftp=ctypes.byref(ft), F=None, stream=0, start=0, frames=1, cap=66, out=None):
        return lib.flacgpu_decode_windows_device_features(
            ctx, t[0], len(t[1]), u64(*t[1]), t[2], t[3], t[4], t[5], t[6], 1, u32(stream), u64(start), u64(frames), fmt, K, masks,
            src, dst, ftp, F, d_out.data_ptr() if out is None else out, u64(0), u64(cap), d_res.data_ptr(), flacgpu._stream(r.st))

    m = (ctypes.c_uint8 * 8)
    inf = (ctypes.c_float * 66)(*([1.0] * 65 + [float("nan")]))
    assert call(fmt=0) == -2 and call(fmt=4) == -2 and call(ftp=None) == -2
    assert call(ftp=ctypes.byref(flacgpu.Features(66, 67, 0))) == -2 and call(ftp=ctypes.byref(flacgpu.Features(64, 16, 2))) == -2
    assert call(ftp=ctypes.byref(flacgpu.Features(64, 16, 2)), F=inf) == -2
    assert call(src=44100, dst=44100) == -2 and call(src=192000, dst=8000) == -2 and call(src=0, dst=8000) == -2
    assert call(K=1, masks=m(4)) == -2 and call(K=0, masks=m(1)) == -2 and call(K=9, masks=m(1)) == -2 and call(K=1, masks=m(7)) == -2
    assert call(stream=3) == -2 and call(frames=(1 << 31) // 16) == -2 and call(fmt=F16, out=d_out.data_ptr() + 1) == -2
    r.d.sync_check(r.st)
    assert (d_out.cpu().numpy() == 0xA5).all() and (d_res.cpu().numpy() == 0xA5).all()  # nothing ran
    assert call() == 0
    r.d.sync_check(r.st)
    assert flacgpu.WindowResult.from_buffer_copy(d_res.cpu().numpy().tobytes()[:32]).status == 0


# ---- 9. the banks ---------------------------------------------------------------------------------------------------
def test_flacbank_features(sources):
    import flacbank
    import flacgpu

    torch, _ = tgd._torch()
    names = ["a16", "c48"]
    n_fft, hop, frames = 400, 160, 12
    F = flacbank.mel_filters(16000, n_fft, 80)
    with flacbank.FlacBank([sources[n][0] for n in names], device=0, max_frames=8) as b:
        totals = b.samples_at(16000)
        f, s = [1, 0, 0, 1, 0], [100, 0, totals[0] - 500, totals[1] + 50, 4000]
        x, n = b.features(f, s, frames, n_fft, hop, filters=F, rate=16000)
        assert tuple(x.shape) == (5, 2, 80, frames) and x.dtype == torch.float32
        assert n == [min(frames, max(0, -(-(totals[fi] - si) // hop))) for fi, si in zip(f, s)] and n[2] == 4 and n[3] == 0
        got = x.cpu().numpy()
        for w, (fi, si) in enumerate(zip(f, s)):
            sig, _ = b.crops([fi], [0], totals[fi], rate=16000)  # the existing path: [1, 2, total]
            for k in range(2):
                y, _ = flacgpu.features_f32_host(sig[0, k].cpu().numpy(), n_fft, hop, si, frames, F)
                assert (got[w, k].view(np.uint32) == y.view(np.uint32)).all(), (w, k)
        # the logarithm is torch's over the linear call
        lg, n2 = b.features(f, s, frames, n_fft, hop, filters=F, rate=16000, log="log10", floor=1e-6)
        assert n2 == n and torch.equal(lg, torch.log10(x.clamp_min(1e-6)))
        ln, _ = b.features(f, s, frames, n_fft, hop, filters=F, rate=16000, log="ln", dtype=torch.bfloat16)
        assert ln.dtype == torch.bfloat16 and torch.equal(ln, torch.log(x.clamp_min(1e-10)).to(torch.bfloat16))
        # out= is filled in place, bins without a bank, narrowed
        out = torch.full((5, 2, 201, frames), 7.0, dtype=torch.float16, device=b.device)
        y, n3, st = b.features(f, s, frames, n_fft, hop, rate=16000, dtype=torch.float16, out=out, strict=False)
        assert y is out and n3 == n and st == [0] * 5 and not (out == 7.0).any()
        lin, _ = b.features(f, s, frames, n_fft, hop, rate=16000)
        assert torch.equal(out, lin.to(torch.float16))
        with pytest.raises(ValueError, match="out must be"):
            b.features(f, s, frames, n_fft, hop, rate=16000, out=out)  # float32 asked, float16 given
        for kw in (dict(n_fft=401), dict(hop=0), dict(log="log2"), dict(dtype=torch.int32), dict(filters=np.ones((3, 7), np.float32))):
            with pytest.raises(ValueError):
                b.features(f, s, frames, **dict(dict(n_fft=n_fft, hop=hop, rate=16000), **kw))


def test_strict_names_the_crop(sources):
    import flacbank
    import flacgpu

    damaged = _break_frame(sources["a16"][0], 1)
    with flacbank.FlacBank([sources["a16"][0], damaged], device=0, max_frames=8) as b:
        f, s = [0, 1, 1], [5000, 5000, 100]
        with pytest.raises(flacgpu.FlacGpuError, match=r"FlacBank\.features: crop 1 \(file 1, start 5000\) is BAD_FRAME, frame 1"):
            b.features(f, s, 4, 400, 160)
        x, n, st = b.features(f, s, 4, 400, 160, strict=False)
        assert st == [0, 2, 0] and n == [4, 0, 4] and (x[1] == 0).all() and (x[0] != 0).any()
        assert torch_equal(x[0], b.features([0], [5000], 4, 400, 160)[0][0])


def torch_equal(a, b):
    import torch

    return torch.equal(a, b)


def test_flacmixbank_features(sources):
    import flacbank
    import flacgpu

    names = ["a16", "m16", "c48", "t24"]
    n_fft, hop, frames = 400, 160, 9
    F = flacbank.mel_filters(16000, n_fft, 40, scale="htk", norm=None)
    with flacbank.FlacMixBank([sources[n][0] for n in names], channels=1, device=0, max_frames=8, sample_rate=16000) as b:
        f, s = [2, 0, 3, 1, 2], [0, 777, 4000, b.out_samples[1] - 300, 1500]
        x, n = b.features(f, s, frames, n_fft, hop, filters=F)
        assert tuple(x.shape) == (5, 1, 40, frames)
        assert n == [min(frames, -(-(b.out_samples[fi] - si) // hop)) for fi, si in zip(f, s)] and n[3] == 2
        got = x.cpu().numpy()
        for w, (fi, si) in enumerate(zip(f, s)):
            sig, _ = b.crops([fi], [0], b.out_samples[fi])  # [1, 1, total] at 16000, mixed to mono
            y, _ = flacgpu.features_f32_host(sig[0, 0].cpu().numpy(), n_fft, hop, si, frames, F)
            assert (got[w, 0].view(np.uint32) == y.view(np.uint32)).all(), w
