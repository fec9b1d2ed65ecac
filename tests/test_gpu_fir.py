"""Sample windows delivered convolved with a per-window FIR filter on the GPU:
flacgpu_decode_windows_device_fir (k_window_fir on the f32-input MFMA), FlacBank.crops(fir=) and
FlacMixBank.crops(fir=).

The expected values are never the code under test: a stream's whole F32 signal comes from the
existing window call (flacgpu_decode_windows_device_to: the elements of _as, of the masks, of the
weights, or of _resample where the rates differ, each checked bit for bit against its own host
statement by its own tests), each channel then goes through the host statement of the rule,
flacgpu.fir_f32_host (itself checked against float64 under the derived bound by
tests/test_fir_args.py and tests/test_fir_host.py), and is narrowed by numpy (f16) or torch on the
CPU (bf16).  Every output buffer is filled with 0xA5 before the call and compared whole, bit for bit,
so the guard elements around every window's region are checked too.  The taps lie in device memory
between runs of NaN: a tap read outside a filter's rows would show in every element.

Sources: blocks of 1024 in contexts of 4 frames a chunk, so a window's span crosses chunks."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fir_ref as fref  # noqa: E402
import oracle_ref  # noqa: E402
import resample_ref as rref  # noqa: E402
import synth  # noqa: E402
import test_gpu_deliver as tgd  # noqa: E402
from test_gpu_deliver import BF16, ESZ, F16, F32, PAD, PLANAR, layout  # noqa: E402
from test_gpu_resample import _break_frame  # noqa: E402
from window_helpers import NONE, Resident, cover  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = 1024
# name -> (group, channels, bits, rate, samples, synth stream); a group is one decode context
SOURCES = {
    "a16": ("st16", 2, 16, 44100, 10 * BLOCK + 300, 70),
    "b16": ("st16", 2, 16, 44100, 2 * BLOCK + 77, 71),
    "t24": ("tr24", 3, 24, 16000, 3 * BLOCK + 200, 72),
    "m8": ("mo8", 1, 8, 16000, 2 * BLOCK + 100, 73),
}
GROUPS = {"st16": (2, 16), "tr24": (3, 24), "mo8": (1, 8)}
EDGE = 241  # T + 15 = 256: the last T of one chunk of steps (tests/test_fir_host.py pins it to fir_geometry)


def _members(group):
    return [n for n, s in SOURCES.items() if s[0] == group]


@pytest.fixture(scope="module")
def sources():
    """{name: (flac file, blocks)}: made once, shared, never changed."""
    out = {}
    for name, (_, ch, bits, rate, n, stream) in SOURCES.items():
        pcm = synth.synth_pcm(n, ch, bits, rate, stream=stream)
        out[name] = (oracle_ref.encode_file(pcm, ch, bits, rate, block=BLOCK), [BLOCK] * (n // BLOCK) + ([n % BLOCK] if n % BLOCK else []))
    return out


@pytest.fixture(scope="module")
def residents(sources):
    import flacgpu

    with contextlib.ExitStack() as stack:
        out = {}
        for g, (ch, bits) in GROUPS.items():
            d = stack.enter_context(flacgpu.Decoder(ch, bits, 16000, device=0, max_frames=4, block_size=BLOCK))
            names = _members(g)
            r = Resident(d, [(tgd._bare(sources[n][0]), bits, SOURCES[n][3]) for n in names])
            assert r.totals == [SOURCES[n][4] for n in names]
            out[g] = r
        yield out


# ---- the filters on the device ---------------------------------------------------------------------
class Taps:
    """filters = [(h float32 [T] or [rows, T], delay)] packed at odd offsets between runs of NaN."""

    def __init__(self, filters):
        torch, dev = tgd._torch()
        flat, self.table, self.host = [np.full(3, np.nan, dtype=np.float32)], [], []
        at = 3
        for h, d in filters:
            h = np.asarray(h, dtype=np.float32)
            h2 = h[None, :] if h.ndim == 1 else h
            self.table.append((at, h2.shape[1], d, h2.shape[0]))
            self.host.append((h2, d))
            flat += [h2.reshape(-1), np.full(5, np.nan, dtype=np.float32)]
            at += h2.size + 5
        self.dev = torch.from_numpy(np.concatenate(flat)).to(dev)
        self.len = at
        assert self.dev.numel() == at


# ---- the expectation -------------------------------------------------------------------------------
_WHOLE = {}


def _key(v):
    return None if v is None else np.asarray(v, dtype=np.float32).tobytes()


def out_total(name, src, dst):
    n = SOURCES[name][4]
    return n if not src else rref.out_total(n, *rref.ratio(src, dst)[:2])


def whole_f32(residents, name, masks, weights, src, dst):
    """The stream's whole delivered signal, float32 [K, total]: from the existing window call."""
    key = (name, _key(masks), _key(weights), src, dst)
    if key not in _WHOLE:
        group = SOURCES[name][0]
        r, s = residents[group], _members(group).index(name)
        K = len(masks) if masks is not None else (len(weights) if weights is not None else GROUPS[group][0])
        total = out_total(name, src, dst)
        w = [(s, 0, total)]
        out, res = r._call(w, 4 * K * total + 64, lambda o, rs: r.d.decode_windows_device_to(
            *r._tables(), w, F32, PLANAR | PAD, o, [0], [K * total], rs, channel_masks=masks, channel_weights=weights,
            src_rate=src, dst_rate=dst, stream=r.st))
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


def expected(x, filt, start, count):
    """([K, count] float32, n) by the host rule over the whole signal x [K, total]."""
    import flacgpu

    h, d = filt
    ys, n = [], 0
    for k in range(x.shape[0]):
        y, n = flacgpu.fir_f32_host(np.ascontiguousarray(x[k]), h[k if h.shape[0] > 1 else 0], d, start, count)
        ys.append(y)
    return np.stack(ys), n


def fir_call(r, windows, fmt, flags, taps, wf, offs, caps, size, masks=None, weights=None, src=0, dst=0):
    return r._call(windows, size, lambda out, res: r.d.decode_windows_device_fir(
        *r._tables(), windows, fmt, flags, taps.dev.data_ptr(), taps.len, taps.table, wf, out, offs, caps, res,
        channel_masks=masks, channel_weights=weights, src_rate=src, dst_rate=dst, stream=r.st))


def run(residents, sources, group, windows, taps, wf, fmt=F32, flags=PLANAR | PAD, masks=None, weights=None, src=0, dst=0,
        short=None, expect_status=None):
    """One call: the windows [(file of the group, start, count)], window w through filter wf[w], each
    with exactly the capacity it needs (short: {window: elements less}) at every destination
    alignment in turn; every result and the whole buffer checked -> the results."""
    r, names = residents[group], _members(group)
    K = len(masks) if masks is not None else (len(weights) if weights is not None else GROUPS[group][0])
    exp, sizes = [], []
    for w, (s, start, count) in enumerate(windows):
        x = whole_f32(residents, names[s], masks, weights, src, dst)
        y, n = expected(x, taps.host[wf[w]], start, count)
        exp.append((y, n))
        sizes.append(K * (count if flags else n) - (short or {}).get(w, 0))
    offs, size = layout(sizes, fmt)
    out, res = fir_call(r, windows, fmt, flags, taps, wf, offs, sizes, size, masks, weights, src, dst)
    dt = np.uint32 if ESZ[fmt] == 4 else np.uint16
    want = np.frombuffer(b"\xA5" * len(out), dtype=dt).copy()
    for w, ((s, start, count), v) in enumerate(zip(windows, res)):
        name = names[s]
        if expect_status and w in expect_status:
            st, bad = expect_status[w]
            assert (v.status, v.n_samples, v.first_bad_frame) == (st, 0, bad), (w, v.status, v.n_samples, v.first_bad_frame)
            continue
        y, n = exp[w]
        assert (v.status, v.n_samples, v.first_bad_frame, v.first_bad_status) == (0, n, NONE, 0), (w, v.status, v.n_samples, n)
        if not src:  # the covering frames of [start + d - (T - 1), start + count + d) inside the stream
            _, T, d, _ = taps.table[wf[w]]
            lo, hi = max(0, start + d - (T - 1)), min(SOURCES[name][4], start + count + d) if count else 0
            if hi > lo:
                first, nfr, _ = cover(sources[name][1], lo, hi - lo)
                assert (v.first_frame, v.n_frames) == (first, nfr), w
            else:
                assert v.n_frames == 0, w
        m = count if flags & PAD else n  # the samples written
        e = narrow(np.ascontiguousarray(y), fmt)
        region = want[offs[w]:offs[w] + K * count]  # (a view: K * count elements exist only under PLANAR or PAD)
        if flags & PLANAR:
            for k in range(K):
                region[k * count:k * count + m] = e[k, :m]
        else:
            want[offs[w]:offs[w] + K * m] = e[:, :m].T.reshape(-1)
    got = np.frombuffer(out, dtype=dt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]])
    return res


def usual_windows(s, other, total):
    """Counts 1, 15, 17, 255, 257 and 3000; at sample 0, clipped at the end, wholly outside, empty;
    two that overlap; one in the second file."""
    return [(s, 0, 17), (s, 5, 1), (s, 300, 15), (s, 1000, 255), (s, 1100, 257), (s, 2000, 3000), (s, total - 100, 255),
            (s, total, 15), (s, total + 5000, 17), (s, 400, 0), (other, 50, 257), (s, 0, 3000)]


# ---- 1. every filter length, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 15, 16, 17, EDGE, EDGE + 1, 4096])
def test_f32_bit_for_bit(residents, sources, T):
    total = SOURCES["a16"][4]
    windows = usual_windows(0, 1, total)
    taps = Taps([(fref.taps(T, T), 0), (fref.taps(T, T + 7), (T - 1) // 2), (fref.taps(T, T + 9), T - 1)])
    wf = [w % 3 for w in range(len(windows))]
    res = run(residents, sources, "st16", windows, taps, wf)
    assert [v.n_samples for v in res] == [17, 1, 15, 255, 257, 3000, 100, 0, 0, 0, 257, 3000]
    # the span of 3000 + T - 1 samples crosses the chunks of 4 frames
    assert res[5].n_frames >= 4 and res[11].n_frames >= 3


# ---- 2. layouts and narrowed formats -------------------------------------------------------------------
@pytest.mark.parametrize("fmt,flags", [(F32, 0), (F32, PLANAR), (F32, PAD), (F32, PLANAR | PAD), (F16, PLANAR | PAD), (F16, 0),
                                       (BF16, PAD), (BF16, PLANAR)],
                         ids=["f32", "f32_planar", "f32_pad", "f32_planar_pad", "f16_planar_pad", "f16", "bf16_pad", "bf16_planar"])
def test_layouts_and_formats(residents, sources, fmt, flags):
    total = SOURCES["a16"][4]
    windows = usual_windows(0, 1, total)
    assert len(windows) >= 8  # layout() gives window w the alignment w mod 8: every destination alignment
    taps = Taps([(fref.taps(33, 1), 16), (fref.taps(257, 2) * np.float32(3.0), 0)])
    run(residents, sources, "st16", windows, taps, [w % 2 for w in range(len(windows))], fmt=fmt, flags=flags)


def test_f16_is_infinity_from_65520_on(residents, sources):
    taps = Taps([(np.array([2.0 ** 20, 0.0, 2.0 ** -3], dtype=np.float32), 0)])  # |x| >= 1 / 16 passes 65520
    x = whole_f32(residents, "a16", None, None, 0, 0)
    y, _ = expected(x, taps.host[0], 500, 600)
    assert np.abs(y).max() >= 65520.0
    assert ((narrow(y, F16) & 0x7FFF) == 0x7C00).any()
    for fmt in (F16, BF16):
        run(residents, sources, "st16", [(0, 500, 600)], taps, [0], fmt=fmt)


# ---- 3. several filters in one call ----------------------------------------------------------------------
def test_filters_of_different_lengths_delays_and_rows_in_one_call(residents, sources):
    total = SOURCES["a16"][4]
    two = np.stack([fref.taps(100, 3), fref.taps(100, 4)])  # rows = K: one response a channel
    taps = Taps([(np.array([1.0], dtype=np.float32), 0), (fref.taps(7, 5), 6), (two, 40), (fref.taps(1000, 6), 999),
                 (fref.taps(EDGE + 1, 8), 100)])
    windows = usual_windows(0, 1, total)
    wf = [(w * 3 + 1) % 5 for w in range(len(windows))]
    assert set(wf) == set(range(5))
    run(residents, sources, "st16", windows, taps, wf)
    run(residents, sources, "st16", windows, taps, wf[::-1], fmt=BF16, flags=0)


def test_one_tap_of_one_is_the_unfiltered_crop(residents, sources):
    r = residents["st16"]
    windows = usual_windows(0, 1, SOURCES["a16"][4])
    taps = Taps([(np.array([1.0], dtype=np.float32), 0)])
    for fmt, flags in ((F32, PLANAR | PAD), (F16, 0), (BF16, PAD)):
        sizes = [2 * c for _, _, c in windows]
        offs, size = layout(sizes, fmt)
        got, res = fir_call(r, windows, fmt, flags, taps, [0] * len(windows), offs, sizes, size)
        want, ref = r.deliver(windows, fmt, flags, offs, sizes, size)
        assert got == want
        assert [tgd._fields(v) for v in res] == [tgd._fields(v) for v in ref]


# ---- 4. sources ---------------------------------------------------------------------------------------------
def test_three_channels_of_24_bits(residents, sources):
    total = SOURCES["t24"][4]
    three = np.stack([fref.taps(50, 20 + k) for k in range(3)])
    taps = Taps([(fref.taps(EDGE, 11), 120), (three, 0)])
    windows = [(0, 0, 300), (0, 77, 3000), (0, total - 40, 257), (0, total + 3, 5), (0, 1500, 1)]
    run(residents, sources, "tr24", windows, taps, [0, 1, 0, 1, 1])
    run(residents, sources, "tr24", windows, taps, [1, 0, 1, 0, 0], flags=0)


def test_mono_8_bit_at_every_source_alignment(residents, sources):
    taps = Taps([(fref.taps(17, 31), 8), (fref.taps(16, 32), 0)])
    windows = [(0, 100 + a, 255 + a) for a in range(8)] + [(0, a, 17) for a in range(8)]  # the span starts at every byte mod 8
    run(residents, sources, "mo8", windows, taps, [w % 2 for w in range(16)])
    run(residents, sources, "mo8", windows, taps, [(w + 1) % 2 for w in range(16)], fmt=F16, flags=PAD)


# ---- 5. composition ----------------------------------------------------------------------------------------
def test_with_masks(residents, sources):
    one = [(fref.taps(33, 41), 16), (fref.taps(EDGE + 1, 42), 0)]
    windows = usual_windows(0, 1, SOURCES["a16"][4])
    run(residents, sources, "st16", windows, Taps(one), [w % 2 for w in range(len(windows))], masks=[3])  # the mono mean
    # K = 3 (swap, silence, mean) and a rows = K filter, which a call of one channel would refuse
    taps = Taps(one + [(np.stack([fref.taps(9, 43 + k) for k in range(3)]), 4)])
    run(residents, sources, "st16", windows[:6], taps, [2, 0, 2, 1, 2, 2], masks=[2, 0, 3], flags=PAD)


def test_with_a_weight_matrix(residents, sources):
    W = np.array([[0.5, 0.5], [0.5, -0.5], [1.0 / 3, 0.0]], dtype=np.float32)
    taps = Taps([(fref.taps(64, 51), 63), (np.stack([fref.taps(20, 52 + k) for k in range(3)]), 10)])
    windows = usual_windows(0, 1, SOURCES["a16"][4])
    run(residents, sources, "st16", windows, taps, [w % 2 for w in range(len(windows))], weights=W)
    Wd = np.array([[0.25, 0.5, 0.25]], dtype=np.float32)  # 24-bit, three channels to one
    run(residents, sources, "tr24", [(0, 0, 300), (0, 2000, 3000)], Taps([(fref.taps(64, 51), 63)]), [0, 0], weights=Wd, fmt=BF16)


def test_with_44100_to_48000(residents, sources):
    total = out_total("a16", 44100, 48000)
    taps = Taps([(fref.taps(31, 61), 15), (fref.taps(EDGE + 1, 62), 0)])
    windows = [(0, 0, 257), (0, 1234, 3000), (0, total - 90, 255), (0, total, 15), (0, total + 4000, 17), (1, 10, 17)]
    res = run(residents, sources, "st16", windows, taps, [w % 2 for w in range(6)], src=44100, dst=48000)
    assert [v.n_samples for v in res] == [257, 3000, 90, 0, 0, 17]
    run(residents, sources, "st16", windows[:3], taps, [1, 0, 1], src=44100, dst=48000, masks=[3], fmt=F16, flags=0)


# ---- 6. the statuses that write nothing ---------------------------------------------------------------------
def test_too_small_writes_nothing(residents, sources):
    total = SOURCES["a16"][4]
    taps = Taps([(fref.taps(33, 71), 16)])
    windows = [(0, 100, 300), (1, 40, 600), (0, total - 100, 255)]
    for flags in (PAD, PLANAR, 0):
        res = run(residents, sources, "st16", windows, taps, [0, 0, 0], flags=flags, short={1: 1}, expect_status={1: (3, NONE)})
        assert [v.status for v in res] == [0, 3, 0]
    # without PLANAR or PAD the capacity is that of the clipped window, as in _as: 100 samples fit, 99 do not
    res = run(residents, sources, "st16", windows, taps, [0, 0, 0], flags=0, short={2: 1}, expect_status={2: (3, NONE)})
    assert [v.status for v in res] == [0, 0, 3]


def test_bad_frame_in_the_reach_and_bad_index_write_nothing(sources):
    """Frame 3 of the first file is damaged: a window in frame 4 whose taps reach back into frame 3 is
    BAD_FRAME, one further on is intact; a stream with no frame at offset 0 is BAD_INDEX."""
    import flacgpu

    damaged = _break_frame(sources["a16"][0], 3)
    taps = Taps([(fref.taps(200, 81), 0), (fref.taps(200, 82), 199)])
    windows = [(0, 4 * BLOCK + 100, 300), (0, 4 * BLOCK + 300, 300), (1, 0, 100), (2, 100, 50), (0, 3 * BLOCK - 250, 100),
               (0, 3 * BLOCK - 250, 100)]
    wf = [0, 0, 0, 0, 0, 1]  # the last two: the delay of 199 reaches forward into frame 3, no delay does not
    with flacgpu.Decoder(2, 16, 44100, device=0, max_frames=4, block_size=BLOCK) as d:
        bad = b"\x00" * 7 + tgd._bare(sources["b16"][0])
        r = Resident(d, [(tgd._bare(damaged), 16, 44100), (bad, 16, 44100), (tgd._bare(sources["b16"][0]), 16, 44100)])
        clean = Resident(d, [(tgd._bare(sources["a16"][0]), 16, 44100), (tgd._bare(sources["b16"][0]), 16, 44100),
                             (tgd._bare(sources["b16"][0]), 16, 44100)])
        assert r.index[1][0] == 1
        sizes = [2 * w[2] for w in windows]
        offs, size = layout(sizes, F32)
        out, res = fir_call(r, windows, F32, PLANAR | PAD, taps, wf, offs, sizes, size)
        ref_out, ref_res = fir_call(clean, windows, F32, PLANAR | PAD, taps, wf, offs, sizes, size)
        assert [v.status for v in ref_res] == [0] * 6 and [v.status for v in res] == [2, 0, 1, 0, 0, 2]
        for w in (0, 5):
            assert (res[w].n_samples, res[w].first_bad_frame) == (0, 3) and res[w].first_bad_status != 0
        assert (res[2].n_samples, res[2].n_frames, res[2].first_bad_frame) == (0, 0, NONE)
        got, want = np.frombuffer(out, dtype=np.uint32).copy(), np.frombuffer(ref_out, dtype=np.uint32).copy()
        for w in (0, 2, 5):  # they write nothing
            assert (got[offs[w]:offs[w] + sizes[w]] == 0xA5A5A5A5).all()
            want[offs[w]:offs[w] + sizes[w]] = 0xA5A5A5A5
        assert (got == want).all() and (want != 0xA5A5A5A5).sum() == sum(sizes[w] for w in (1, 3, 4))


# ---- refusals that need a context ------------------------------------------------------------------------------
def test_refusals_on_a_context(residents):
    import ctypes

    import flacgpu

    r = residents["st16"]
    lib, ctx = r.d.lib, r.d.ctx
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    t = r._tables()
    torch, dev = tgd._torch()
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    d_taps = torch.ones(64, dtype=torch.float32, device=dev)
    ft = flacgpu.Features(64, 16, 0)
    m = (ctypes.c_uint8 * 8)

    def call(fmt=F32, flags=0, K=0, masks=None, weights=None, src=0, dst=0, features=None, size=None, fil=(0, 16, 0, 1, 0), taps_len=64,
             taps=None, n_filters=1, wf=0, stream=0, count=10, cap=64, out=None):
        how = flacgpu.WindowDelivery(ctypes.sizeof(flacgpu.WindowDelivery) if size is None else size, fmt, flags, K,
                                     ctypes.cast(masks, ctypes.c_void_p) if masks is not None else None,
                                     ctypes.cast(weights, ctypes.c_void_p) if weights is not None else None, src, dst, features, None)
        return lib.flacgpu_decode_windows_device_fir(
            ctx, t[0], len(t[1]), u64(*t[1]), t[2], t[3], t[4], t[5], t[6], 1, u32(stream), u64(0), u64(count), ctypes.byref(how),
            d_taps.data_ptr() if taps is None else taps, taps_len, n_filters, (flacgpu.Fir * 1)(flacgpu.Fir(*fil)), u32(wf),
            d_out.data_ptr() if out is None else out, u64(0), u64(cap), d_res.data_ptr(), flacgpu._stream(r.st))

    assert call(fmt=0) == -2 and call(fmt=4) == -2 and call(flags=4) == -2 and call(size=48) == -2
    assert call(features=ctypes.cast(ctypes.pointer(ft), ctypes.c_void_p)) == -2
    assert call(taps=0) == -2 and call(taps=d_taps.data_ptr() + 2) == -2
    assert call(fil=(0, 0, 0, 1, 0)) == -2 and call(fil=(0, 4097, 0, 1, 0), taps_len=1 << 20) == -2
    assert call(fil=(0, 16, 16, 1, 0)) == -2                                   # delay >= taps
    assert call(fil=(0, 16, 0, 3, 0)) == -2 and call(fil=(0, 16, 0, 0, 0)) == -2  # rows neither 1 nor K = 2
    assert call(fil=(0, 16, 0, 1, 0), K=3, masks=m(1, 2, 3)) == 0 and call(fil=(0, 16, 0, 2, 0), K=3, masks=m(1, 2, 3)) == -2
    assert call(fil=(0, 16, 0, 1, 7)) == -2                                    # reserved
    assert call(fil=(49, 16, 0, 1, 0)) == -2 and call(fil=(33, 16, 0, 2, 0)) == -2  # offset + rows * taps > taps_len
    assert call(wf=1) == -2 and call(n_filters=0) == -2
    assert call(count=(1 << 31) - 15) == -2                                    # count + taps - 1 = 2^31
    assert call(src=44100, dst=44100) == -2 and call(src=0, dst=8000) == -2
    assert call(K=1, masks=m(4)) == -2 and call(K=1, masks=m(1), weights=(ctypes.c_float * 2)(0.5, 0.5)) == -2
    assert call(K=1, weights=(ctypes.c_float * 2)(0.5, float("nan"))) == -2
    assert call(stream=3) == -2 and call(fmt=F16, out=d_out.data_ptr() + 1) == -2
    r.d.sync_check(r.st)
    assert (d_out.cpu().numpy()[256:] == 0xA5).all()  # only the one valid call above wrote, inside its 64 elements
    assert call() == 0
    r.d.sync_check(r.st)
    assert flacgpu.WindowResult.from_buffer_copy(d_res.cpu().numpy().tobytes()[:32]).status == 0


# ---- 7. the banks ---------------------------------------------------------------------------------------------------
def _bank_windows(b, tables, file, start, length, fmt, flags, fir, fir_index, K, **kw):
    """The C call for the same crops over the bank's own tables -> the elements as a numpy array."""
    torch, dev = tgd._torch()
    W = len(file)
    out = torch.zeros(W * K * length, dtype={F32: torch.float32, F16: torch.float16}[fmt], device=dev)
    d_res = torch.zeros(32 * W, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    b._dec.decode_windows_device_fir(*tables, [(f, s, length) for f, s in zip(file, start)], fmt, flags, fir.taps.data_ptr(),
                                     fir.taps.numel(), fir.table, fir_index, out.data_ptr(), [w * K * length for w in range(W)],
                                     [K * length] * W, d_res.data_ptr(), stream=st, **kw)
    b._dec.sync_check(st)
    return out.cpu().numpy().view(np.uint32 if fmt == F32 else np.uint16)


def test_flacbank_crops_with_a_filter(sources):
    import flacbank
    import flacgpu

    torch, _ = tgd._torch()
    h, d = flacbank.fir_windowed_sinc(44100, 300, 3400, 255)
    with flacbank.FlacBank([sources["a16"][0], sources["b16"][0]], device=0, max_frames=4) as b:
        fir = flacbank.FirBank([h, [1.0], np.stack([fref.taps(40, 1), fref.taps(40, 2)])], delays=[d, 0, 39], device=0)
        assert len(fir) == 3 and fir.table == [(0, 255, 127, 1), (255, 1, 0, 1), (256, 40, 39, 2)]
        f, s, idx = [0, 1, 0, 0, 1], [0, 100, b.samples[0] - 50, 5000, 1000], [0, 2, 1, 2, 1]
        x, n = b.crops(f, s, 300, fir=fir, fir_index=idx)
        assert tuple(x.shape) == (5, 2, 300) and x.dtype == torch.float32 and n == [300, 300, 50, 300, 300]
        want = _bank_windows(b, b._tables(), f, s, 300, F32, PLANAR | PAD, fir, idx, 2)
        assert (x.cpu().numpy().view(np.uint32).reshape(-1) == want).all()
        # against the host rule over the bank's own unfiltered signal; the filter of one tap is the plain crop
        sig, _ = b.crops([0], [0], b.samples[0])
        y, _ = flacgpu.fir_f32_host(sig[0, 1].cpu().numpy(), h, d, 0, 300)
        assert (x[0, 1].cpu().numpy().view(np.uint32) == y.view(np.uint32)).all()
        plain, _ = b.crops(f, s, 300)
        assert torch.equal(x[2], plain[2]) and torch.equal(x[4], plain[4]) and not torch.equal(x[0], plain[0])
        # interleaved, narrowed, not padded, into out=
        out = torch.full((5, 300, 2), 7.0, dtype=torch.float16, device=b.device)
        y16, n2, st = b.crops(f, s, 300, dtype=torch.float16, planar=False, pad=False, out=out, strict=False, fir=fir, fir_index=idx)
        assert y16 is out and n2 == n and st == [0] * 5 and (out[2, 50:] == 0).all()
        assert torch.equal(out, x.transpose(1, 2).to(torch.float16))
        for kw, why in ((dict(dtype=torch.int32), "int32 crops through a filter"), (dict(fir_index=[0, 1]), "one filter index a crop"),
                        (dict(fir_index=[0, 1, 2, 3, 0]), "filter index 3"), (dict(fir_index=None), "one filter index a crop")):
            with pytest.raises(ValueError, match=why):
                b.crops(f, s, 300, **dict(dict(fir=fir, fir_index=idx), **kw))
        with pytest.raises(ValueError, match="fir_index without fir"):
            b.crops(f, s, 300, fir_index=idx)


def test_flacmixbank_crops_with_a_filter_and_a_rate(sources):
    import flacbank

    torch, _ = tgd._torch()
    names = ["a16", "t24", "m8", "b16"]
    with flacbank.FlacMixBank([sources[n][0] for n in names], channels=1, device=0, max_frames=4, sample_rate=48000,
                              channel_map={3: [[0.25, 0.5, 0.25]]}) as b:
        fir = flacbank.FirBank([fref.taps(64, 9), fref.taps(EDGE + 1, 10)], delays=[32, 0])
        f, s, idx = [1, 0, 2, 3, 0, 1], [0, 700, b.out_samples[2] - 80, 50, 4000, 2000], [0, 1, 0, 1, 0, 1]
        x, n = b.crops(f, s, 400, fir=fir, fir_index=idx)
        assert tuple(x.shape) == (6, 1, 400) and n == [400, 400, 80, 400, 400, 400]
        got = x.cpu().numpy().view(np.uint32)
        for w in range(6):  # the C call over the file's own group: masks or weights, and its rate
            g, j = b._where[f[w]]
            bank, mix = b._groups[g]
            weighted = flacbank._is_weights(mix)
            src = b.sample_rates[f[w]]
            want = _bank_windows(bank, bank._tables(), [j], [s[w]], 400, F32, PLANAR | PAD, fir, [idx[w]], 1,
                                 channel_masks=None if weighted else mix, channel_weights=mix if weighted else None,
                                 src_rate=src, dst_rate=48000)
            assert (got[w].reshape(-1) == want).all(), w
        two = flacbank.FirBank([fref.taps(64, 9), np.stack([fref.taps(5, 1), fref.taps(5, 2)])])
        with pytest.raises(ValueError, match="filter 1 has 2 rows, the crops 1 channels"):  # the call refuses such a table
            b.crops(f, s, 400, fir=two, fir_index=[0] * 6)
