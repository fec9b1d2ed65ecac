"""The filtered delivery without a device: flacgpu_fir_f32_host through ctypes against
tests/fir_ref.py, the refusals of flacgpu_decode_windows_device_fir that come before any device work
(each of them alone is exercised on the header's own predicate in tests/test_fir_host.py), its place
in the binding, and the ValueErrors of flacbank.FirBank and flacbank.fir_windowed_sinc."""
import ctypes
import os

import numpy as np
import pytest

import fir_ref as ref
import flacgpu
from test_mix_args import _arrays, _masks

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("T", [1, 2, 16, 17, 257, 4096])
def test_host_statement_against_float64(T):
    total = 3000
    x, h = ref.signal(total, 11 + T), ref.taps(T, T)
    for d in sorted({0, (T - 1) // 2, T - 1}):
        for start, count in ((0, 200), (total - 50, 120), (total, 10), (total + 9000, 10), (1500, 300), (5, 0)):
            y, n = flacgpu.fir_f32_host(x, h, d, start, count)
            y64, mag, want_n = ref.window64(x, h, d, start, count)
            assert n == want_n and y.shape == (count,) and y.dtype == np.float32
            assert (np.abs(y[:n].astype(np.float64) - y64) <= ref.gamma(T) * mag).all(), (T, d, start)
            assert (y[n:].view(np.uint32) == 0).all()


def test_host_statement_identity_and_argument_checks():
    x = ref.signal(400, 5, bits=24)
    y, n = flacgpu.fir_f32_host(x, [1.0], 0, 100, 500)
    assert n == 300 and (y[:300].view(np.uint32) == x[100:].view(np.uint32)).all() and (y[300:].view(np.uint32) == 0).all()
    L = flacgpu.load_library()
    f, got = L.flacgpu_fir_f32_host, ctypes.c_uint64(7)
    xs, h, out = (ctypes.c_float * 8)(*range(8)), (ctypes.c_float * 3)(0.5, 0.25, -1.0), (ctypes.c_float * 8)()
    assert f(xs, 8, h, 3, 1, 2, 8, out, ctypes.byref(got)) == 0 and got.value == 6
    assert list(out)[:6] == [0.5 * 3 + 0.25 * 2 - 1, 0.5 * 4 + 0.25 * 3 - 2, 0.5 * 5 + 0.25 * 4 - 3, 0.5 * 6 + 0.25 * 5 - 4,
                             0.5 * 7 + 0.25 * 6 - 5, 0.25 * 7 - 6] and list(out)[6:] == [0.0, 0.0]
    assert f(xs, 8, h, 3, 1, 2, 8, out, None) == -2            # nowhere to put n
    assert f(None, 8, h, 3, 1, 2, 8, out, ctypes.byref(got)) == -2
    assert f(xs, 8, None, 3, 1, 2, 8, out, ctypes.byref(got)) == -2
    assert f(xs, 8, h, 0, 0, 2, 8, out, ctypes.byref(got)) == -2   # no taps
    assert f(xs, 8, h, 4097, 0, 2, 8, out, ctypes.byref(got)) == -2
    assert f(xs, 8, h, 3, 3, 2, 8, out, ctypes.byref(got)) == -2   # delay >= taps
    assert f(xs, 8, h, 3, 1, 2, 8, None, ctypes.byref(got)) == -2
    assert f(xs, 8, h, 3, 1, 2, (1 << 31) - 2, out, ctypes.byref(got)) == -2  # count + taps - 1 reaches 2^31
    assert f(xs, (1 << 40) + 1, h, 3, 1, 2, 8, out, ctypes.byref(got)) == -2
    assert f(None, 0, h, 3, 1, 2, 0, None, ctypes.byref(got)) == 0 and got.value == 0  # nothing to do
    for bad in (float("nan"), float("inf"), -float("inf")):
        hb = (ctypes.c_float * 3)(0.5, bad, -1.0)
        assert f(xs, 8, hb, 3, 1, 2, 8, out, ctypes.byref(got)) == -2
    with pytest.raises(ValueError, match="finite taps"):
        flacgpu.fir_f32_host(x, [1.0, float("nan")], 0, 0, 4)
    with pytest.raises(ValueError, match="span reaches"):
        flacgpu.fir_f32_host(x, [1.0, 2.0], 0, 0, (1 << 31) - 1)


def _how(**kw):
    h = flacgpu.WindowDelivery(ctypes.sizeof(flacgpu.WindowDelivery), flacgpu.SAMPLE_F32, 0, 0, None, None, 0, 0, None, None)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_decode_windows_fir_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, u32 = _arrays()
    f = L.flacgpu_decode_windows_device_fir
    head = (buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64)
    tail = (buf, u64, u64, buf, None)
    fil = (flacgpu.Fir * 2)(flacgpu.Fir(0, 16, 0, 1, 0), flacgpu.Fir(16, 4, 3, 2, 0))
    wf = (ctypes.c_uint32 * 2)(0, 1)
    taps = ctypes.create_string_buffer(4 * 24)
    good = (taps, 24, 2, fil, wf)
    pm = ctypes.cast(_masks(1, 2), ctypes.c_void_p)
    ft = flacgpu.Features(400, 160, 0)

    def call(how, fir=good, ctx=None, h=head):
        return f(ctx, *h, ctypes.byref(how) if how is not None else None, *fir, *tail)

    # no context can be opened without a device: every refusal below returns before one is needed
    assert call(_how()) == -2
    assert call(None) == -2
    assert call(_how(size=48)) == -2
    assert call(_how(features=ctypes.cast(ctypes.pointer(ft), ctypes.c_void_p))) == -2
    assert call(_how(sample_format=flacgpu.SAMPLE_I32)) == -2 and call(_how(sample_format=4)) == -2
    assert call(_how(flags=4)) == -2
    assert call(_how(channel_masks=pm, channel_weights=pm, out_channels=2)) == -2
    assert call(_how(src_rate=44100)) == -2 and call(_how(src_rate=48000, dst_rate=48000)) == -2
    assert call(_how(), fir=(None, 24, 2, fil, wf)) == -2                          # no taps
    assert call(_how(), fir=(ctypes.c_void_p(ctypes.addressof(taps) + 2), 23, 2, fil, wf)) == -2  # misaligned
    assert call(_how(), fir=(taps, 24, 2, None, wf)) == -2 and call(_how(), fir=(taps, 24, 2, fil, None)) == -2
    assert call(_how(), fir=(taps, 23, 2, fil, wf)) == -2                          # offset + rows * taps > taps_len
    assert call(_how(), fir=(taps, 24, 1, fil, wf)) == -2                          # window_filter[1] >= n_filters
    for bad in (flacgpu.Fir(0, 0, 0, 1, 0), flacgpu.Fir(0, 4097, 0, 1, 0), flacgpu.Fir(0, 4, 4, 1, 0), flacgpu.Fir(0, 4, 0, 3, 0),
                flacgpu.Fir(0, 4, 0, 1, 1), flacgpu.Fir(21, 4, 0, 1, 0)):
        assert call(_how(), fir=(taps, 24, 2, (flacgpu.Fir * 2)(fil[0], bad), wf)) == -2
    big = (ctypes.c_uint64 * 2)(8, (1 << 31) - 4)
    assert call(_how(), h=(buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, big)) == -2  # count + taps - 1 >= 2^31
    assert call(_how(), h=(buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64)) == -2
    assert ctypes.sizeof(flacgpu.Fir) == 24 and ctypes.sizeof(flacgpu.WindowDelivery) == 56


def test_binding():
    names = ("flacgpu_decode_windows_device_fir", "flacgpu_fir_f32_host")
    assert set(names) <= set(flacgpu.exported_symbols())
    for name in names:
        assert hasattr(flacgpu.load_library(), name)
    assert hasattr(flacgpu.Decoder, "decode_windows_device_fir")
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    assert "typedef struct { uint64_t offset; uint32_t taps, delay, rows, reserved; } flacgpu_fir;" in text
    assert "int flacgpu_fir_f32_host(const float *x, uint64_t total, const float *taps, uint32_t n_taps, uint32_t delay," in text


# ---- flacbank ---------------------------------------------------------------------------------------
def test_firbank_refusals_come_before_the_device(monkeypatch):
    import flacbank
    import torch

    def refuse(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(torch, "from_numpy", refuse)
    for filters, delays, why in (([], None, "no filters"), ([[1.0, float("nan")]], None, "filter 0 has a tap that is not finite"),
                                 ([[1.0], [float("inf")]], None, "filter 1 has a tap"), ([np.zeros(4097)], None, "4097 taps"),
                                 ([np.zeros(0)], None, "0 taps"), ([np.zeros((9, 4))], None, "1 to 8 rows"),
                                 ([np.zeros((1, 2, 3))], None, r"not \[T\] or \[K, T\]"), ([[1.0, 2.0]], [2], "delay 2, not 0 to 1"),
                                 ([[1.0, 2.0]], [-1], "delay -1"), ([[1.0]], [0, 0], "2 delays for 1 filters")):
        with pytest.raises(ValueError, match=f"FirBank: .*{why}"):
            flacbank.FirBank(filters, delays)
    with pytest.raises(AssertionError, match="the device was touched"):  # a valid bank gets as far as the device
        flacbank.FirBank([[1.0], np.ones((2, 5))], [0, 2])


def test_windowed_sinc():
    import flacbank

    h, d = flacbank.fir_windowed_sinc(16000, 300, 3400, 255)
    assert h.dtype == np.float32 and h.shape == (255,) and d == 127 and (h == h[::-1]).all()
    H = np.abs(np.fft.rfft(h.astype(np.float64), 16000))  # 1 Hz a bin
    assert abs(H[1000] - 1) < 1e-3 and abs(H[2500] - 1) < 1e-3 and H[0] < 1e-3 and H[100] < 1e-2 and H[3800:].max() < 1e-2
    m = np.arange(255) - 127.0
    want = ((2 * 3400 / 16000) * np.sinc(2 * 3400 / 16000 * m) - (2 * 300 / 16000) * np.sinc(2 * 300 / 16000 * m)) * np.kaiser(255, 9.0)
    assert (h.view(np.uint32) == want.astype(np.float32).view(np.uint32)).all()  # float64, rounded once
    lo, d = flacbank.fir_windowed_sinc(48000, 0, 4000, 64)  # a low-pass, even length
    assert d == 31 and abs(float(lo.astype(np.float64).sum()) - 1) < 1e-3
    hp, d = flacbank.fir_windowed_sinc(16000, 100, None, 1001)  # a high-pass
    Hh = np.abs(np.fft.rfft(hp.astype(np.float64), 16000))
    assert d == 500 and Hh[0] < 1e-3 and abs(Hh[8000] - 1) < 1e-3 and abs(Hh[1000] - 1) < 1e-3
    one, d = flacbank.fir_windowed_sinc(8000, 0, 4000, 1)
    assert d == 0 and one.tolist() == [1.0]
    for args, why in (((16000, 100, None, 100), "odd number of taps"), ((16000, 0, None, 101), "f_lo > 0"),
                      ((16000, 3400, 300, 101), "f_lo < f_hi"), ((16000, 300, 8001, 101), "f_lo < f_hi"),
                      ((16000, -1, 300, 101), "f_lo < f_hi"), ((16000, 300, 3400, 0), "1 to 4096 taps"),
                      ((16000, 300, 3400, 4097), "1 to 4096 taps"), ((0, 300, 3400, 11), "sample rate")):
        with pytest.raises(ValueError, match=f"fir_windowed_sinc: .*{why}"):
            flacbank.fir_windowed_sinc(*args)


def test_crops_take_the_keywords():
    import inspect

    import flacbank

    for cls in (flacbank.FlacBank, flacbank.FlacMixBank):
        p = inspect.signature(cls.crops).parameters
        assert p["fir"].default is None and p["fir_index"].default is None
