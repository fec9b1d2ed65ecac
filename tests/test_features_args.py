"""flacgpu_decode_windows_device_features, the Python checks in front of it, the `features` methods
of the banks and flacbank.mel_filters: everything that needs no device.  (The rule itself:
tests/test_features_host.py on the host, tests/test_gpu_features.py through a context.)"""
import ctypes
import inspect
import os

import numpy as np
import pytest

import flacgpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _arrays():
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    u32 = (ctypes.c_uint32 * 2)(0, 1)
    return ctypes.create_string_buffer(64), u64, u32


def _masks(*m):
    return (ctypes.c_uint8 * 8)(*m)


def _ft(N=64, H=16, R=0):
    return ctypes.byref(flacgpu.Features(N, H, R))


def test_features_call_argument_checks_without_a_device():
    f = flacgpu.load_library().flacgpu_decode_windows_device_features
    buf, u64, u32 = _arrays()
    head = (buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64)
    F = (ctypes.c_float * (2 * 33))(*([0.5] * 66))
    tail = (buf, u64, u64, buf, None)
    F32 = flacgpu.SAMPLE_F32
    # no context: refused whatever else is right or wrong
    assert f(None, *head, F32, 2, _masks(1, 2), 0, 0, _ft(), None, *tail) == -2
    assert f(None, *head, F32, 0, None, 44100, 16000, _ft(64, 16, 2), F, *tail) == -2
    assert f(None, *head, F32, 2, _masks(1, 2), 0, 0, None, None, *tail) == -2            # no parameters
    for N, H, R in ((14, 4, 0), (2050, 4, 0), (65, 4, 0), (64, 0, 0), (64, 65, 0), (64, 16, 257)):
        assert f(None, *head, F32, 2, _masks(1, 2), 0, 0, _ft(N, H, R), F, *tail) == -2, (N, H, R)
    assert f(None, *head, F32, 2, _masks(1, 2), 0, 0, _ft(64, 16, 2), None, *tail) == -2  # rows without a matrix
    assert f(None, *head, flacgpu.SAMPLE_I32, 2, _masks(1, 2), 0, 0, _ft(), None, *tail) == -2
    assert f(None, *head, 4, 2, _masks(1, 2), 0, 0, _ft(), None, *tail) == -2             # unknown format
    assert f(None, *head, F32, 2, _masks(1, 2), 44100, 44100, _ft(), None, *tail) == -2   # equal rates that are not 0
    assert f(None, *head, F32, 2, _masks(1, 2), 192000, 8000, _ft(), None, *tail) == -2   # 24 to 1 down
    assert f(None, *head, F32, 2, _masks(1, 2), 0, 16000, _ft(), None, *tail) == -2
    assert f(None, *head, F32, 9, _masks(1, 2), 0, 0, _ft(), None, *tail) == -2
    assert f(None, *head, F32, 1, _masks(7), 0, 0, _ft(), None, *tail) == -2              # a mean of three
    assert f(None, None, 2, None, None, None, None, None, None, 2, None, None, None, F32, 2, None, 0, 0, _ft(), None, None, None,
             None, None, None) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, F32, 2, _masks(1, 2), 0, 0, _ft(), None, *tail) == -2


def test_python_checks_come_before_the_library():
    d = flacgpu.Decoder.__new__(flacgpu.Decoder)  # no context: a call that got to the library would fail otherwise
    ok = dict(sample_format=flacgpu.SAMPLE_F32, channel_masks=None, src_rate=0, dst_rate=0, n_fft=64, hop=16, filters=None)
    inf = np.ones((2, 33), np.float32)
    inf[1, 5] = np.inf
    bad = [dict(n_fft=14), dict(n_fft=65), dict(n_fft=4096), dict(hop=0), dict(hop=65), dict(filters=np.ones((2, 32), np.float32)),
           dict(filters=np.ones((257, 33), np.float32)), dict(filters=np.ones(33, np.float32)), dict(filters=inf),
           dict(filters=np.full((1, 33), np.nan, np.float32)), dict(sample_format=flacgpu.SAMPLE_I32), dict(sample_format=7),
           dict(channel_masks=[256]), dict(channel_masks=[]), dict(channel_masks=[1] * 9), dict(src_rate=44100, dst_rate=44100),
           dict(src_rate=192000, dst_rate=8000), dict(src_rate=0, dst_rate=16000)]
    for change in bad:
        kw = dict(ok, **change)
        with pytest.raises(ValueError):
            d.decode_windows_device_features(0, [0], 0, 0, 0, 0, 0, [(0, 0, 1)], kw["sample_format"], kw["channel_masks"],
                                             kw["src_rate"], kw["dst_rate"], kw["n_fft"], kw["hop"], kw["filters"], 0, [0], [33], 0)
    for windows in ([(0, -1, 1)], [(0, 0, -1)], [(0, 0, (1 << 31) // 16)]):  # the last: (frames - 1) * 16 + 64 >= 2^31
        with pytest.raises(ValueError):
            d.decode_windows_device_features(0, [0], 0, 0, 0, 0, 0, windows, flacgpu.SAMPLE_F32, None, 0, 0, 64, 16, None, 0, [0],
                                             [33], 0)
    with pytest.raises(ValueError):
        flacgpu.features_f32_host(np.zeros((4, 2), np.float32), 64, 16, 0, 1)
    with pytest.raises(ValueError):
        flacgpu.features_table(18 + 1)
    ft, f, rows = flacgpu.features_params(400, 160, np.ones((80, 201)))
    assert (ft.n_fft, ft.hop, ft.n_rows, rows) == (400, 160, 80, 80) and f.dtype == np.float32 and f.flags["C_CONTIGUOUS"]
    assert flacgpu.features_params(400, 160)[1:] == (None, 201)


def test_binding():
    names = ("flacgpu_decode_windows_device_features", "flacgpu_features_table", "flacgpu_features_f32_host")
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    for name in names:
        assert name in flacgpu.exported_symbols() and hasattr(flacgpu.load_library(), name) and f"int {name}(" in text
    assert hasattr(flacgpu.Decoder, "decode_windows_device_features")
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5
    assert "typedef struct { uint32_t n_fft, hop, n_rows; } flacgpu_features;" in text and ctypes.sizeof(flacgpu.Features) == 12


def test_bank_surface():
    import flacbank

    for cls in (flacbank.FlacBank, flacbank.FlacMixBank):
        p = inspect.signature(cls.features).parameters
        assert list(p)[:6] == ["self", "file", "start", "frames", "n_fft", "hop"]
        assert p["filters"].default is None and p["log"].default is None and p["floor"].default == 1e-10
        assert p["strict"].default is True and p["out"].default is None and p["dtype"].default is None
    assert "rate" in inspect.signature(flacbank.FlacBank.features).parameters
    assert "rate" not in inspect.signature(flacbank.FlacMixBank.features).parameters
    assert "feat" in inspect.signature(flacbank._crops).parameters  # the one body is shared


# ---- mel_filters -------------------------------------------------------------------------------------
def _htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def _slaney(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-9) / 1000.0) / np.log(6.4))


@pytest.mark.parametrize("rate,n_fft,n_mels,fmin,fmax,scale,norm", [
    (16000, 400, 80, 0.0, None, "slaney", "slaney"), (16000, 400, 128, 0.0, None, "htk", None),
    (44100, 2048, 128, 20.0, 16000.0, "slaney", "slaney"), (22050, 1024, 40, 0.0, 8000.0, "htk", "slaney"),
    (48000, 512, 23, 100.0, None, "slaney", None)])
def test_mel_filters(rate, n_fft, n_mels, fmin, fmax, scale, norm):
    import flacbank

    F = flacbank.mel_filters(rate, n_fft, n_mels, fmin=fmin, fmax=fmax, scale=scale, norm=norm)
    B = n_fft // 2 + 1
    assert F.shape == (n_mels, B) and F.dtype == np.float32 and F.flags["C_CONTIGUOUS"] and np.isfinite(F).all()
    assert (F >= 0).all()
    mel = _htk if scale == "htk" else _slaney
    top = rate / 2.0 if fmax is None else fmax
    m = np.linspace(mel(fmin), mel(top), n_mels + 2)
    g = np.arange(B) * rate / n_fft
    gm = mel(g)
    for r in range(n_mels):
        row = F[r].astype(np.float64)
        nz = np.nonzero(row)[0]
        # support inside (m_r, m_{r+2}) on the mel axis
        assert ((gm[nz] > m[r] - 1e-9) & (gm[nz] < m[r + 2] + 1e-9)).all()
        if len(nz) == 0:  # a band narrower than a bin, between two bins
            assert not ((gm > m[r] + 1e-9) & (gm < m[r + 2] - 1e-9)).any()
            continue
        # single-peaked: it rises up to the peak, then falls
        k = int(np.argmax(row))
        assert (np.diff(row[nz[0]:k + 1]) >= 0).all() and (np.diff(row[k:nz[-1] + 1]) <= 0).all()
        # the peak is the bin next to the stated centre (the nearest one on its side of the triangle)
        centre = m[r + 1]
        near = np.argsort(np.abs(gm - centre))[:2]
        assert k in near or abs(gm[k] - centre) <= np.abs(gm[near[1]] - centre) + 1e-9
    # the mel scale itself
    if scale == "htk":
        assert np.allclose(flacbank._hz_to_mel([0.0, 700.0, 1000.0, 8000.0], "htk"), _htk([0.0, 700.0, 1000.0, 8000.0]), rtol=1e-12)
        assert abs(float(flacbank._hz_to_mel(700.0, "htk")) - 2595.0 * np.log10(2.0)) < 1e-9
    else:
        assert np.allclose(flacbank._hz_to_mel([0.0, 200.0, 1000.0, 6400.0], "slaney"), [0.0, 3.0, 15.0, 42.0], rtol=1e-12)
    f = np.array([0.0, 55.0, 999.0, 1000.0, 1001.0, 7999.0])
    assert np.allclose(flacbank._mel_to_hz(flacbank._hz_to_mel(f, scale), scale), f, rtol=1e-10, atol=1e-9)
    # the area rule: with the triangle's exact edges, row r * (f_{r+2} - f_r) / 2 has a peak value of at most 1
    edges = flacbank._mel_to_hz(m, scale)
    width = (edges[2:] - edges[:-2]) / 2.0
    if norm == "slaney":
        unit = F.astype(np.float64) * width[:, None]
        plain = flacbank.mel_filters(rate, n_fft, n_mels, fmin=fmin, fmax=fmax, scale=scale, norm=None).astype(np.float64)
        assert np.allclose(unit, plain, rtol=1e-6, atol=1e-7) and plain.max() <= 1.0 + 1e-7
        # where the bins sample a triangle densely its discrete area is 1
        wide = [r for r in range(n_mels) if np.count_nonzero(F[r]) >= 12]
        assert wide or n_fft < 1024
        for r in wide:
            assert abs(F[r].astype(np.float64).sum() * rate / n_fft - 1.0) < 0.02
    else:
        assert F.max() <= 1.0 + 1e-7


def test_mel_filters_refusals():
    import flacbank

    for kw in (dict(scale="mel"), dict(norm="l1"), dict(fmin=-1.0), dict(fmax=9000.0), dict(fmin=4000.0, fmax=4000.0)):
        with pytest.raises(ValueError):
            flacbank.mel_filters(16000, 400, 80, **kw)
    for args in ((0, 400, 80), (16000, 401, 80), (16000, 400, 0), (16000, 400, 257), (16000, 4096, 80)):
        with pytest.raises(ValueError):
            flacbank.mel_filters(*args)
