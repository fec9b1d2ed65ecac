"""flacgpu_decode_windows_device_resample, the two host-only resample functions, and the rate
keywords of FlacBank and FlacMixBank: the argument checks that need no device, the shapes of the
coefficient tables, and their place in the binding.  (The rule itself: tests/test_resample_host.py on
the host, tests/test_gpu_resample.py through a context.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

import flacgpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as ref  # noqa: E402


def _arrays():
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    u32 = (ctypes.c_uint32 * 2)(0, 1)
    return ctypes.create_string_buffer(64), u64, u32


def _masks(*m):
    return (ctypes.c_uint8 * 8)(*m)


def test_decode_windows_resample_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, u32 = _arrays()
    f = L.flacgpu_decode_windows_device_resample
    ok = (flacgpu.SAMPLE_F32, flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD)
    head = (buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64)
    rates = (44100, 48000)
    tail = (buf, u64, u64, buf, None)
    assert f(None, *head, *ok, 2, _masks(1, 2), *rates, *tail) == -2  # no context
    assert f(None, *head, *ok, 2, None, *rates, *tail) == -2           # no context, the identity
    assert f(None, *head, *ok, 0, _masks(1, 2), *rates, *tail) == -2   # no output channel
    assert f(None, *head, *ok, 9, _masks(1, 2), *rates, *tail) == -2   # more than eight
    assert f(None, *head, *ok, 1, _masks(7), *rates, *tail) == -2      # a mean of three
    assert f(None, *head, flacgpu.SAMPLE_I32, 0, 2, _masks(1, 2), *rates, *tail) == -2  # integers are not offered
    assert f(None, *head, 4, 0, 2, _masks(1, 2), *rates, *tail) == -2  # bad format
    assert f(None, *head, 1, 4, 2, _masks(1, 2), *rates, *tail) == -2  # bad flags
    assert f(None, *head, *ok, 2, _masks(1, 2), 44100, 44100, *tail) == -2   # equal rates
    assert f(None, *head, *ok, 2, _masks(1, 2), 192000, 8000, *tail) == -2   # 24 to 1 down
    assert f(None, *head, *ok, 2, _masks(1, 2), 44100, 44101, *tail) == -2   # L = 44101
    assert f(None, *head, *ok, 2, _masks(1, 2), 0, 48000, *tail) == -2
    assert f(None, None, 2, None, None, None, None, None, None, 2, None, None, None, *ok, 2, None, *rates, None, None, None,
             None, None) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, *ok, 2, _masks(1, 2), *rates, *tail) == -2


def test_resample_filter_refusals_and_sizes():
    L = flacgpu.load_library()
    up, down, taps, n = ctypes.c_uint32(9), ctypes.c_uint32(9), ctypes.c_uint32(9), ctypes.c_size_t(9)
    f = L.flacgpu_resample_filter
    for src, dst in ((44100, 44100), (192000, 8000), (44100, 44101), (0, 48000), (48000, 0), (8000 * 1025, 8000)):
        assert f(src, dst, ctypes.byref(up), ctypes.byref(down), ctypes.byref(taps), None, 0, ctypes.byref(n)) == -2, (src, dst)
    assert f(44100, 48000, None, None, None, None, 0, None) == -2                  # nowhere to put the size
    assert f(44100, 48000, None, None, None, None, 10, ctypes.byref(n)) == -2      # a capacity without a buffer
    assert f(44100, 48000, ctypes.byref(up), ctypes.byref(down), ctypes.byref(taps), None, 0, ctypes.byref(n)) == -4
    assert (up.value, down.value, taps.value, n.value) == (160, 147, 48, 160 * 48)
    small = (ctypes.c_float * (160 * 48 - 1))()
    assert f(44100, 48000, None, None, None, small, len(small), ctypes.byref(n)) == -4 and n.value == 160 * 48
    assert all(v == 0.0 for v in small)  # nothing written
    with pytest.raises(flacgpu.FlacGpuError):
        flacgpu.resample_filter(44100, 44100)
    assert flacgpu.resample_ratio(44100, 44100) is None and flacgpu.resample_ratio(-1, 8000) is None


@pytest.mark.parametrize("src,dst,L,M,T", [(44100, 48000, 160, 147, 48), (48000, 44100, 147, 160, 54), (48000, 16000, 1, 3, 144),
                                           (24000, 48000, 2, 1, 48), (44100, 16000, 160, 441, 134), (96000, 8000, 1, 12, 576)],
                         ids=["160_147", "147_160", "1_3", "2_1", "160_441", "1_12"])
def test_resample_filter_shapes(src, dst, L, M, T):
    assert ref.ratio(src, dst) == (L, M, T // 2, T)
    got = flacgpu.resample_filter(src, dst)
    assert got[:3] == (L, M, T) and got[3].shape == (L, T) and got[3].dtype == np.float32
    assert flacgpu.resample_ratio(src, dst) == (L, M, T)
    h = got[3].astype(np.float64)
    assert np.abs(h.sum(axis=1) - 1.0).max() <= T * 2.0 ** -24
    # phase 0 peaks at tap Hw - 1, the sample the output sits on, and is symmetric about it
    assert int(np.argmax(h[0])) == T // 2 - 1 and np.array_equal(got[3][0][:T - 1], got[3][0][:T - 1][::-1])


def test_resample_f32_host_refusals():
    L = flacgpu.load_library()
    x = (ctypes.c_float * 8)(*([0.5] * 8))
    y = (ctypes.c_float * 16)()
    n = ctypes.c_uint64(99)
    f = L.flacgpu_resample_f32_host
    assert f(x, 8, 44100, 44100, 0, 8, y, ctypes.byref(n)) == -2      # equal rates
    assert f(x, 8, 192000, 8000, 0, 8, y, ctypes.byref(n)) == -2      # no such ratio
    assert f(None, 8, 44100, 48000, 0, 8, y, ctypes.byref(n)) == -2   # samples without a buffer
    assert f(x, 8, 44100, 48000, 0, 8, y, None) == -2
    assert f(x, 8, 44100, 48000, 0, 8, None, ctypes.byref(n)) == -2   # outputs without a buffer
    assert f(x, (1 << 40) + 1, 44100, 48000, 0, 8, y, ctypes.byref(n)) == -2
    assert f(x, 8, 44100, 48000, 0, 16, y, ctypes.byref(n)) == 0 and n.value == 9   # ceil(8 * 160 / 147)
    assert f(x, 8, 44100, 48000, 9, 16, None, ctypes.byref(n)) == 0 and n.value == 0  # past the end: nothing to write
    assert f(None, 0, 44100, 48000, 0, 16, None, ctypes.byref(n)) == 0 and n.value == 0
    assert f(x, 8, 44100, 48000, 3, 0, None, ctypes.byref(n)) == 0 and n.value == 0
    with pytest.raises(flacgpu.FlacGpuError):
        flacgpu.resample_f32_host(np.zeros(4, np.float32), 8000, 8000)
    with pytest.raises(ValueError):
        flacgpu.resample_f32_host(np.zeros((4, 2), np.float32), 8000, 16000)
    assert len(flacgpu.resample_f32_host(np.zeros(4, np.float32), 8000, 16000)) == 8


def test_binding():
    names = ("flacgpu_decode_windows_device_resample", "flacgpu_resample_filter", "flacgpu_resample_f32_host")
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    for name in names:
        assert name in flacgpu.exported_symbols() and hasattr(flacgpu.load_library(), name) and f"int {name}(" in text
    assert hasattr(flacgpu.Decoder, "decode_windows_device_resample")
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5
    assert "uint32_t src_rate, uint32_t dst_rate," in text and "NOT a decode path" in text


def test_decoder_method_refuses_bad_masks_and_rates_before_the_library():
    d = flacgpu.Decoder.__new__(flacgpu.Decoder)  # no context: the checks come first
    for masks, src, dst in (([256], 44100, 48000), ([-1], 44100, 48000), ([1], -1, 48000), ([1], 44100, 1 << 32)):
        with pytest.raises(flacgpu.FlacGpuError) as e:
            d.decode_windows_device_resample(0, [0], 0, 0, 0, 0, 0, [(0, 0, 1)], flacgpu.SAMPLE_F32, 0, masks, src, dst, 0, [0], [1], 0)
        assert e.value.code == -2


# ---- the banks ---------------------------------------------------------------------------------------
def _golden(name):
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        return f.read()


def _file(channels, bits, frames, rate=44100, block=4096):
    """Golden bare frames with a STREAMINFO in front: a file."""
    return flacgpu.header_bytes(flacgpu.StreamInfo.new(rate, channels, bits, 0, block), True) + _golden(frames)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(flacgpu, "Decoder", refuse)


def test_flacmixbank_rate_errors_name_the_callers_file(no_device):
    import flacbank

    stereo, mono = _golden("c1_44k16_stereo_file.flac"), _file(1, 16, "mono_44k16.flac")
    hi = _file(2, 24, "c3_96k24_stereo.flac", 96000)
    assert [flacgpu.flac_index(f)[0].sample_rate for f in (stereo, mono, hi)] == [44100, 44100, 96000]
    with pytest.raises(ValueError, match=r"FlacMixBank: file 2 is at 96000 Hz, and 96000 -> 7000 is not a ratio"):
        flacbank.FlacMixBank([stereo, mono, hi], channels=1, sample_rate=7000)  # 44100 -> 7000 is 10/63: served
    with pytest.raises(ValueError, match=r"file 0 is at 44100 Hz, and 44100 -> 44101"):
        flacbank.FlacMixBank([stereo, mono, hi], channels=1, sample_rate=44101)
    with pytest.raises(ValueError, match=r"file 1 is at 44100 Hz, and 44100 -> 96001"):
        flacbank.FlacMixBank([_file(2, 24, "c3_96k24_stereo.flac", 96001), mono], channels=1, sample_rate=96001)  # file 0 is at the rate


def test_flacmixbank_valid_rates_get_as_far_as_the_device(monkeypatch):
    import flacbank

    class Opened(Exception):
        pass

    def refuse(*a, **k):
        raise Opened()

    monkeypatch.setattr(flacgpu, "Decoder", refuse)
    stereo, hi = _golden("c1_44k16_stereo_file.flac"), _file(2, 24, "c3_96k24_stereo.flac", 96000)
    for rate in (48000, 44100, 96000, 16000, None):
        with pytest.raises(Opened):
            flacbank.FlacMixBank([stereo, hi], channels=1, sample_rate=rate)


def test_rate_keywords_exist():
    import inspect

    import flacbank

    assert "rate" in inspect.signature(flacbank.FlacBank.crops).parameters
    assert "sample_rate" in inspect.signature(flacbank.FlacMixBank.__init__).parameters
    assert hasattr(flacbank.FlacBank, "samples_at")
    assert flacbank._out_samples(1000, 44100, 44100) == 1000 and flacbank._out_samples(1000, 44100, 48000) == 1089
    assert flacbank._rate_error("X", 0, 44100, 44100) is None and flacbank._rate_error("X", 0, 44100, 48000) is None
