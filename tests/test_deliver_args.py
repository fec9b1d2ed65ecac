"""flacgpu_decode_windows_device_as and FlacBank: the argument checks that need no device, and
their place in the binding."""
import ctypes
import os

import pytest

import flacgpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _arrays():
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    u32 = (ctypes.c_uint32 * 2)(0, 1)
    return ctypes.create_string_buffer(64), u64, u32


def test_decode_windows_as_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, u32 = _arrays()
    f = L.flacgpu_decode_windows_device_as
    ok = (flacgpu.SAMPLE_F32, flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD)
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, *ok, buf, u64, u64, buf, None) == -2  # no context
    assert f(None, None, 2, None, None, None, None, None, None, 2, None, None, None, *ok, None, None, None, None, None) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, 4, 0, buf, u64, u64, buf, None) == -2  # bad format
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, 0xFFFFFFFF, 0, buf, u64, u64, buf, None) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, 1, 4, buf, u64, u64, buf, None) == -2  # bad flags
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, *ok, buf, u64, u64, buf, None) == -2
    assert f(None, buf, 0, None, None, None, None, None, None, 0, None, None, None, *ok, None, None, None, None, None) == -2


def test_binding():
    assert (flacgpu.SAMPLE_I32, flacgpu.SAMPLE_F32, flacgpu.SAMPLE_F16, flacgpu.SAMPLE_BF16) == (0, 1, 2, 3)
    assert (flacgpu.DELIVER_PLANAR, flacgpu.DELIVER_PAD) == (1, 2)
    assert "flacgpu_decode_windows_device_as" in flacgpu.exported_symbols()
    assert hasattr(flacgpu.load_library(), "flacgpu_decode_windows_device_as")
    assert hasattr(flacgpu.Decoder, "decode_windows_device_as")
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5


def test_header_states_the_formats_and_flags():
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    for decl in ("FLACGPU_SAMPLE_I32 = 0", "FLACGPU_SAMPLE_F32 = 1", "FLACGPU_SAMPLE_F16 = 2", "FLACGPU_SAMPLE_BF16 = 3",
                 "FLACGPU_DELIVER_PLANAR = 1", "FLACGPU_DELIVER_PAD = 2"):
        assert decl in text


def _golden(name):
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        return f.read()


def test_flacbank_is_importable_without_a_device():
    import flacbank

    assert hasattr(flacbank.FlacBank, "crops") and hasattr(flacbank.FlacBank, "close")
    assert hasattr(flacbank.FlacBank, "__enter__") and hasattr(flacbank.FlacBank, "__exit__")


def test_flacbank_refuses_mixed_depths_before_any_device_call(monkeypatch):
    import flacbank

    def no_device(*a, **k):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(flacgpu, "Decoder", no_device)
    # the golden 24-bit stream is bare frames: a STREAMINFO in front makes it a file
    a = _golden("c1_44k16_stereo_file.flac")
    b = flacgpu.header_bytes(flacgpu.StreamInfo.new(96000, 2, 24, 0, 4096), True) + _golden("c3_96k24_stereo.flac")
    assert flacgpu.flac_index(a)[0].bit_depth == 16 and flacgpu.flac_index(b)[0].bit_depth == 24
    with pytest.raises(ValueError, match="file 2"):
        flacbank.FlacBank([a, a, b, a])
    with pytest.raises(ValueError, match="file 1"):
        flacbank.FlacBank([a, b"fLaX" + bytes(60)])
    with pytest.raises(ValueError):
        flacbank.FlacBank([])
