"""flacgpu_decode_windows_device_mix and FlacMixBank: the argument checks that need no device, and
their place in the binding.  (The validity rule of a mix over a context's channel count is
fg_deliver.hpp's mix_valid: tests/test_mix_host.py runs it on the host, tests/test_gpu_mix.py
through a context.)"""
import ctypes
import os

import pytest

import flacgpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _arrays():
    u64 = (ctypes.c_uint64 * 2)(0, 8)
    u32 = (ctypes.c_uint32 * 2)(0, 1)
    return ctypes.create_string_buffer(64), u64, u32


def _masks(*m):
    return (ctypes.c_uint8 * 8)(*m)


def test_decode_windows_mix_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, u32 = _arrays()
    f = L.flacgpu_decode_windows_device_mix
    ok = (flacgpu.SAMPLE_F32, flacgpu.DELIVER_PLANAR | flacgpu.DELIVER_PAD)
    head = (buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64)
    tail = (buf, u64, u64, buf, None)
    assert f(None, *head, *ok, 2, _masks(1, 2), *tail) == -2  # no context
    assert f(None, *head, *ok, 2, None, *tail) == -2           # no masks
    assert f(None, *head, *ok, 0, _masks(1, 2), *tail) == -2   # no output channel
    assert f(None, *head, *ok, 9, _masks(1, 2), *tail) == -2   # more than eight
    assert f(None, *head, *ok, 1, _masks(7), *tail) == -2      # a mean of three
    assert f(None, *head, flacgpu.SAMPLE_I32, 0, 1, _masks(3), *tail) == -2  # a mean as integers
    assert f(None, *head, 4, 0, 2, _masks(1, 2), *tail) == -2  # bad format
    assert f(None, *head, 1, 4, 2, _masks(1, 2), *tail) == -2  # bad flags
    assert f(None, None, 2, None, None, None, None, None, None, 2, None, None, None, *ok, 2, None, None, None, None, None,
             None) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, *ok, 2, _masks(1, 2), *tail) == -2


def test_binding():
    assert "flacgpu_decode_windows_device_mix" in flacgpu.exported_symbols()
    assert hasattr(flacgpu.load_library(), "flacgpu_decode_windows_device_mix")
    assert hasattr(flacgpu.Decoder, "decode_windows_device_mix")
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    assert "uint32_t out_channels, const uint8_t *channel_masks" in text


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


@pytest.fixture(scope="module")
def sources():
    s = {"stereo16": _golden("c1_44k16_stereo_file.flac"), "mono16": _file(1, 16, "mono_44k16.flac"),
         "stereo24": _file(2, 24, "c3_96k24_stereo.flac", 96000), "eight24": _file(8, 24, "c4_96k24_8ch.flac", 96000),
         "three8": _file(3, 8, "3ch_8bit.flac", 22050)}
    got = {k: (flacgpu.flac_index(v)[0].channels, flacgpu.flac_index(v)[0].bit_depth) for k, v in s.items()}
    assert got == {"stereo16": (2, 16), "mono16": (1, 16), "stereo24": (2, 24), "eight24": (8, 24), "three8": (3, 8)}
    return s


def test_flacmixbank_is_importable_without_a_device():
    import flacbank

    for name in ("crops", "close", "__enter__", "__exit__", "__len__"):
        assert hasattr(flacbank.FlacMixBank, name)
    assert hasattr(flacbank.FlacBank, "crops")


def test_flacmixbank_policy_errors_name_the_callers_file(no_device, sources):
    import flacbank

    s = sources
    # three channels have no default mix to one, nor to two; file 2 is the first such file
    with pytest.raises(ValueError, match=r"file 2 has 3 channels.*channel_map\[3\]"):
        flacbank.FlacMixBank([s["stereo16"], s["mono16"], s["three8"], s["three8"]], channels=1)
    with pytest.raises(ValueError, match="file 1 has 3 channels"):
        flacbank.FlacMixBank([s["stereo16"], s["three8"]], channels=2)
    # stereo to three, eight to two: no default either
    with pytest.raises(ValueError, match="file 0 has 2 channels"):
        flacbank.FlacMixBank([s["stereo16"]], channels=3)
    with pytest.raises(ValueError, match="file 3 has 8 channels"):
        flacbank.FlacMixBank([s["stereo16"], s["mono16"], s["stereo24"], s["eight24"]], channels=2)
    with pytest.raises(ValueError, match="file 1 is not a FLAC file"):
        flacbank.FlacMixBank([s["stereo16"], b"fLaX" + bytes(60)], channels=1)
    with pytest.raises(ValueError, match="no files"):
        flacbank.FlacMixBank([], channels=1)
    for k in (0, 9):
        with pytest.raises(ValueError, match="channels"):
            flacbank.FlacMixBank([s["stereo16"]], channels=k)


def test_flacmixbank_map_errors_name_the_callers_file(no_device, sources):
    import flacbank

    s = sources
    files = [s["mono16"], s["stereo16"], s["three8"]]
    for bad, why in (([7], "mean of 3"), ([8], "at or above 3"), ([1, 2], "2 masks, not 1"), ([256], "0..255"), ([-1], "0..255")):
        with pytest.raises(ValueError, match=rf"channel_map\[3\], which file 2 needs.*{why}"):
            flacbank.FlacMixBank(files, channels=1, channel_map={3: bad})
    # a map for the stereo file too: it is checked although a default exists
    with pytest.raises(ValueError, match=r"channel_map\[2\], which file 1 needs.*at or above 2"):
        flacbank.FlacMixBank(files, channels=1, channel_map={3: [3], 2: [4]})


def test_flacmixbank_block_rule_names_the_callers_file(no_device, sources):
    import flacbank

    most = flacgpu.decoder_max_block(16)
    big = flacgpu.header_bytes(flacgpu.StreamInfo.new(44100, 2, 16, 0, most + 1), True) + _golden("c1_44k16_stereo.flac")
    assert flacgpu.flac_index(big)[0].max_block_size == most + 1
    with pytest.raises(ValueError, match=rf"file 2 states blocks of {most + 1} samples"):
        flacbank.FlacMixBank([sources["mono16"], sources["stereo24"], big], channels=1)


def test_flacmixbank_valid_banks_get_as_far_as_the_device(monkeypatch, sources):
    """The same files with a good policy or map pass every host check: the first thing that fails
    is the context."""
    import flacbank

    class Opened(Exception):
        pass

    def refuse(*a, **k):
        raise Opened()

    monkeypatch.setattr(flacgpu, "Decoder", refuse)
    s = sources
    with pytest.raises(Opened):
        flacbank.FlacMixBank([s["stereo16"], s["mono16"], s["stereo24"], s["eight24"]], channels=1)
    with pytest.raises(Opened):
        flacbank.FlacMixBank([s["stereo16"], s["mono16"], s["three8"]], channels=2, channel_map={3: [3, 4]})
