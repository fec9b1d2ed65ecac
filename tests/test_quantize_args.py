"""flacgpu_pcm_from_elements_device / _host and FlacBank.from_tensors: the argument checks that need no
device, and their place in the binding.  (The rule itself: tests/test_quantize_host.py on the host,
tests/test_gpu_bank_write.py on the device.)"""
import ctypes
import os
import re

import numpy as np
import pytest

import flacgpu

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("flacgpu_pcm_from_elements_device", "flacgpu_pcm_from_elements_host")


def test_binding():
    L = flacgpu.load_library()
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        assert name in flacgpu.exported_symbols()
        assert hasattr(L, name) and getattr(L, name).argtypes is not None
        assert re.search(rf"\bint {name}\s*\(", text)
    assert hasattr(flacgpu.Encoder, "pcm_from_elements_device") and hasattr(flacgpu, "pcm_from_elements_host")
    assert L.flacgpu_abi_version() == 5
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added


def test_device_call_refusals_without_a_context():
    f = flacgpu.load_library().flacgpu_pcm_from_elements_device
    buf = ctypes.create_string_buffer(256)
    src = (ctypes.c_void_p * 2)(ctypes.addressof(buf), ctypes.addressof(buf))
    n = (ctypes.c_uint64 * 2)(8, 8)
    off = (ctypes.c_uint64 * 2)(0, 64)
    ok = dict(n_streams=2, d_src=src, samples=n, stride=n, fmt=flacgpu.SAMPLE_F32, flags=flacgpu.DELIVER_PLANAR, pcm=buf, off=off,
              cap=256, clipped=buf)

    def call(ctx=None, **kw):
        a = dict(ok, **kw)
        return f(ctx, a["n_streams"], a["d_src"], a["samples"], a["stride"], a["fmt"], a["flags"], a["pcm"], a["off"], a["cap"],
                 a["clipped"], None)

    assert call() == -2  # no context
    for kw in (dict(d_src=None), dict(samples=None), dict(pcm=None), dict(off=None), dict(clipped=None),
               dict(d_src=(ctypes.c_void_p * 2)(ctypes.addressof(buf), None)),       # a null source
               dict(off=(ctypes.c_uint64 * 2)(0, 66)),                               # an unaligned offset
               dict(cap=64 + 8 * 2 * 2 - 1),                                         # a stream passes the capacity
               dict(off=(ctypes.c_uint64 * 2)(0, 16)),                               # a stream runs into the next
               dict(off=(ctypes.c_uint64 * 2)(64, 0)),                               # offsets that descend
               dict(fmt=4), dict(fmt=0xFFFFFFFF),                                    # a format outside the four
               dict(flags=flacgpu.DELIVER_PAD), dict(flags=4),                       # a flag other than PLANAR
               dict(stride=(ctypes.c_uint64 * 2)(8, 7)),                             # a stride below T
               dict(n_streams=65536)):                                               # too many streams
        assert call(**kw) == -2, kw


def _host(x, samples, stride, channels, bits, fmt, flags, cap=None, out=None, clipped=True):
    L = flacgpu.load_library()
    out = np.zeros(64, dtype=np.uint32) if out is None else out
    c = ctypes.c_uint64(99)
    rc = L.flacgpu_pcm_from_elements_host(x.ctypes.data if x is not None else None, samples, stride, channels, bits, fmt, flags,
                                          out if isinstance(out, int) else out.ctypes.data, 256 if cap is None else cap,
                                          ctypes.byref(c) if clipped else None)
    return rc, out, c.value


def test_host_call_refusals():
    x = np.zeros((2, 8), dtype=np.float32)
    ok = (x, 8, 8, 2, 16, flacgpu.SAMPLE_F32, flacgpu.DELIVER_PLANAR)
    assert _host(*ok)[0] == 0
    assert _host(None, *ok[1:])[0] == -2
    assert _host(*ok, out=0)[0] == -2 and _host(*ok, clipped=False)[0] == -2
    aligned = np.zeros(64, dtype=np.uint32)
    assert _host(*ok, out=aligned.ctypes.data + 2)[0] == -2  # an unaligned destination
    for channels in (0, 9):
        assert _host(x, 8, 8, channels, 16, 1, 1)[0] == -2
    for bits in (0, 12, 20, 33, 64):
        assert _host(x, 8, 8, 2, bits, 1, 1)[0] == -2
    assert _host(x, 8, 8, 2, 16, 4, 1)[0] == -2 and _host(x, 8, 8, 2, 16, 1, 2)[0] == -2 and _host(x, 8, 8, 2, 16, 1, 3)[0] == -2
    assert _host(x, 8, 7, 2, 16, 1, 1)[0] == -2   # a plane stride below the samples
    assert _host(x, 8, 0, 2, 16, 1, 0)[0] == 0    # which an interleaved source does not have
    assert _host(x, 1 << 62, 1 << 62, 2, 16, 1, 1)[0] == -2
    assert _host(*ok, cap=31)[0] == -4 and _host(*ok, cap=32)[0] == 0
    assert _host(x, 3, 8, 1, 8, 1, 1, cap=3)[0] == -4 and _host(x, 3, 8, 1, 8, 1, 1, cap=4)[0] == 0  # the last word is whole


def test_host_call_writes_the_rule():
    x = np.array([[0.5, -1.0, 1.0], [np.nan, 0.25, -0.5]], dtype=np.float32)
    pcm, clipped = flacgpu.pcm_from_elements_host(x, 16, flacgpu.SAMPLE_F32)
    assert clipped == 2 and len(pcm) == 12
    assert np.frombuffer(pcm, dtype="<i2").tolist() == [16384, 0, -32768, 8192, 32767, -16384]
    pcm2, _ = flacgpu.pcm_from_elements_host(np.ascontiguousarray(x.T), 16, flacgpu.SAMPLE_F32, planar=False)
    assert pcm2 == pcm
    pcm8, c8 = flacgpu.pcm_from_elements_host(np.array([[-128, 127, -129, 5, 300]], dtype=np.int32), 8, flacgpu.SAMPLE_I32)
    assert c8 == 2 and pcm8 == bytes([0x80, 0x7F, 0x80, 5, 0x7F, 0, 0, 0])


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a context was opened")

    monkeypatch.setattr(flacgpu, "Encoder", refuse)
    monkeypatch.setattr(flacgpu, "Decoder", refuse)


def test_from_tensors_refusals_come_before_any_device_use(no_device):
    import torch

    import flacbank

    ft = flacbank.FlacBank.from_tensors
    good = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="no tensors"):
        ft([], 44100)
    with pytest.raises(ValueError, match="channels"):
        ft([good, torch.zeros(1, 100)], 44100)
    with pytest.raises(ValueError, match="one dtype"):
        ft([good, torch.zeros(2, 100, dtype=torch.float16)], 44100)
    with pytest.raises(ValueError, match="dtype"):
        ft([torch.zeros(2, 100, dtype=torch.float64)], 44100)
    with pytest.raises(ValueError, match="dtype"):
        ft([torch.zeros(2, 100, dtype=torch.int16)], 44100)
    for C in (0, 9):
        with pytest.raises(ValueError, match="channels, not 1 to 8"):
            ft([torch.zeros(C, 100)], 44100)
    with pytest.raises(ValueError, match="channels, not 1 to 8"):
        ft([torch.zeros(100, 9)], 44100, planar=False)
    for bits in (0, 12, 20, 64):
        with pytest.raises(ValueError, match="bits"):
            ft([good], 44100, bits=bits)
    for block in (0, 15, 4097, 8192):
        with pytest.raises(ValueError, match="block_size"):
            ft([good], 44100, block_size=block)
    for p in (-1, 13):
        with pytest.raises(ValueError, match="prediction"):
            ft([good], 44100, prediction=p)
    with pytest.raises(ValueError, match="tensor 1 holds no samples"):
        ft([good, torch.zeros(2, 0)], 44100)
    with pytest.raises(ValueError, match="holds no samples"):
        ft(torch.zeros(3, 0, 2), 44100, planar=False)
    with pytest.raises(ValueError, match="more than 65535"):
        ft(torch.zeros(65536, 1, 1), 44100)
    with pytest.raises(ValueError, match="sample_rate"):
        ft([good, good], [44100], bits=16)
    with pytest.raises(ValueError, match="sample_rate"):
        ft([good], 1 << 20)
    with pytest.raises(ValueError, match="dimensions"):
        ft(torch.zeros(2, 100), 44100)
    with pytest.raises(ValueError, match="two dimensions"):
        ft([torch.zeros(100)], 44100)


def test_from_tensors_valid_arguments_get_as_far_as_the_device(monkeypatch):
    import torch

    import flacbank

    class Opened(Exception):
        pass

    def refuse(*a, **k):
        raise Opened()

    monkeypatch.setattr(flacgpu, "Encoder", refuse)
    for kw in (dict(), dict(bits=8), dict(bits=32, block_size=16, prediction=12)):
        with pytest.raises(Opened):
            flacbank.FlacBank.from_tensors([torch.zeros(2, 100), torch.zeros(2, 7)], [44100, 48000], **kw)
    with pytest.raises(Opened):
        flacbank.FlacBank.from_tensors(torch.zeros(3, 50, 8, dtype=torch.int32), 8000, planar=False)


def test_file_bytes_and_clipped_are_part_of_a_bank():
    import flacbank

    assert hasattr(flacbank.FlacBank, "file_bytes") and hasattr(flacbank.FlacBank, "from_tensors")
