"""The level measurement without a device: flacgpu_levels_host through ctypes against numpy and
Python integers, the refusals of flacgpu_levels_windows_device that come before any device work, its
place in the binding, and the ValueErrors of FlacBank.levels and FlacBank.crop_levels.  (The scalar
rule under sanitizers: tests/test_levels_host.py; through a context: tests/test_gpu_levels.py.)"""
import ctypes
import inspect
import os

import numpy as np
import pytest

import flacgpu
from test_mix_args import _arrays

HERE = os.path.dirname(os.path.abspath(__file__))


def f64_bits(values):
    return np.array([float(int(v)) for v in values], dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_host_statement_against_python_integers(bits, C):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = np.random.default_rng([bits, C])
    n = 2003
    x = rng.integers(lo, hi + 1, size=(n, C), dtype=np.int64)
    x[10:30] = lo
    x[30:50:2], x[31:50:2] = lo, hi
    x[50:60] = 0
    for hop in (1, 3, 64, 1000, n + 5):
        peak, total, energy = flacgpu.levels_host(x, hop)
        blocks = (n + hop - 1) // hop
        assert peak.shape == total.shape == energy.shape == (blocks, C)
        assert (peak.dtype, total.dtype, energy.dtype) == (np.uint32, np.int64, np.float64)
        at = np.arange(0, n, hop)
        assert (peak == np.maximum.reduceat(np.abs(x), at, axis=0)).all() and (total == np.add.reduceat(x, at, axis=0)).all()
        sq = [sum(int(v) * int(v) for v in x[j * hop:(j + 1) * hop, c]) for j in range(blocks) for c in range(C)]
        assert (energy.view(np.uint64).reshape(-1) == f64_bits(sq)).all(), hop
        if bits == 32 and hop >= 1000:
            assert max(sq) >= 1 << 64 and any(int(float(v)) != v for v in sq)  # past 64 bits, and rounded
    assert peak.max() == -lo


def test_host_statement_argument_checks():
    f = flacgpu.load_library().flacgpu_levels_host
    x = (ctypes.c_int32 * 6)(1, -2, 3, -4, 5, -(1 << 31))
    peak, total, energy = (ctypes.c_uint32 * 4)(), (ctypes.c_int64 * 4)(), (ctypes.c_double * 4)()
    assert f(x, 3, 2, 2, peak, total, energy) == 0
    assert list(peak) == [3, 4, 5, 1 << 31] and list(total) == [4, -6, 5, -(1 << 31)]
    assert list(energy) == [10.0, 20.0, 25.0, 2.0 ** 62]
    assert f(x, 3, 2, 0, peak, total, energy) == -2          # no hop
    assert f(x, 3, 2, 1 << 31, peak, total, energy) == -2    # a hop of 2^31
    assert f(x, 3, 2, (1 << 31) - 1, peak, total, energy) == 0
    assert f(x, 3, 0, 2, peak, total, energy) == -2          # no channel
    assert f(x, (1 << 40) + 1, 2, 2, peak, total, energy) == -2
    for a in ((None, peak, total, energy), (x, None, total, energy), (x, peak, None, energy), (x, peak, total, None)):
        assert f(a[0], 3, 2, 2, *a[1:]) == -2
    assert f(None, 0, 2, 2, None, None, None) == 0           # nothing to do
    assert flacgpu.levels_host(np.zeros((0, 2), np.int32), 5)[0].shape == (0, 2)
    for bad, why in ((np.zeros(4, np.int32), "integer array"), (np.zeros((2, 2), np.float32), "integer array"),
                     (np.array([[1 << 31]]), "outside 32 bits")):
        with pytest.raises(ValueError, match=why):
            flacgpu.levels_host(bad, 2)
    for hop in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="hop"):
            flacgpu.levels_host(np.zeros((2, 2), np.int32), hop)


def test_levels_windows_argument_checks_without_a_device():
    f = flacgpu.load_library().flacgpu_levels_windows_device
    buf, u64, u32 = _arrays()
    head = (buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64)
    out = ctypes.create_string_buffer(128)
    a = ctypes.addressof(out)
    a += (-a) % 8
    arrays = (ctypes.c_void_p(a), ctypes.c_void_p(a + 32), ctypes.c_void_p(a + 64))
    tail = (u64, u64, buf, None)
    assert f(None, *head, 64, *arrays, *tail) == -2                     # no context
    # a context that no call may dereference before its checks: every refusal below comes first
    fake = ctypes.create_string_buffer(4096)
    assert f(fake, *head, 0, *arrays, *tail) == -2                      # no hop
    assert f(fake, *head, 1 << 31, *arrays, *tail) == -2                # a hop of 2^31
    for k in range(3):
        gone = list(arrays)
        gone[k] = None
        assert f(fake, *head, 64, *gone, *tail) == -2                   # a NULL output array
    assert f(fake, *head, 64, ctypes.c_void_p(a + 2), arrays[1], arrays[2], *tail) == -2   # peak not on 4 bytes
    assert f(fake, *head, 64, arrays[0], ctypes.c_void_p(a + 36), arrays[2], *tail) == -2  # sum not on 8
    assert f(fake, *head, 64, arrays[0], arrays[1], ctypes.c_void_p(a + 68), *tail) == -2  # energy not on 8
    wrap = (ctypes.c_uint64 * 2)(1, (1 << 64) - 1)
    assert f(fake, *head, 64, *arrays, wrap, u64, buf, None) == -2      # offset + cap passes 64 bits
    # the existing argument errors
    assert f(fake, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, 64, *arrays, *tail) == -2
    assert f(fake, buf, 1, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, 64, *arrays, *tail) == -2  # a window names stream 1 of 1
    assert f(fake, None, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64, 64, *arrays, *tail) == -2
    assert f(fake, *head, 64, *arrays, None, u64, buf, None) == -2
    assert f(fake, *head, 64, *arrays, u64, u64, None, None) == -2


def test_binding():
    names = {"flacgpu_levels_windows_device", "flacgpu_levels_host"}
    assert names <= set(flacgpu.exported_symbols())
    for name in names:
        assert hasattr(flacgpu.load_library(), name)
    assert hasattr(flacgpu.Decoder, "levels_windows_device") and callable(flacgpu.levels_host)
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    assert "uint32_t hop, uint32_t *d_peak, int64_t *d_sum, double *d_energy," in text
    assert "int flacgpu_levels_host(const int32_t *samples, uint64_t n, uint32_t channels, uint32_t hop, uint32_t *peak," in text
    d = flacgpu.Decoder.__new__(flacgpu.Decoder)  # no context: a call that got to the library would fail otherwise
    with pytest.raises(flacgpu.FlacGpuError, match="hop"):
        d.levels_windows_device(0, [0], 0, 0, 0, 0, 0, [(0, 0, 1)], 1 << 32, 0, 0, 0, [0], [1], 0)


def _bank_without_a_device():
    """A FlacBank as far as the checks look at it; its context is an object no call may reach."""
    import flacbank

    b = flacbank.FlacBank.__new__(flacbank.FlacBank)
    b._dec = object()
    b.channels, b.bits, b.samples, b.sample_rates = 2, 16, [1000, 0, 5], [44100] * 3
    b.device = None
    return b


def test_flacbank_levels_and_crop_levels_refuse_before_the_device(monkeypatch):
    import flacbank
    import torch

    def refuse(*a, **k):
        raise AssertionError("the device was used")

    monkeypatch.setattr(torch.cuda, "device", refuse)
    monkeypatch.setattr(torch.cuda, "current_stream", refuse)
    b = _bank_without_a_device()
    for hop in (0, -5, 1 << 31):
        with pytest.raises(ValueError, match="the hop is 1 to 2\\^31 - 1"):
            b.levels(hop)
    for kw in (dict(span=0), dict(scratch_bytes=0), dict(span=-1)):
        with pytest.raises(ValueError, match="span and scratch_bytes"):
            b.levels(64, **kw)
    for args, why in ((([0, 1], [0], 10), "differ in length"), (([3], [0], 10), "out of range"), (([-1], [0], 10), "out of range"),
                      (([0], [-1], 10), "out of range"), (([0], [0], -1), "out of range"), (([0], [0], 1 << 31), "out of range")):
        with pytest.raises(ValueError, match=why):
            b.crop_levels(*args)
    b._dec = None
    with pytest.raises(ValueError, match="closed"):
        b.levels(64)
    with pytest.raises(ValueError, match="closed"):
        b.crop_levels([0], [0], 10)
    b._data = b._off = b._fbytes = b._ires = b._pos = b._totals = None  # what close() leaves, for __del__
    p = inspect.signature(flacbank.FlacBank.levels).parameters
    assert list(p) == ["self", "hop", "span", "scratch_bytes"] and p["span"].default == 1 << 20 and p["scratch_bytes"].default == 1 << 30
    p = inspect.signature(flacbank.FlacBank.crop_levels).parameters
    assert list(p) == ["self", "file", "start", "length", "strict"] and p["strict"].default is True
    for name in ("file", "rms_dbfs", "active"):
        assert callable(getattr(flacbank.BankLevels, name))
