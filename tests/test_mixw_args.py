"""The weighted channel mix without a device: flacgpu_mix_weights_valid and
flacgpu_mix_weights_f32_host through ctypes against tests/mixw_ref.py, the refusals of
flacgpu_decode_windows_device_to that come before any device work, its place in the binding, the
matrix form of FlacMixBank's channel_map, downmix= and flacbank.downmix_matrix (bit patterns pinned
in tests/golden/downmix_matrices.json, written once from the double-precision formula)."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import flacgpu
import mixw_ref
from test_mix_args import _arrays, _masks, sources  # noqa: F401  (sources is a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))


def _f32(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


def test_validity_through_the_library():
    L = flacgpu.load_library()
    lo, hi = (127 - 32) << 23, (127 + 32) << 23

    def valid(C, K, bit_patterns, fmt=flacgpu.SAMPLE_F32):
        w = (ctypes.c_uint32 * max(len(bit_patterns), 1))(*bit_patterns)
        return L.flacgpu_mix_weights_valid(C, K, w, fmt)

    one = 0x3F800000
    for u, want in ((lo, 1), (lo - 1, 0), (hi, 1), (hi + 1, 0), (lo | 1 << 31, 1), ((hi + 1) | 1 << 31, 0), (0, 1), (1 << 31, 1),
                    (0x7F800000, 0), (0xFF800000, 0), (0x7FC00000, 0), (1, 0), (0x007FFFFF, 0), (one, 1)):
        assert valid(1, 1, [u]) == want, hex(u)
        assert valid(8, 8, [one] * 63 + [u]) == want, hex(u)
    for C, K, want in ((0, 1, 0), (1, 0, 0), (9, 1, 0), (1, 9, 0), (8, 8, 1), (1, 1, 1)):
        assert valid(C, K, [one] * 64) == want, (C, K)
    for fmt, want in ((flacgpu.SAMPLE_I32, 0), (flacgpu.SAMPLE_F32, 1), (flacgpu.SAMPLE_F16, 1), (flacgpu.SAMPLE_BF16, 1), (4, 0)):
        assert valid(2, 2, [one] * 4, fmt) == want
    assert L.flacgpu_mix_weights_valid(2, 2, None, flacgpu.SAMPLE_F32) == 0
    assert flacgpu.mix_weights_valid([[0.5, 0.5], [0.5, -0.5]]) and not flacgpu.mix_weights_valid([[float("inf")]])
    assert not flacgpu.mix_weights_valid([[1.0]], flacgpu.SAMPLE_I32)


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_host_statement_against_the_reference(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for C, K in ((1, 1), (2, 2), (3, 1), (6, 2), (8, 8)):
        rng = np.random.default_rng([bits, C, K])
        x = rng.integers(lo, hi + 1, size=(3000, C), dtype=np.int64)
        x[0], x[1], x[2] = lo, hi, 0
        W = (rng.uniform(1.0, 2.0, size=(K, C)) * np.exp2(rng.integers(-32, 32, size=(K, C))) *
             rng.choice([-1.0, 1.0], size=(K, C))).astype(np.float32)
        W[rng.random(size=(K, C)) < 0.2] = 0.0
        got = flacgpu.mix_weights_f32_host(x, bits, W)
        assert got.shape == (3000, K) and (got.view(np.uint32) == mixw_ref.mix(x, bits, W).view(np.uint32)).all()
    ms = flacgpu.mix_weights_f32_host(np.array([[7, 7], [lo, lo], [hi, lo]]), bits, [[0.5, 0.5], [0.5, -0.5]])
    assert ms.view(np.uint32)[0, 1] == 0 and ms.view(np.uint32)[1, 1] == 0 and ms[1, 0] == -1.0  # +0.0f, never -0.0f


def test_host_statement_argument_checks():
    L = flacgpu.load_library()
    x = (ctypes.c_int32 * 4)(1, 2, 3, 4)
    w = (ctypes.c_float * 4)(0.5, 0.5, 0.5, -0.5)
    y = (ctypes.c_float * 4)()
    f = L.flacgpu_mix_weights_f32_host
    assert f(x, 2, 2, 16, 2, w, y) == 0 and list(y) == [1.5 / 32768, -0.5 / 32768, 3.5 / 32768, -0.5 / 32768]
    assert f(x, 2, 2, 12, 2, w, y) == -2          # no such depth
    assert f(x, 2, 2, 16, 2, None, y) == -2       # no weights
    assert f(x, 2, 9, 16, 2, w, y) == -2 and f(x, 2, 2, 16, 0, w, y) == -2
    assert f(None, 2, 2, 16, 2, w, y) == -2 and f(x, 2, 2, 16, 2, w, None) == -2
    assert f(None, 0, 2, 16, 2, w, None) == 0     # nothing to do
    big = (ctypes.c_int32 * 2)(128, 0)
    assert f(big, 1, 2, 8, 2, w, y) == -2         # 128 is no 8-bit sample
    bad = (ctypes.c_float * 4)(0.5, float("nan"), 0.5, -0.5)
    assert f(x, 2, 2, 16, 2, bad, y) == -2
    with pytest.raises(ValueError, match="outside 8 bits"):
        flacgpu.mix_weights_f32_host(np.array([[128]]), 8, [[1.0]])


def _how(**kw):
    h = flacgpu.WindowDelivery(ctypes.sizeof(flacgpu.WindowDelivery), flacgpu.SAMPLE_F32, 0, 2, None, None, 0, 0, None, None)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_decode_windows_to_argument_checks_without_a_device():
    L = flacgpu.load_library()
    buf, u64, u32 = _arrays()
    f = L.flacgpu_decode_windows_device_to
    head = (buf, 2, u64, buf, buf, buf, buf, buf, 2, u32, u64, u64)
    tail = (buf, u64, u64, buf, None)
    w = (ctypes.c_float * 4)(0.5, 0.5, 0.5, -0.5)
    pw, pm = ctypes.cast(w, ctypes.c_void_p), ctypes.cast(_masks(1, 2), ctypes.c_void_p)
    assert f(None, *head, ctypes.byref(_how(channel_weights=pw)), *tail) == -2  # no context
    assert f(None, *head, None, *tail) == -2                                   # no delivery
    assert f(None, *head, ctypes.byref(_how(size=48, channel_weights=pw)), *tail) == -2
    assert f(None, *head, ctypes.byref(_how(channel_weights=pw, channel_masks=pm)), *tail) == -2
    assert f(None, buf, 2, u64, buf, buf, buf, buf, buf, 65536, u32, u64, u64, ctypes.byref(_how(channel_weights=pw)), *tail) == -2
    assert ctypes.sizeof(flacgpu.WindowDelivery) == 56


def test_binding():
    assert {"flacgpu_decode_windows_device_to", "flacgpu_mix_weights_valid", "flacgpu_mix_weights_f32_host"} <= set(
        flacgpu.exported_symbols())
    for name in ("flacgpu_decode_windows_device_to", "flacgpu_mix_weights_valid", "flacgpu_mix_weights_f32_host"):
        assert hasattr(flacgpu.load_library(), name)
    assert hasattr(flacgpu.Decoder, "decode_windows_device_to")
    assert flacgpu.K_INDEX == 7 and len(flacgpu.KERNEL_NAMES) == 5  # no kernel ids added
    assert flacgpu.load_library().flacgpu_abi_version() == 5
    with open(os.path.join(HERE, "..", "include", "flacgpu.h")) as f:
        text = f.read()
    assert "} flacgpu_window_delivery;" in text and "const float *channel_weights;" in text
    assert "const flacgpu_window_delivery *how" in text


# ---- FlacMixBank -----------------------------------------------------------------------------------
class Opened(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise Opened()

    monkeypatch.setattr(flacgpu, "Decoder", refuse)


def test_flacmixbank_downmix_gets_as_far_as_the_context(no_device, sources):  # noqa: F811
    import flacbank

    s = sources
    with pytest.raises(Opened):
        flacbank.FlacMixBank([s["stereo16"], s["three8"]], channels=2, downmix="itu")
    with pytest.raises(Opened):
        flacbank.FlacMixBank([s["stereo16"], s["three8"]], channels=1, downmix="mean")
    with pytest.raises(Opened):
        flacbank.FlacMixBank([s["stereo16"], s["three8"]], channels=2, channel_map={2: [[0.5, 0.5], [0.5, -0.5]],
                                                                                    3: np.array([[1, 0, 0.5], [0, 1, 0.5]])})
    # without downmix: today's message
    with pytest.raises(ValueError, match=r"file 1 has 3 channels and there is no default mix of 3 channels to 2: give channel_map\[3\]"):
        flacbank.FlacMixBank([s["stereo16"], s["three8"]], channels=2)
    # "itu" has nothing for 2 channels to 3
    with pytest.raises(ValueError, match="file 0 has 2 channels and there is no default mix"):
        flacbank.FlacMixBank([s["stereo16"]], channels=3, downmix="itu")
    with pytest.raises(ValueError, match="file 1 has 3 channels and there is no default mix"):
        flacbank.FlacMixBank([s["stereo16"], s["three8"]], channels=2, downmix="mean")
    with pytest.raises(ValueError, match="downmix is None, 'mean' or 'itu'"):
        flacbank.FlacMixBank([s["stereo16"]], channels=2, downmix="ITU")


def test_flacmixbank_weight_errors_name_the_callers_file(no_device, sources):  # noqa: F811
    import flacbank

    s = sources
    files = [s["mono16"], s["stereo16"], s["three8"]]
    for bad, why in (([[1.0, 0.5, float("nan")]], r"weight \[0\]\[2\] \(nan\)"), ([[1.0, 2.0 ** 33, 0]], r"weight \[0\]\[1\]"),
                     ([[1e-45, 0, 0]], r"weight \[0\]\[0\]"), ([[1.0, 1.0]], "1 rows of 2 weights, not 1 rows of 3"),
                     ([[1.0, 0, 0], [0, 1.0, 0]], "2 rows of 3 weights, not 1 rows of 3"),
                     ([[1.0, 0, 0], 7], "mixes masks and rows"), ([7, [1.0, 0, 0]], "mixes masks and rows"),
                     ([[1.0, 0], [1.0, 0, 0]], "differ in length"), (np.zeros((1, 1, 3)), "3 dimensions")):
        with pytest.raises(ValueError, match=rf"channel_map\[3\], which file 2 needs, is not valid: .*{why}"):
            flacbank.FlacMixBank(files, channels=1, channel_map={3: bad})
    # masks keep today's messages beside a weighted entry
    with pytest.raises(ValueError, match=r"channel_map\[3\], which file 2 needs.*mean of 3"):
        flacbank.FlacMixBank(files, channels=1, channel_map={2: [[0.5, 0.5]], 3: [7]})


# ---- downmix_matrix ----------------------------------------------------------------------------------
def test_downmix_matrices_are_pinned_valid_and_normalised():
    import flacbank

    with open(os.path.join(HERE, "golden", "downmix_matrices.json")) as f:
        golden = json.load(f)
    assert len(golden["itu"]) == 12 and len(golden["mean"]) == 8
    seen = 0
    for kind in ("itu", "mean"):
        for name, rows in golden[kind].items():
            C, K = (int(v) for v in name.split("to"))
            w = flacbank.downmix_matrix(C, K, kind)
            assert w.dtype == np.float32 and w.shape == (K, C)
            assert [[f"{int(u):08x}" for u in row] for row in w.view(np.uint32)] == rows, (kind, name)
            assert flacgpu.mix_weights_valid(w)
            for row in w:
                total = float(np.sum(row.astype(np.float64)))
                assert abs(total - 1.0) <= 2 * 2.0 ** -23, (kind, name, total)  # within 2 ulp of 1
                assert (row >= 0).all()
            seen += 1
    assert seen == 20
    six = flacbank.downmix_matrix(6, 2, "itu")
    assert six[0, 3] == 0 and six[1, 3] == 0 and six[0, 1] == 0 and six[0, 2] == six[1, 2] == six[0, 4] == six[1, 5]  # LFE dropped
    assert (flacbank.downmix_matrix(3, 1, "mean") == np.float32(1.0 / 3)).all()
    for C, K, kind in ((2, 2, "itu"), (2, 1, "itu"), (6, 3, "itu"), (9, 1, "mean"), (6, 2, "mean"), (0, 1, "mean"), (6, 2, "rms")):
        with pytest.raises(ValueError, match="downmix_matrix"):
            flacbank.downmix_matrix(C, K, kind)
