"""The feature rule of the delivery of sample windows (zig-flac_amd/csrc/fg_features.hpp) on the
host, under AddressSanitizer and UBSan, through the stand-alone program
tests/cpp/features_host_main.cpp, against tests/features_ref.py (numpy float64, np.fft.rfft).  No GPU.

`table`: the library's table against the formula to one float ulp (two libms may differ in the last
bit of a cosine), and against the program's.  `rule`: flacgpu_features_f32_host against
features_ref under the bound derived there from u = 2^-24 -- every element, and the bound itself
below 1/256 of the case's largest value -- and against the program bit for bit; inside the program
the powers against a plain double DFT, the zero extension, and dense against zero-skipping filter
chains.  `narrow`: f16 (infinity from 65520 on) and bf16 against numpy and torch on the CPU.
`geometry`: feat_geometry over every (n_fft, hop), with and without a filter bank."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flacgpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import features_ref as ref  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "..", "zig-flac_amd"))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("featureshost")), "features_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "features_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


# ---- the table -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [16, 34, 64, 400, 512, 2048])
def test_table_against_the_formula(exe, tmp_path, n_fft):
    t = flacgpu.features_table(n_fft)
    B = n_fft // 2 + 1
    assert t.shape == (2, B, n_fft) and t.dtype == np.float32
    t64 = ref.table64(n_fft)
    want = t64.astype(np.float32)
    # one float ulp at the entry's magnitude, and the absolute error of a float64 cosine near its zeros
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    assert (np.abs(t.astype(np.float64) - t64) <= ulp + 2.0 ** -50).all()
    assert (t[0, 0] == ref.hann(n_fft).astype(np.float32)).all() and (t[1, 0] == 0).all()  # bin 0: the window itself
    assert t[0, :, 0].max() == 0 and abs(float(t[0, 1, n_fft // 2]) + 1.0) < 1e-6  # w[0] = 0, w[N/2] cos(pi) = -1
    if n_fft <= 512:
        path = os.path.join(str(tmp_path), "t.bin")
        assert run(exe, ["table", n_fft, path]) == {"B": B, "n": 2 * B * n_fft}
        assert (np.fromfile(path, dtype="<f4").view(np.uint32) == t.reshape(-1).view(np.uint32)).all()


def test_table_refusals_and_sizes():
    import ctypes

    f, n = flacgpu.load_library().flacgpu_features_table, ctypes.c_size_t(9)
    for bad in (0, 14, 17, 401, 2050, 4096):
        assert f(bad, None, 0, ctypes.byref(n)) == -2, bad
    assert f(400, None, 0, None) == -2 and f(400, None, 10, ctypes.byref(n)) == -2
    assert f(400, None, 0, ctypes.byref(n)) == -4 and n.value == 2 * 201 * 400
    small = (ctypes.c_float * 100)()
    assert f(400, small, 100, ctypes.byref(n)) == -4 and all(v == 0.0 for v in small)


# ---- the rule --------------------------------------------------------------------------------------
def mel_like(rows, B, seed):
    """Rows with a band of positive entries and zeros elsewhere; of three rows or more the last is all zero."""
    rng = np.random.RandomState(seed)
    F = np.zeros((rows, B), dtype=np.float32)
    for r in range(rows - 1 if rows > 2 else rows):
        lo = (r * B) // rows
        hi = min(B, lo + max(2, (2 * B) // rows))
        F[r, lo:hi] = rng.uniform(0.0, 1.0, hi - lo).astype(np.float32)
    return F


CASES = [  # n_fft, hop, rows, total, [(start, frames)]
    (64, 16, 0, 700, [(0, 30), (5, 12), (650, 10), (700, 3), (900, 2), (31, 1)]),
    (34, 7, 1, 300, [(0, 20), (3, 50), (299, 4)]),
    (400, 160, 80, 3000, [(0, 19), (100, 25), (2900, 3)]),
    (512, 128, 0, 2000, [(0, 16), (255, 17)]),
    (2048, 512, 128, 6000, [(0, 12), (1000, 3)]),
    (2048, 2048, 0, 6000, [(0, 3), (1, 4)]),
]


@pytest.mark.parametrize("n_fft,hop,rows,total,windows", CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}" for c in CASES])
def test_rule_against_float64_and_the_program(exe, tmp_path, n_fft, hop, rows, total, windows):
    B = n_fft // 2 + 1
    x = ref.tone(total, n_fft, max(2, n_fft // 8), seed=n_fft + hop)
    F = mel_like(rows, B, rows) if rows else None
    a, fb, yb = (os.path.join(str(tmp_path), n) for n in ("x.bin", "f.bin", "y.bin"))
    x.astype("<f4").tofile(a)
    if rows:
        F.astype("<f4").tofile(fb)
    for start, frames in windows:
        y, n = flacgpu.features_f32_host(x, n_fft, hop, start, frames, F)
        y64, bound, n64 = ref.features64(x, n_fft, hop, start, frames, F)
        assert y.shape == y64.shape == (rows or B, frames) and n == n64 == ref.delivered(total, start, frames, hop)
        err = np.abs(y.astype(np.float64) - y64)
        print(f"n_fft {n_fft} hop {hop} rows {rows} start {start}: max err {err.max():.3e}, max err / bound "
              f"{(err / bound).max():.3f}, max bound / max value {bound.max() / max(y64.max(), 1e-300):.3e}")
        bad = np.argwhere(err > bound)
        assert len(bad) == 0, (start, frames, [(tuple(i), float(y[tuple(i)]), float(y64[tuple(i)])) for i in bad[:5]])
        if y64.max() > 0:
            assert bound.max() < y64.max() / 256.0  # a loose bound cannot pass a wrong result
        info = run(exe, ["frames", n_fft, hop, rows, start, frames, a, fb if rows else "-", yb])
        assert (info["rows"], info["frames"], info["n"]) == (rows or B, frames, n)
        assert info["over_bound"] == 0 and info["skip_differs"] == 0 and info["worst"] < 1.0
        got = np.fromfile(yb, dtype="<f4").reshape(rows or B, frames)
        assert (got.view(np.uint32) == y.view(np.uint32)).all(), (start, frames)


def test_zero_extension_at_both_ends(exe, tmp_path):
    """A constant signal: an interior frame sees the whole window, the first and the last see half of
    it and zeros -- not a reflected or clamped edge -- and a frame wholly outside is +0.0f."""
    n_fft, hop, total = 64, 32, 640
    x = np.ones(total, dtype=np.float32)
    y, n = flacgpu.features_f32_host(x, n_fft, hop, 0, 24)
    assert n == 20 and y.shape == (33, 24)
    dc = y[0]
    full = float(np.sum(ref.hann(n_fft))) ** 2
    first, last = float(np.sum(ref.hann(n_fft)[32:])) ** 2, float(np.sum(ref.hann(n_fft)[:32])) ** 2  # 16.5^2 and 15.5^2
    assert abs(dc[5] / full - 1.0) < 1e-5 and abs(dc[0] / first - 1.0) < 1e-5 and abs(dc[20] / last - 1.0) < 1e-5
    assert (y[:, 21:].view(np.uint32) == 0).all() and dc[19] > 0.9 * full  # frames 21.. reach nothing: +0.0f
    a, yb = os.path.join(str(tmp_path), "x.bin"), os.path.join(str(tmp_path), "y.bin")
    x.tofile(a)
    info = run(exe, ["frames", n_fft, hop, 0, 0, 24, a, "-", yb])
    assert info["zero_frames"] == 3 and info["over_bound"] == 0
    assert (np.fromfile(yb, dtype="<f4").reshape(33, 24).view(np.uint32) == y.view(np.uint32)).all()


def test_host_rule_refusals():
    import ctypes

    f = flacgpu.load_library().flacgpu_features_f32_host
    x, y, n = (ctypes.c_float * 64)(*([0.25] * 64)), (ctypes.c_float * 4096)(), ctypes.c_uint64(99)
    F = (ctypes.c_float * (2 * 9))(*([1.0] * 18))

    def ft(N, H, R):
        return ctypes.byref(flacgpu.Features(N, H, R))

    assert f(x, 64, ft(16, 4, 0), None, 0, 8, y, ctypes.byref(n)) == 0 and n.value == 8
    assert f(x, 64, ft(16, 4, 2), F, 60, 8, y, ctypes.byref(n)) == 0 and n.value == 1
    assert f(x, 64, ft(16, 4, 0), None, 64, 8, y, ctypes.byref(n)) == 0 and n.value == 0
    assert f(x, 64, ft(16, 4, 0), None, 0, 0, None, ctypes.byref(n)) == 0 and n.value == 0
    for N, H, R in ((14, 4, 0), (18, 0, 0), (16, 17, 0), (17, 4, 0), (2050, 4, 0), (16, 4, 257)):
        assert f(x, 64, ft(N, H, R), F, 0, 8, y, ctypes.byref(n)) == -2, (N, H, R)
    assert f(x, 64, None, None, 0, 8, y, ctypes.byref(n)) == -2
    assert f(x, 64, ft(16, 4, 2), None, 0, 8, y, ctypes.byref(n)) == -2      # rows without a matrix
    assert f(None, 64, ft(16, 4, 0), None, 0, 8, y, ctypes.byref(n)) == -2   # samples without a buffer
    assert f(x, 64, ft(16, 4, 0), None, 0, 8, None, ctypes.byref(n)) == -2   # frames without a buffer
    assert f(x, 64, ft(16, 4, 0), None, 0, 8, y, None) == -2
    assert f(x, (1 << 40) + 1, ft(16, 4, 0), None, 0, 8, y, ctypes.byref(n)) == -2
    assert f(x, 64, ft(16, 16, 0), None, 0, 1 << 27, y, ctypes.byref(n)) == -2  # a span of 2^31
    F[3] = float("inf")
    assert f(x, 64, ft(16, 4, 2), F, 0, 8, y, ctypes.byref(n)) == -2


# ---- narrowing -------------------------------------------------------------------------------------
def test_narrowing_of_power(exe, tmp_path):
    import torch

    rng = np.random.RandomState(9)
    v = [np.array([0.0, 1.0, 65503.9, 65504.0, 65519.996, 65520.0, 65521.0, 65536.0, 2.0 ** 18, 1e9, 3e38, 2.0 ** -24, 2.0 ** -25,
                   6e-8, 1e-30], np.float32),
         (10.0 ** rng.uniform(-12, 8, 100000)).astype(np.float32), rng.uniform(65000, 66000, 5000).astype(np.float32)]
    for e in range(-16, 17, 4):  # ties and their neighbours around 2^e
        for mant in (10, 7):
            ulp = 2.0 ** (e - mant)
            base = 2.0 ** e + ulp * np.arange(0, 300, dtype=np.float64)
            for off in (0.5, 0.5 - 2.0 ** -12, 0.5 + 2.0 ** -12):
                v.append((base + off * ulp).astype(np.float32))
    x = np.concatenate(v)
    a, b = os.path.join(str(tmp_path), "v.bin"), os.path.join(str(tmp_path), "n.bin")
    x.astype("<f4").tofile(a)
    assert run(exe, ["narrow", a, b])["count"] == len(x)
    rec = np.fromfile(b, dtype=np.dtype([("f16", "<u2"), ("bf16", "<u2")]))
    with np.errstate(over="ignore"):
        want16 = x.astype(np.float16).view(np.uint16)
    wantbf = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (rec["f16"] == want16).all() and (rec["bf16"] == wantbf).all()
    assert rec["f16"][3] == 0x7BFF and rec["f16"][4] == 0x7BFF and (rec["f16"][5:11] == 0x7C00).all()  # 65504, then infinity


# ---- geometry --------------------------------------------------------------------------------------
def test_geometry_over_the_whole_domain(exe):
    g = run(exe, ["geometry"])
    n_pairs = sum(n for n in range(16, 2049, 2))
    assert g["checked"] == 3 * n_pairs and g["bad"] == 0
    assert g["min_frames"] >= 1 and 60000 < g["max_lds"] <= 65536
    assert g["hist"][5] > 0 and g["hist"][2] > 0  # tiles of 32 frames, and of 4 where n_fft and the hop are large
    assert g["g400"][0] == 32 and g["g400"][1] <= 65536 and g["g2048_2048"][0] == 4 and g["g2048_512_128"][0] == 8
