"""The channel mix of the delivery of sample windows (zig-flac_amd/csrc/fg_deliver.hpp: mix_valid,
mean_element, mix_element) on the host, under AddressSanitizer and UBSan, through the stand-alone
program tests/cpp/mix_host_main.cpp.  No GPU.

`valid`, `mixes`: the validity rule against its three conditions written out here.  `elements`:
the mean of m = 2, 4, 8 samples as f32 / f16 / bf16 bit patterns against numpy (the exact int64
sum -> f32, times the power of two; f16) and torch on the CPU (bf16): all pairs of 8-bit values,
and per depth a directed set (the limits, 24-bit pairs summing to +-2^24, 32-bit sums on and next
to the ties of the 64-bit -> f32 rounding around every power of two from 2^24 to 2^34, sums whose
f16 result is subnormal) plus 10^5 seeded random tuples; m = 1 against element() and m = 0 against
0 inside the program.  `rows`: the destination rows of a tile, filled by the kernel's own fill_row_slot, against the
rule element by element in a guarded buffer.  Bit patterns are compared; no tolerance."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
I32, F32, F16, BF16 = range(4)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("mixhost")), "mix_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "mix_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


# ---- validity ------------------------------------------------------------------------------------
def mask_ok(C, mask, fmt):
    """The three conditions of a valid mask."""
    m = bin(mask).count("1")
    no_bit_at_or_above_c = mask < (1 << C)
    a_mean_that_is_offered = m in (0, 1, 2, 4, 8)
    integers_take_no_mean = fmt != I32 or m <= 1
    return no_bit_at_or_above_c and a_mean_that_is_offered and integers_take_no_mean


def test_validity_of_every_mask(exe):
    got = run(exe, ["valid"])["valid"]
    assert len(got) == 4 and all(len(g) == 8 and all(len(v) == 256 for v in g) for g in got)
    n_valid = 0
    for fmt in range(4):
        for C in range(1, 9):
            want = [int(mask_ok(C, mask, fmt)) for mask in range(256)]
            assert got[fmt][C - 1] == want, (fmt, C)
            n_valid += sum(want)
    assert got[F32][7][0xFF] == 1 and got[I32][7][0xFF] == 0 and got[F32][6][0xFF] == 0 and got[F32][7][0x07] == 0
    assert got[I32][1] == [1, 1, 1] + [0] * 253 and got[BF16][1] == [1, 1, 1, 1] + [0] * 252
    assert 500 < n_valid < 4 * 8 * 256 // 2  # both answers occur often


def test_validity_of_whole_mixes(exe):
    cases = [  # (C, format, K, NULL, masks) -> valid
        ((2, F32, 2, 0, [1, 2]), 1), ((2, F32, 1, 0, [3]), 1), ((2, I32, 2, 0, [2, 1]), 1), ((2, I32, 1, 0, [3]), 0),
        ((2, F32, 3, 0, [1, 2, 0]), 1), ((2, F32, 3, 0, [1, 2, 4]), 0),      # the last mask names channel 2 of 2
        ((8, F16, 8, 0, [0xFF] * 8), 1), ((8, F16, 8, 0, [0xFF] * 7 + [0x07]), 0),  # a mean of three, last
        ((8, BF16, 2, 0, [0x0F, 0xF0]), 1), ((3, F32, 2, 0, [3, 4]), 1), ((3, F32, 1, 0, [7]), 0),
        ((2, F32, 0, 0, [1, 2]), 0), ((2, F32, 9, 0, [1] * 8), 0), ((2, F32, 2, 1, [1, 2]), 0),  # K of 0 and 9, no masks
        ((2, 4, 2, 0, [1, 2]), 0),                                         # no such format
        ((2, F32, 1, 0, [1, 0xFF]), 1),                                    # masks past K do not count
    ]
    args = []
    for (C, fmt, K, null, masks), _ in cases:
        args += [C, fmt, K, null] + (masks + [0] * 8)[:8]
    assert run(exe, ["mixes"] + args)["valid"] == [want for _, want in cases]


# ---- elements ------------------------------------------------------------------------------------
def expected(x, bits):
    """(f32, f16, bf16) bit patterns of the mean of every row of the int array x [tuples, m]."""
    import torch

    m = x.shape[1]
    log2m = {1: 0, 2: 1, 4: 2, 8: 3}[m]
    s = x.astype(np.int64).sum(axis=1)
    f32 = s.astype(np.float32) * np.float32(2.0 ** -(bits - 1 + log2m))
    f16 = f32.astype(np.float16)
    bf16 = torch.from_numpy(f32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return f32.view(np.uint32), f16.view(np.uint16), bf16


def mix(exe, tmp_path, x, bits):
    m = x.shape[1]
    src, dst = os.path.join(str(tmp_path), f"in{bits}_{m}.bin"), os.path.join(str(tmp_path), f"out{bits}_{m}.bin")
    x.astype("<i4").tofile(src)
    assert run(exe, ["elements", bits, m, src, dst])["count"] == len(x)
    rec = np.fromfile(dst, dtype=np.dtype([("f32", "<u4"), ("f16", "<u2"), ("bf16", "<u2")]))
    return rec["f32"], rec["f16"], rec["bf16"]


def split(s, m, lo, hi, rng):
    """m values in [lo, hi] whose sum is s (which such values can reach)."""
    assert m * lo <= s <= m * hi
    out = []
    for left in range(m - 1, 0, -1):  # what the rest can still make up bounds this one
        a, b = max(lo, s - left * hi), min(hi, s - left * lo)
        v = rng.randint(a, b) if rng.random() < 0.5 else (a if rng.random() < 0.5 else b)
        out.append(v)
        s -= v
    out.append(s)
    assert lo <= s <= hi
    rng.shuffle(out)
    return out


def directed_sums(bits, m):
    """The sums of the directed set, all reachable by m samples of `bits` bits."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = {m * lo, m * hi, m * lo + 1, m * hi - 1, 0, 1, -1, m, -m, m - 1, 1 - m}
    v.update({1 << 24, -(1 << 24), (1 << 24) + 1, -(1 << 24) - 1})  # what the depth and m cannot reach is dropped below
    for k in range(8, 35):  # around every power of two: the ties and near-ties of the three roundings
        for half in {1 << max(k - 24, 0), 1 << max(k - 11, 0), 1 << max(k - 8, 0)}:  # half an ulp of f32 / f16 / bf16 at 2^k
            for odd in (0, 2 * half):  # the tie above an even and above an odd significand
                for d in (-1, 0, 1):
                    for sign in (1, -1):
                        v.add(sign * ((1 << k) + odd + half + d))
        v.update({(1 << k) - 1, (1 << k) + 1, -(1 << k) - 1, -(1 << k) + 1, 1 << k, -(1 << k)})
    # sums whose f16 result is subnormal: |s| * 2^-(bits - 1 + log2 m) < 2^-14, and the ties below its unit 2^-24
    sub = 1 << max(bits - 1 + m.bit_length() - 1 - 14, 0)
    step = max(sub // 512, 1)
    v.update(range(-sub - 3 * step, sub + 3 * step + 1, step))
    v.update(range(-300, 301))
    return sorted(s for s in v if m * lo <= s <= m * hi)


def tuples(bits, m):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = random.Random(f"mix{bits}x{m}")
    rows = [[lo] * m, [hi] * m]
    for s in directed_sums(bits, m):
        rows.append(split(s, m, lo, hi, rng))
        rows.append(split(s, m, lo, hi, rng))
    rows += [[rng.randint(lo, hi) for _ in range(m)] for _ in range(100000)]
    return np.array(rows, dtype=np.int64)


def test_every_pair_of_8_bit_values(exe, tmp_path):
    a = np.arange(-128, 128, dtype=np.int64)
    x = np.stack([np.repeat(a, 256), np.tile(a, 256)], axis=1)
    assert x.shape == (65536, 2)
    for got, want in zip(mix(exe, tmp_path, x, 8), expected(x, 8)):
        assert (got == want).all()
    assert mix(exe, tmp_path, x, 8)[0][0] == 0xBF800000  # -128, -128 is exactly -1.0


@pytest.mark.parametrize("m", [1, 2, 4, 8])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_means_over_a_directed_set(exe, tmp_path, bits, m):
    x = tuples(bits, m)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assert len(x) > 100000 and x.min() == lo and x.max() == hi
    s = x.sum(axis=1)
    f32, f16, bf = expected(x, bits)
    got = mix(exe, tmp_path, x, bits)
    assert got[0][0] == 0xBF800000 and f32[0] == 0xBF800000  # all channels at the minimum: exactly -1.0
    assert s[1] == m * hi and got[0][1] < 0x3F800000 + (bits == 32)  # all at the maximum: below 1.0, or rounded to it
    for name, g, w in zip(("f32", "f16", "bf16"), got, (f32, f16, bf)):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (name, [(x[i].tolist(), hex(int(g[i])), hex(int(w[i]))) for i in bad[:5]])
    # what the set exercises
    sums = set(s.tolist())
    sub16 = int((((f16 & 0x7C00) == 0) & ((f16 & 0x3FF) != 0)).sum())
    assert (sub16 > 0) == (bits - 1 + m.bit_length() - 1 > 14)  # one unit of the sum is 2^-(bits - 1 + log2 m); f16 normals end at 2^-14
    inexact = int((s.astype(np.float32).astype(np.float64) != s.astype(np.float64)).sum())
    if bits == 24 and m == 2:  # two samples reach -2^24 (both at the minimum) and at most 2^24 - 2: every sum converts exactly
        assert {-(1 << 24), (1 << 24) - 2}.issubset(sums) and inexact == 0
    if bits == 24 and m == 4:
        assert {1 << 24, -(1 << 24), (1 << 24) + 1, -(1 << 24) - 1}.issubset(sums) and inexact > 0
    if bits == 32 and m > 1:
        top = 31 + m.bit_length() - 1  # |s| <= 2^top
        assert inexact > 1000
        for k in range(24, top):  # exact ties of the int64 -> f32 rounding at 2^k: half an ulp is 2^(k - 24)
            half = 1 << (k - 24)
            assert {(1 << k) + half, (1 << k) + 3 * half, -(1 << k) - half, (1 << k) + half + 1, (1 << k) + half - 1} <= sums, k
        assert {1 << top, -(1 << top)} & sums  # the last power of two itself, where the depth reaches it
    if bits < 32 and bits + m.bit_length() - 1 <= 25:
        assert inexact == 0


def test_tile_rows_against_the_rule_element_by_element(exe):
    # i32 and f32: 4 alignments; f16 and bf16: 8; 41 lengths, 4 source and 3 output channel counts, 4 flag sets each
    assert run(exe, ["rows"])["cases"] == (4 + 4 + 8 + 8) * 41 * 4 * 3 * 4
