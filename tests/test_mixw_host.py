"""The weighted channel mix of the delivery of sample windows (zig-flac_amd/csrc/fg_deliver.hpp:
mixw_valid, mixw_step, mixw_value, mixw_element) on the host, under AddressSanitizer and UBSan,
through the stand-alone program tests/cpp/mixw_host_main.cpp.  No GPU.

`valid`: the validity rule against its conditions written out here (C and K in 1..8, a float
format, every weight 0 or 2^-32 <= |w| <= 2^32): the bounds, one ulp outside each, NaN, infinity,
subnormals, -0.0f, K and C of 0 and 9, I32.  `elements`: the chain as f32 / f16 / bf16 bit
patterns against tests/mixw_ref.py (float64 with an explicit correction of the double rounding,
itself checked here against exact rational arithmetic) for C in 1..8 and every depth: every pair of
8-bit values under {0.5, 0.5} and {0.5, -0.5}; per depth a directed set (the limits, equal samples
under {1, -1}, weights at 2^-32 and 2^32, the ITU rows, 1/3, 1/5, 1/6, 1/7, 32-bit samples on the
ties of the int -> float rounding) and 10^5 seeded tuples under seeded weights.  `equiv`: identity
and unit rows against element() and the one-channel mask, {0.5, 0.5} against the mask mean, inside
the program.  `rows`: the destination rows of a tile, filled by the kernel's own fill_row_slot,
against the chain element by element in a guarded buffer.  Bit patterns are compared; no tolerance."""
import json
import math
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import mixw_ref
from test_mix_host import directed_sums, split

HERE = os.path.dirname(os.path.abspath(__file__))
I32, F32, F16, BF16 = range(4)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("mixwhost")), "mixw_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "mixw_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def bits_of(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


# ---- the reference itself ------------------------------------------------------------------------
def test_reference_fma_against_exact_rational_arithmetic():
    """fma32 (float64, corrected) equals the Fraction fma where the correction matters: sums that
    sit on a float32 tie in float64 but not exactly, and seeded operands of far-apart magnitudes."""
    rng = random.Random("mixw-ref")
    cases = []
    for _ in range(3000):
        a = f32(rng.getrandbits(23) | ((127 + rng.randint(-32, 32)) << 23) | (rng.getrandbits(1) << 31))
        b = f32(rng.getrandbits(23) | ((127 - rng.randint(0, 31)) << 23) | (rng.getrandbits(1) << 31))
        c = f32(rng.getrandbits(23) | ((127 + rng.randint(-40, 34)) << 23) | (rng.getrandbits(1) << 31))
        cases.append((a, b, c))
    for k in (0, 5, 20, 30):  # c = 2^k + half an ulp of f32 at 2^k exactly, the product a sliver either way: a tie that is none
        big = float(np.float32(2.0 ** k))
        for sign in (1.0, -1.0):
            cases.append((float(np.float32(2.0 ** -32)) * sign, float(np.float32(2.0 ** -31)), big))
            cases.append((float(np.float32(2.0 ** (k - 24))), 1.0, big))                        # an exact tie: to even
            cases.append((float(np.float32(2.0 ** (k - 24))), 1.0, float(np.float32(big * (1 + 2.0 ** -23)))))  # a tie above an odd one
            cases.append((float(np.float32(2.0 ** (k - 24) * (1 + sign * 2.0 ** -23))), 1.0, big))  # just off the tie
    # the product 2^m (1 - 2^-46) = 2^m (1 + 2^-23) (1 - 2^-23) lies a sliver below half an ulp of c = 2^(m + 24) (1 + 2^-23),
    # whose significand is odd: the sum rounds down; float64 drops the sliver, lands on the tie and would round up to even
    for m in (-30, -8, 0, 7):
        for sign in (1.0, -1.0):
            cases.append((sign * 2.0 ** m * (1 + 2.0 ** -23), 1 - 2.0 ** -23, sign * 2.0 ** (m + 24) * (1 + 2.0 ** -23)))
            cases.append((sign * 2.0 ** m * (1 + 2.0 ** -23), 1 - 2.0 ** -23, sign * 2.0 ** (m + 24) * (1 + 3 * 2.0 ** -23)))
    a, b, c = (np.array(v, dtype=np.float32) for v in zip(*cases))
    got = mixw_ref.fma32(a, b, c)
    want = np.array([mixw_ref.fma32_exact(*t) for t in cases], dtype=np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (plain.view(np.uint32) != want.view(np.uint32)).any()  # plain float64 is not exact: the set shows it


# ---- validity ------------------------------------------------------------------------------------
LO, HI = (127 - 32) << 23, (127 + 32) << 23  # the bit patterns of 2^-32 and 2^32


def weight_ok(u):
    """The conditions of a valid weight, on its bit pattern: zero of either sign, or a finite
    normal number of magnitude 2^-32 to 2^32."""
    a = u & 0x7FFFFFFF
    if a == 0:
        return True
    if a >= 0x7F800000:  # infinity and NaN
        return False
    return 2.0 ** -32 <= abs(f32(u)) <= 2.0 ** 32


def matrix_ok(C, K, fmt, null, weights):
    if null or not 1 <= C <= 8 or not 1 <= K <= 8 or fmt not in (F32, F16, BF16):
        return False
    return all(weight_ok(u) for u in weights[:K * C])


def test_validity(exe, tmp_path):
    one = bits_of(1.0)
    single = [0, 0x80000000, LO, LO - 1, LO + 1, HI, HI + 1, HI - 1, LO | 0x80000000, (LO - 1) | 0x80000000,
              HI | 0x80000000, (HI + 1) | 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,
              1, 0x007FFFFF, 0x80000001, 0x00800000, 0x7F7FFFFF, one, bits_of(-0.5), bits_of(1 / 3)]
    cases = []
    for u in single:
        for fmt in (F32, F16, BF16):
            cases.append((1, 1, fmt, 0, [u]))
        cases.append((8, 8, F32, 0, [one] * 63 + [u]))      # the last weight of the largest matrix
        cases.append((3, 2, BF16, 0, [one, u, one, 0, one, one]))
        cases.append((2, 1, F32, 0, [one, one, u]))          # a weight past K * C does not count
    for C in (0, 1, 8, 9):
        for K in (0, 1, 8, 9):
            cases.append((C, K, F32, 0, [one] * 64))
    for fmt in (I32, F32, F16, BF16, 4, 0xFFFFFFFF):
        cases.append((2, 2, fmt, 0, [one] * 4))
    cases.append((2, 2, F32, 1, [one] * 4))                  # no weights at all
    blob = b"".join(struct.pack("<68I", C, K, fmt, null, *(w + [0] * 64)[:64]) for C, K, fmt, null, w in cases)
    src = os.path.join(str(tmp_path), "valid.bin")
    with open(src, "wb") as f:
        f.write(blob)
    got = run(exe, ["valid", src])["valid"]
    want = [int(matrix_ok(*c)) for c in cases]
    assert got == want
    assert 0 < sum(want) < len(want)
    by = {(c[0], c[1], c[2], c[4][0] if len(c[4]) == 1 else None): w for c, w in zip(cases, want)}
    assert by[(1, 1, F32, LO)] == 1 and by[(1, 1, F32, LO - 1)] == 0 and by[(1, 1, F32, HI)] == 1 and by[(1, 1, F32, HI + 1)] == 0
    assert by[(1, 1, F32, 0x80000000)] == 1 and by[(1, 1, F32, 1)] == 0 and by[(1, 1, F32, 0x7FC00000)] == 0


# ---- elements ------------------------------------------------------------------------------------
def mixw(exe, tmp_path, x, bits, W, tag):
    """The program's (f32, f16, bf16) bit patterns [n, K] for the samples x [n, C] under W [K, C]."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    K, C = W.shape
    assert x.shape[1] == C
    base = os.path.join(str(tmp_path), f"{tag}_{bits}_{C}_{K}")
    W.astype("<f4").tofile(base + ".w")
    x.astype("<i4").tofile(base + ".in")
    assert run(exe, ["elements", bits, C, K, base + ".w", base + ".in", base + ".out"])["count"] == len(x)
    rec = np.fromfile(base + ".out", dtype=np.dtype([("f32", "<u4"), ("f16", "<u2"), ("bf16", "<u2")])).reshape(len(x), K)
    return rec["f32"], rec["f16"], rec["bf16"]


def check(exe, tmp_path, x, bits, W, tag):
    got = mixw(exe, tmp_path, x, bits, W, tag)
    want = mixw_ref.narrow(mixw_ref.mix(x, bits, W))
    for name, g, w in zip(("f32", "f16", "bf16"), got, want):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (tag, bits, name, [(x[i].tolist(), int(k), hex(int(g[i, k])), hex(int(w[i, k]))) for i, k in bad[:5]])
    return got


def test_every_pair_of_8_bit_values_mid_and_side(exe, tmp_path):
    a = np.arange(-128, 128, dtype=np.int64)
    x = np.stack([np.repeat(a, 256), np.tile(a, 256)], axis=1)
    got = check(exe, tmp_path, x, 8, [[0.5, 0.5], [0.5, -0.5]], "pairs")
    assert got[0][0, 0] == 0xBF800000 and got[0][0, 1] == 0  # -128, -128: mid exactly -1.0, side +0.0f
    assert (got[0][x[:, 0] == x[:, 1], 1] == 0).all()        # a cancellation is +0.0f, never -0.0f


def itu_rows(C):
    """The unnormalised ITU rows of C channels in double, divided by their own sums: the formula of
    the issue, written out here."""
    a = math.sqrt(0.5)
    left = {3: [1, 0, a], 4: [1, 0, a, 0], 5: [1, 0, a, a, 0], 6: [1, 0, a, 0, a, 0], 7: [1, 0, a, 0, 0.5, a, 0],
            8: [1, 0, a, 0, a, 0, a, 0]}[C]
    right = {3: [0, 1, a], 4: [0, 1, 0, a], 5: [0, 1, a, 0, a], 6: [0, 1, a, 0, 0, a], 7: [0, 1, a, 0, 0.5, 0, a],
             8: [0, 1, a, 0, 0, a, 0, a]}[C]
    both = [l + r for l, r in zip(left, right)]
    return [np.array([v / sum(row) for v in row], dtype=np.float64).astype(np.float32) for row in (left, right, both)]


def directed_weights(C):
    """The rows of the directed set for C channels (each a float32 [C])."""
    rows = []
    if C >= 2:
        rows.append([1.0, -1.0] + [0.0] * (C - 2))
        rows.append([0.5, 0.5] + [0.0] * (C - 2))
        rows.append([0.0] * (C - 2) + [0.5, -0.5])
    rows.append([2.0 ** -32] * C)
    rows.append([2.0 ** 32] * C)
    rows.append([2.0 ** 32 if c % 2 == 0 else -(2.0 ** 32) for c in range(C)])
    rows.append([2.0 ** -32 if c % 2 else 2.0 ** 32 for c in range(C)])
    for d in (3, 5, 6, 7):
        rows.append([np.float32(1.0 / d)] * C)
    rows.append([np.float32(1.0 / C)] * C)
    rows.append([0.0] * C)
    rows.append([-0.0] * (C - 1) + [1.0])
    if C >= 3:
        rows += [r.tolist() for r in itu_rows(C)]
    return [np.array(r, dtype=np.float32) for r in rows]


def directed_samples(bits, C):
    """Tuples of C samples of `bits` bits: the limits, equal samples, and tuples whose sums are the
    directed sums of test_mix_host (the ties of the int -> float rounding among them)."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = random.Random(f"mixw{bits}x{C}")
    rows = [[lo] * C, [hi] * C, [0] * C, [lo, hi] * (C // 2) + [lo] * (C % 2), [1] * C, [-1] * C]
    for v in (lo, hi, lo + 1, hi - 1, 12345 % hi, -(54321 % hi)):
        rows.append([v] * C)  # equal samples: {1, -1} must cancel to +0.0f
    for s in directed_sums(bits, C)[::3]:
        rows.append(split(s, C, lo, hi, rng))
    if bits == 32:  # every channel itself on a tie of the int32 -> float rounding, and next to it
        for k in range(24, 31):
            half = 1 << (k - 24)
            for odd in (0, 2 * half):
                for d in (-1, 0, 1):
                    for sign in (1, -1):
                        v = sign * ((1 << k) + odd + half + d)
                        rows.append([v] * C)
                        rows.append([v if c % 2 == 0 else rng.randint(lo, hi) for c in range(C)])
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_chains_over_a_directed_set_and_seeded_tuples(exe, tmp_path, bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    for C in range(1, 9):
        x = directed_samples(bits, C)
        rows = directed_weights(C)
        for k0 in range(0, len(rows), 8):  # the program takes up to 8 rows a run
            W = np.stack(rows[k0:k0 + 8])
            got = check(exe, tmp_path, x, bits, W, f"dir{k0}")
            if k0 == 0 and C >= 2:  # row 0 is {1, -1, 0...}: equal samples cancel to bit pattern 0
                equal = (x[:, 0] == x[:, 1])
                assert equal.sum() >= 10 and (got[0][equal, 0] == 0).all() and (got[1][equal, 0] == 0).all()
        # 10^5 seeded tuples over the eight channel counts of this depth, under seeded weights of every magnitude
        rng = np.random.default_rng([bits, C])
        n = 12500
        xs = rng.integers(lo, hi + 1, size=(n, C), dtype=np.int64)
        expo = rng.integers(-32, 32, size=(8, C))
        W = (rng.uniform(1.0, 2.0, size=(8, C)) * np.exp2(expo) * rng.choice([-1.0, 1.0], size=(8, C))).astype(np.float32)
        W[rng.random(size=(8, C)) < 0.15] = 0.0
        W = np.clip(W, -2.0 ** 32, 2.0 ** 32)
        check(exe, tmp_path, xs, bits, W, "seeded")


def test_reference_chain_against_exact_rational_arithmetic():
    """mixw_ref.mix equals the Fraction chain on a sample of the directed set."""
    for bits in (8, 32):
        for C in (2, 3, 6, 8):
            x = directed_samples(bits, C)[:40]
            for w in directed_weights(C):
                got = mixw_ref.mix(x, bits, w[None, :])[:, 0]
                want = np.array([mixw_ref.mix_exact(r, bits, w) for r in x], dtype=np.float32)
                assert (got.view(np.uint32) == want.view(np.uint32)).all(), (bits, C, w)


def test_equivalences_with_the_existing_rules(exe):
    # 4 depths x 8 channel counts x 4000 samples x C unit rows x 3 formats, and 708^2 pairs x 3 formats
    assert run(exe, ["equiv"])["checked"] == 4 * 4000 * sum(range(1, 9)) * 3 + 708 * 708 * 3


def test_tile_rows_against_the_rule_element_by_element(exe):
    # f32: 4 alignments; f16 and bf16: 8; 41 lengths, 4 source and 3 output channel counts, 4 flag sets each
    assert run(exe, ["rows"])["cases"] == (4 + 8 + 8) * 41 * 4 * 3 * 4
