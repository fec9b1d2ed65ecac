"""The scalar rules of turning tensor elements into the encoder's PCM
(zig-flac_amd/csrc/fg_quantize.hpp) on the host, under AddressSanitizer and UBSan, through the
stand-alone program tests/cpp/quantize_host_main.cpp.  No GPU.

`sample`: element -> sample against numpy in float64, clip(rint(float64(x) * 2^(bits-1)), lo, hi) with
NaN giving 0, and the clipped flags against numpy's: for 24 and 32 bits a directed set (every tie
around the powers of two, the limits, infinities, NaN, zeros, subnormals) plus 10^5 seeded random
values, in f32; the f16 and bf16 widening over all 65536 patterns; int32 inside and outside every
depth.  `roundtrip`: every sample of 8 and 16 (and 24) bits through deliver::element and back.
`rows`: the kernel's own PCM writer in a guarded buffer against sample-by-sample int.to_bytes.
Bit patterns are compared; every step of the rule is exact, so no tolerance."""
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
I32, F32, F16, BF16 = range(4)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("quantizehost")), "quantize_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "quantize_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def as_f64(patterns, fmt):
    """The values of the elements `patterns` (u32; 16-bit ones in the low half) as float64."""
    p = np.asarray(patterns, dtype=np.uint32)
    if fmt == F32:
        return p.view(np.float32).astype(np.float64)
    if fmt == F16:
        return p.astype(np.uint16).view(np.float16).astype(np.float64)
    if fmt == BF16:
        return (p << np.uint32(16)).view(np.float32).astype(np.float64)
    return p.view(np.int32).astype(np.float64)


def expected(patterns, fmt, bits):
    """(samples, clipped flags) by the rule in float64."""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    with np.errstate(all="ignore"):  # signalling NaNs, infinities
        x = as_f64(patterns, fmt)
        r = np.rint(x * (1.0 if fmt == I32 else 2.0 ** (bits - 1)))
    nan = np.isnan(x)
    clipped = nan | (r < lo) | (r > hi)
    s = np.where(nan, 0.0, np.clip(np.where(nan, 0.0, r), lo, hi)).astype(np.int64)
    return s, clipped


def quantize(exe, tmp_path, patterns, fmt, bits):
    src, dst = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    np.asarray(patterns, dtype="<u4").tofile(src)
    res = run(exe, ["sample", bits, fmt, src, dst])
    assert res["count"] == len(patterns)
    rec = np.fromfile(dst, dtype=np.dtype([("s", "<i4"), ("clipped", "<u4")]))
    assert res["clipped"] == int(rec["clipped"].sum())
    return rec["s"].astype(np.int64), rec["clipped"].astype(bool)


def check(exe, tmp_path, patterns, fmt, bits):
    got_s, got_c = quantize(exe, tmp_path, patterns, fmt, bits)
    want_s, want_c = expected(patterns, fmt, bits)
    bad = np.nonzero((got_s != want_s) | (got_c != want_c))[0]
    assert len(bad) == 0, [(hex(int(patterns[i])), int(got_s[i]), int(want_s[i]), bool(got_c[i]), bool(want_c[i])) for i in bad[:5]]
    return want_s, want_c


def directed_f32(bits):
    unit = 2.0 ** -(bits - 1)
    v = []
    for j in range(0, 23):  # k + 0.5 has at most 24 significant bits: every tie is an f32
        for d in (-2, -1, 0, 1, 2):  # above even and above odd k
            k = (1 << j) + d
            if k >= 0:
                v += [(k + 0.5) * unit, -(k + 0.5) * unit]
    one = np.float32(1.0)
    below = float(np.nextafter(one, np.float32(0.0)))
    above = float(np.nextafter(one, np.float32(2.0)))
    v += [1.0, -1.0, below, -below, above, -above, 2.0 ** 31, -(2.0 ** 31), float("inf"), float("-inf"), float("nan"), 0.0, -0.0,
          1.0 - unit, -1.0 - unit, 1.0 - unit / 2, -1.0 - unit / 2, unit, -unit, unit / 2, -unit / 2, unit / 4, 1.5 * unit,
          float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny),
          1e-45, -1e-45, 1e-40, -1e-40, 0.5, -0.5, 2.0 ** 24 * unit, (2.0 ** 24 + 2) * unit]
    x = np.array(v, dtype=np.float64).astype(np.float32)
    rng = np.random.default_rng(1000 + bits)
    near = (rng.random(50000) * 2.2 - 1.1).astype(np.float32)
    raw = rng.integers(0, 1 << 32, 50000, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([x.view(np.uint32), near.view(np.uint32), raw])


@pytest.mark.parametrize("bits", [24, 32])
def test_the_rule_over_a_directed_set_of_f32(exe, tmp_path, bits):
    p = directed_f32(bits)
    assert len(p) >= 100000
    s, c = check(exe, tmp_path, p, F32, bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assert s.min() == lo and s.max() == hi and c.sum() > 1000 and (~c).sum() > 1000
    x = p.view(np.float32)
    one = np.nonzero(x == np.float32(1.0))[0][0]
    assert s[one] == hi and c[one]  # 1.0 is clipped: a delivery only produces [-1, 1)
    minus = np.nonzero(x == np.float32(-1.0))[0][0]
    assert s[minus] == lo and not c[minus]
    nan = np.nonzero(np.isnan(x))[0]
    assert len(nan) > 0 and (s[nan] == 0).all() and c[nan].all()
    zeros = np.nonzero(x == 0)[0]
    assert len(zeros) >= 2 and (s[zeros] == 0).all() and not c[zeros].any()
    # ties went to the even neighbour: (k + 0.5) units gives k for even k, k + 1 for odd
    unit = 2.0 ** -(bits - 1)
    for k in (2, 3, 1024, 1025):
        i = np.nonzero(x == np.float32((k + 0.5) * unit))[0][0]
        assert s[i] == (k if k % 2 == 0 else k + 1)


@pytest.mark.parametrize("bits", [8, 16])
def test_the_rule_over_f32_around_every_sample(exe, tmp_path, bits):
    """Every sample value of the depth, with a quarter, a half and three quarters of a unit added."""
    k = np.arange(-(1 << (bits - 1)) - 2, (1 << (bits - 1)) + 2, dtype=np.float64)
    x = np.concatenate([(k + f) * 2.0 ** -(bits - 1) for f in (0.0, 0.25, 0.5, 0.75)]).astype(np.float32)
    s, c = check(exe, tmp_path, x.view(np.uint32), F32, bits)
    assert c.sum() > 0 and s.min() == -(1 << (bits - 1)) and s.max() == (1 << (bits - 1)) - 1


@pytest.mark.parametrize("fmt", [F16, BF16])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_the_rule_over_every_16_bit_element(exe, tmp_path, fmt, bits):
    """All 65536 patterns of f16 and of bf16: subnormals, infinities and NaNs of the widening included."""
    p = np.arange(1 << 16, dtype=np.uint32)
    s, c = check(exe, tmp_path, p, fmt, bits)
    assert c.sum() > 0 and (s != 0).sum() > 0


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_int32_elements_inside_and_outside_the_depth(exe, tmp_path, bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = np.random.default_rng(bits)
    v = [0, 1, -1, lo, hi, lo + 1, hi - 1, -(1 << 31), (1 << 31) - 1]
    if bits < 32:
        v += [lo - 1, hi + 1, lo * 2, hi * 2 + 1]
    x = np.concatenate([np.array(v, dtype=np.int64), rng.integers(-(1 << 31), 1 << 31, 20000),
                        rng.integers(lo, hi + 1, 20000)]).astype(np.int32)
    s, c = check(exe, tmp_path, x.view(np.uint32), I32, bits)
    assert (c.sum() > 0) == (bits < 32)
    assert (s[~c] == x[~c]).all()


@pytest.mark.parametrize("bits,fmt", [(8, F32), (16, F32), (8, F16), (8, BF16), (8, I32), (16, I32), (24, I32), (24, F32)])
def test_every_sample_comes_back_through_the_delivery(exe, bits, fmt):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    res = run(exe, ["roundtrip", bits, fmt, lo, hi, 1])
    assert res == {"count": 1 << bits, "bad": 0}


def test_int32_comes_back_at_32_bits(exe):
    lo, hi = -(1 << 31), (1 << 31) - 1
    res = run(exe, ["roundtrip", 32, I32, lo, hi, 65521])
    assert res["bad"] == 0 and res["count"] > 65536
    for first, last in ((lo, lo + 100000), (hi - 100000, hi), (-100000, 100000)):
        assert run(exe, ["roundtrip", 32, I32, first, last, 1])["bad"] == 0


def test_16_bit_floats_do_not_hold_every_16_bit_sample(exe):
    """The converse, so that `bad` is seen to count: f16 and bf16 keep 11 and 8 significant bits."""
    for fmt in (F16, BF16):
        assert run(exe, ["roundtrip", 16, fmt, -32768, 32767, 1])["bad"] > 0


LENGTHS = (1, 2, 3, 4, 5, 17, 4097)
GUARD = 64


def test_the_pcm_writer_against_int_to_bytes(exe, tmp_path):
    rng = np.random.default_rng(7)
    pool = rng.integers(-(1 << 31), 1 << 31, 8 * (4097 + 5), dtype=np.int64).astype(np.int32)
    cases = [(C, B, T, planar, T + 5 if planar else T) for C in (1, 2, 3, 8) for B in (1, 2, 3, 4) for T in LENGTHS
             for planar in (1, 0)]
    assert {(T * C * B) % 4 for C, B, T, _, _ in cases} == {0, 1, 2, 3}
    for B in (1, 2, 3, 4):  # one run a depth: the pool's values are shifted into its range
        mine = [c for c in cases if c[1] == B]
        vals = pool >> (32 - 8 * B)
        src, dst = os.path.join(str(tmp_path), f"pool{B}.bin"), os.path.join(str(tmp_path), f"rows{B}.bin")
        vals.astype("<i4").tofile(src)
        res = run(exe, ["rows", I32, src, dst] + [v for c in mine for v in c])
        assert res["cases"] == len(mine) and res["clipped"] == [0] * len(mine)
        with open(dst, "rb") as f:
            blob = f.read()
        at = 0
        for C, _, T, planar, stride in mine:
            length = T * C * B
            span = (length + 3) // 4 * 4
            buf = blob[at:at + 2 * GUARD + span]
            at += 2 * GUARD + span
            assert buf[:GUARD] == b"\xA5" * GUARD and buf[GUARD + span:] == b"\xA5" * GUARD, (C, B, T, planar)
            want = b"".join(int(vals[c * stride + t] if planar else vals[t * C + c]).to_bytes(B, "little", signed=True)
                            for t in range(T) for c in range(C))
            assert buf[GUARD:GUARD + length] == want, (C, B, T, planar)
            assert buf[GUARD + length:GUARD + span] == bytes(span - length), (C, B, T, planar)
        assert at == len(blob)


def test_the_pcm_writer_counts_clipped_elements(exe, tmp_path):
    x = np.array([1.0, 0.5, -1.0, np.nan, -1.5, 0.25, 1.0, 0.0, 0.999], dtype=np.float32)
    src, dst = os.path.join(str(tmp_path), "clip.bin"), os.path.join(str(tmp_path), "clipout.bin")
    x.view(np.uint32).astype("<u4").tofile(src)
    res = run(exe, ["rows", F32, src, dst, 1, 2, 9, 1, 9, 3, 2, 3, 0, 3])
    assert res["clipped"] == [4, 4]
    want, _ = expected(x.view(np.uint32), F32, 16)
    with open(dst, "rb") as f:
        blob = f.read()
    assert np.frombuffer(blob[GUARD:GUARD + 18], dtype="<i2").tolist() == want.tolist()
