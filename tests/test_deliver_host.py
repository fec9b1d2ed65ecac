"""The scalar rules of the delivery of sample windows as tensor elements
(zig-flac_amd/csrc/fg_deliver.hpp) on the host, under AddressSanitizer and UBSan, through the
stand-alone program tests/cpp/deliver_host_main.cpp.  No GPU.

`sample`: the sample load at every byte alignment for 1 to 4 bytes, against int.from_bytes.
`convert`: int -> f32 -> f16 / bf16 as bit patterns against numpy (f32, f16) and torch on the CPU
(bf16): all 16-bit and 8-bit values, and for 24 and 32 bits a directed set (the ties of every
conversion, the limits, the f16 subnormal range) plus 10^5 seeded random values.  `capacity`: the
capacity rule against Python integers.  `rows`: the row plan, filled by the kernel's own fill_row_slot, against the
element-by-element conversion in a guarded buffer.  Bit patterns are compared; no tolerance."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("deliverhost")), "deliver_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "deliver_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def test_sample_load_at_every_alignment(exe):
    pat = bytes((i * 73 + 0x85) & 0xFF for i in range(32))
    assert any(b & 0x80 for b in pat) and any(not b & 0x80 for b in pat)  # both signs occur
    got = run(exe, ["sample", pat.hex()])["samples"]
    for B in (1, 2, 3, 4):
        want = [int.from_bytes(pat[al:al + B], "little", signed=True) for al in range(16)]
        assert got[B - 1] == want, B
        assert min(want) < 0 < max(want)


def expected(x, bits):
    """(f32, f16, bf16) bit patterns of the int32 array x by numpy and torch-CPU."""
    import torch

    f32 = x.astype(np.float32) * np.float32(2.0 ** -(bits - 1))
    f16 = f32.astype(np.float16)
    bf16 = torch.from_numpy(f32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return f32.view(np.uint32), f16.view(np.uint16), bf16


def convert(exe, tmp_path, x, bits):
    src, dst = os.path.join(str(tmp_path), f"in{bits}.bin"), os.path.join(str(tmp_path), f"out{bits}.bin")
    x.astype("<i4").tofile(src)
    assert run(exe, ["convert", bits, src, dst])["count"] == len(x)
    rec = np.fromfile(dst, dtype=np.dtype([("f32", "<u4"), ("f16", "<u2"), ("bf16", "<u2")]))
    return rec["f32"], rec["f16"], rec["bf16"]


def directed(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = {0, 1, -1, lo, hi, lo + 1, hi - 1}
    for k in range(8, 31):  # around every power of two: the ties and near-ties of the three roundings
        for half in {1 << max(k - 24, 0), 1 << max(k - 11, 0), 1 << max(k - 8, 0)}:  # half an ulp of f32 / f16 / bf16 at 2^k
            for odd in (0, 2 * half):  # the tie above an even and above an odd significand
                for d in (-1, 0, 1):
                    for sign in (1, -1):
                        v.add(sign * ((1 << k) + odd + half + d))
        v.update({(1 << k) - 1, (1 << k) + 1, -(1 << k) - 1, -(1 << k) + 1, 1 << k, -(1 << k)})
    v.update({(1 << 24) + 1, (1 << 24) - 1, -(1 << 24) - 1, -(1 << 24) + 1})
    # the f16 subnormal range, |value| < 2^-14, and the ties below its unit 2^-24
    sub = 1 << max(bits - 1 - 14, 0)
    step = max(sub // 1024, 1)
    v.update(range(-sub - 3 * step, sub + 3 * step + 1, step))
    v.update(range(-1100, 1101))
    rng = random.Random(f"deliver{bits}")
    v.update(rng.randint(lo, hi) for _ in range(100000))
    return np.array(sorted(t for t in v if lo <= t <= hi), dtype=np.int64).astype(np.int32)


def properties(x, bits):
    """What the input set exercises -> (inexact int->f32, f16 ties, bf16 ties, f16 subnormal results)."""
    f32, f16, _ = expected(x, bits)
    inexact = int((x.astype(np.float32).astype(np.float64) != x.astype(np.float64)).sum())
    normal16 = ((f32 >> 23) & 0xFF) >= 113
    tie16 = int((normal16 & ((f32 & 0x1FFF) == 0x1000)).sum())
    tie_bf = int(((f32 & 0xFFFF) == 0x8000).sum())
    sub16 = int((((f16 & 0x7C00) == 0) & ((f16 & 0x3FF) != 0)).sum())
    return inexact, tie16, tie_bf, sub16


@pytest.mark.parametrize("bits", [8, 16])
def test_conversions_over_every_value(exe, tmp_path, bits):
    x = np.arange(-(1 << (bits - 1)), 1 << (bits - 1), dtype=np.int32)
    assert len(x) == 1 << bits
    for got, want in zip(convert(exe, tmp_path, x, bits), expected(x, bits)):
        assert (got == want).all()
    inexact, tie16, tie_bf, sub16 = properties(x, bits)
    assert inexact == 0
    if bits == 16:
        assert tie16 > 0 and tie_bf > 0 and sub16 > 0  # 16-bit audio reaches f16 subnormals: |x| < 2 gives 2^-15


@pytest.mark.parametrize("bits", [24, 32])
def test_conversions_over_a_directed_set(exe, tmp_path, bits):
    x = directed(bits)
    assert len(x) > 100000 and x.min() == -(1 << (bits - 1)) and x.max() == (1 << (bits - 1)) - 1
    inexact, tie16, tie_bf, sub16 = properties(x, bits)
    assert tie16 > 0 and tie_bf > 0 and sub16 > 0
    if bits == 32:
        assert inexact > 1000
        # exact ties of the int -> f32 rounding: half an ulp above a representable value
        assert {(1 << 24) + 1, (1 << 24) + 3, (1 << 30) + 64, -(1 << 24) - 1}.issubset(set(x.tolist()))
        # ties of the subnormal f16 rounding: odd multiples of half its unit, 2^-25 = 64 * 2^-31
        assert {64, 192, -64, -192}.issubset(set(x.tolist()))
    else:
        assert inexact == 0
    for name, got, want in zip(("f32", "f16", "bf16"), convert(exe, tmp_path, x, bits), expected(x, bits)):
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, [(int(x[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


def test_capacity_rule_against_python_integers(exe):
    cases = []
    for flags in (0, 1, 2, 3):
        for unit in (1, 2, 3, 8, 32):
            for n, count, cap in [(0, 0, 0), (0, 5, 0), (0, 5, 5 * unit - 1), (0, 5, 5 * unit), (3, 5, 3 * unit), (3, 5, 3 * unit - 1),
                                  (3, 5, 5 * unit), (3, 5, 5 * unit - 1), (7, U64, U64), (7, U64, 7 * unit), (7, U64, 7 * unit - 1),
                                  (0, U64, U64), (U64 // unit, U64 // unit, U64), (U64 // unit, U64 // unit, U64 - unit),
                                  (min(U64 // unit + 1, U64), U64, U64), ((1 << 63), (1 << 63), U64), (1, 1, 0), (0, 0, U64),
                                  (1 << 62, 1 << 62, (1 << 62) * unit % (1 << 64))]:
                cases.append((n, count, flags, cap, unit))
    got = run(exe, ["capacity"] + [v for c in cases for v in c])["too_small"]
    assert all(0 <= v <= U64 for c in cases for v in c)
    want = [int((count if flags & 3 else n) * unit > cap) for n, count, flags, cap, unit in cases]
    assert got == want
    assert 0 in want and 1 in want
    assert any(count * unit > U64 for _, count, flags, _, unit in cases if flags)  # a product that would wrap


def test_row_plan_against_the_plain_conversion(exe):
    # i32 and f32: 4 alignments; f16 and bf16: 8; 41 lengths each
    assert run(exe, ["rows"])["cases"] == (4 + 4 + 8 + 8) * 41
