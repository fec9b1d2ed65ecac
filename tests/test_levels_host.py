"""The scalar rules of the level measurement (zig-flac_amd/csrc/fg_levels.hpp) on the host, under
AddressSanitizer and UBSan, through the stand-alone program tests/cpp/levels_host_main.cpp.  No GPU,
and nothing is loaded into python.

`f64`: u128_to_f64 against Python's float(int), which is correctly rounded to nearest-even, over a
directed set (every bit length 1..93; one below, at and one above a tie at each length, above an
even and above an odd mantissa; all-ones; the values around 2^64) plus 10^5 seeded random 93-bit
values.  `acc`: acc_add and acc_merge on the worst cases against Python integers.  `geom`: the
blocks and the tiles of a window against a plain statement.  `tile`: the kernel's own tile reader
and its three reduction modes in heap blocks of exactly the words it may read.  Bit patterns are
compared; every step is exact, so there is no tolerance."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LANES, WAVES, PARTS = 0, 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("levelshost")), "levels_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "levels_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def f64_bits(v: int) -> int:
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def directed():
    v = [0, 1, 2, 3, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, (1 << 93) - 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1]
    for L in range(1, 94):
        v += [1 << (L - 1), (1 << L) - 1]  # the smallest and the largest (all ones) of the length
        if L >= 55:
            half = 1 << (L - 54)  # half a unit of the 53-bit mantissa at this length
            for m in ((1 << 52), (1 << 52) + 1, (1 << 53) - 2, (1 << 53) - 1, (1 << 52) + 0x5A5A5A5A5A5A4, (1 << 52) + 0x5A5A5A5A5A5A5):
                tie = (m << (L - 53)) + half  # above an even m and above an odd m
                v += [tie - 1, tie, tie + 1]
    return v


def test_u128_to_f64_against_python_float(exe, tmp_path):
    rng = np.random.default_rng(93)
    rand = [(int(h) << 64) | int(l) for h, l in zip(rng.integers(0, 1 << 29, 100000, dtype=np.uint64),
                                                     rng.integers(0, 1 << 64, 100000, dtype=np.uint64))]
    vals = directed() + rand
    assert {v.bit_length() for v in vals} >= set(range(1, 94)) and len(rand) == 100000
    src, dst = os.path.join(str(tmp_path), "u128.bin"), os.path.join(str(tmp_path), "f64.bin")
    pairs = np.array([[v & ((1 << 64) - 1), v >> 64] for v in vals], dtype="<u8")
    pairs.tofile(src)
    assert run(exe, ["f64", src, dst])["count"] == len(vals)
    got = np.fromfile(dst, dtype="<u8")
    want = np.array([f64_bits(v) for v in vals], dtype=np.uint64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(hex(vals[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    # the set holds what it claims: ties that round down (even) and up (odd), and inexact values on both sides of 2^64
    inexact = [v for v in vals if int(float(v)) != v]
    assert any(v < 1 << 64 for v in inexact) and any(v >= 1 << 64 for v in inexact)
    tie = ((1 << 52) << 11) + (1 << 10)
    assert float(tie) == float((1 << 52) << 11) and float(tie + (1 << 11)) == float(((1 << 52) + 2) << 11)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n,split", [(1, 1), (4, 1), (8, 3), (1000, 64), (100000, 256), (100001, 7)])
def test_accumulate_and_merge_on_the_worst_cases(exe, kind, n, split):
    res = run(exe, ["acc", kind, n, split])
    x = [(2 ** 31 - 1) if (kind == 1 and t % 2) else -2 ** 31 for t in range(n)]
    e = sum(v * v for v in x)
    assert res["peak"] == 2 ** 31 and res["sum"] == sum(x)
    assert (int(res["e_hi"]) << 64) | int(res["e_lo"]) == e
    assert int(res["energy"]) == f64_bits(e)
    if n >= (4 if kind == 0 else 8):
        assert e >= 1 << 64  # four squares of -2^31 are 2^64: the sum has left 64 bits


def plain_tiles(n, hop, T):
    """[(t0, ns, block0, part)] by the statement in fg_levels.hpp."""
    out = []
    blocks = (n + hop - 1) // hop
    if hop >= T:
        for j in range(blocks):
            length = min(hop, n - j * hop)
            for p in range((length + T - 1) // T):
                out.append([j * hop + p * T, min(T, length - p * T), j, p])
    else:
        g = T // hop
        for b0 in range(0, blocks, g):
            out.append([b0 * hop, min(g * hop, n - b0 * hop), b0, 0])
    return out


@pytest.mark.parametrize("per", [1, 4, 9, 32])
def test_blocks_and_tiles(exe, per):
    T = 4096 // per
    hops = sorted({1, 3, 63, 64, T - 1, T, T + 1, 2 * T + 1, 100000})
    for hop in hops:
        for n in sorted({0, 1, hop, hop + 1, 3 * hop - 1, 5 * T + 3}):
            g = run(exe, ["geom", n, hop, per])
            blocks = (n + hop - 1) // hop
            assert g["blocks"] == blocks and g["T"] == T, (n, hop)
            assert g["mode"] == (PARTS if hop >= T else LANES if hop < 64 else WAVES)
            assert g["parts"] == ((hop + T - 1) // T if hop >= T else 1) and g["group"] == (1 if hop >= T else T // hop)
            assert g["last"] == (n - (blocks - 1) * hop if blocks else 0)
            assert g["partials"] == (blocks * g["parts"] * 3 if g["parts"] > 1 else 0)
            assert g["too_small_at"] == [0, 1 if blocks else 0]
            assert g["tiles"] == plain_tiles(n, hop, T), (n, hop)
            at = 0  # the tiles cut [0, n) in order, none longer than T, none across a block edge it does not hold whole
            for t0, ns, b0, part in g["tiles"]:
                assert t0 == at and 0 < ns <= T
                at += ns
                if hop >= T:
                    assert t0 // hop == (t0 + ns - 1) // hop == b0
                else:
                    assert t0 % hop == 0 and (ns % hop == 0 or at == n)
            assert at == n


def reference(x, hop):
    """(peak, sum, energy bits) [blocks, C] of int64 samples x [n, C], by Python integers."""
    n, C = x.shape
    blocks = (n + hop - 1) // hop
    peak, total, energy = np.zeros((blocks, C), np.uint32), np.zeros((blocks, C), np.int64), np.zeros((blocks, C), np.uint64)
    for j in range(blocks):
        blk = x[j * hop:(j + 1) * hop]
        for c in range(C):
            col = [int(v) for v in blk[:, c]]
            peak[j, c] = max(abs(v) for v in col)
            total[j, c] = sum(col)
            energy[j, c] = f64_bits(sum(v * v for v in col))
    return peak, total, energy


REC = np.dtype([("peak", "<u4"), ("pad", "<u4"), ("sum", "<i8"), ("energy", "<u8")])


@pytest.mark.parametrize("B,C", [(1, 1), (2, 2), (3, 3), (4, 8), (3, 2), (1, 3)])
def test_the_tile_reader_in_exact_heap_blocks(exe, tmp_path, B, C):
    bits, per = 8 * B, B * C
    T = 4096 // per
    rng = np.random.default_rng([B, C])
    n = 2 * T + 37
    x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(n, C), dtype=np.int64)
    x[5:40] = -(1 << (bits - 1))
    x[40:60:2] = (1 << (bits - 1)) - 1
    src, dst = os.path.join(str(tmp_path), "x.bin"), os.path.join(str(tmp_path), "rec.bin")
    x.astype("<i4").tofile(src)
    modes = set()
    for k, hop in enumerate((1, 3, 64, 65, T - 1, T, T + 1, 2 * T + 36, n, n + 5)):
        peak, total, energy = reference(x, hop)
        for lead in {k % 8, (k + 3) % 8}:
            res = run(exe, ["tile", src, dst, B, C, n, hop, lead])
            modes.add(res["mode"])
            rec = np.fromfile(dst, dtype=REC).reshape(-1, C)
            assert res["records"] == peak.size and (rec["peak"] == peak).all() and (rec["sum"] == total).all(), (hop, lead)
            assert (rec["energy"] == energy).all(), (hop, lead)
    assert modes == {LANES, WAVES, PARTS}
