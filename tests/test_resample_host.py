"""The resampling rule of the delivery of sample windows (zig-flac_amd/csrc/fg_resample.hpp) on the
host, under AddressSanitizer and UBSan, through the stand-alone program
tests/cpp/resample_host_main.cpp, against tests/resample_ref.py (numpy float64).  No GPU.

`table`: every coefficient of six ratios within one float rounding of the formula
(|h - h64| <= 2^-24 |h64| + 1e-12), row sums within T * 2^-24 of 1.  `samples`: the sample rule
against a float64 sum over the same float table, under the bound of a length-T recursive fma sum
computed per output; inside the program the same outputs tile by tile through a skewed plane, as
the kernel does, bit for bit.  `grid`: validity, out_total, the delivered count and source_range
over all ordered pairs of the rate list and the edge cases.  `narrow`: f16 / bf16 of values up to 4
in magnitude against numpy and torch on the CPU.  `geometry`: the tile plan of every valid pair and
K = 1..8 against its formula and the 64 KiB of LDS.  The library's two host functions give the
program's table and outputs bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as ref  # noqa: E402

SIX = [(44100, 48000, 160, 147), (48000, 44100, 147, 160), (48000, 16000, 1, 3), (24000, 48000, 2, 1),
       (44100, 16000, 160, 441), (96000, 8000, 1, 12)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("resamplehost")), "resample_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "resample_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def tables(exe, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tables"))
    out = {}
    for src, dst, L, M in SIX:
        path = os.path.join(d, f"{src}_{dst}.bin")
        info = run(exe, ["table", src, dst, path])
        assert info["valid"] == 1 and (info["L"], info["M"]) == (L, M)
        out[(src, dst)] = (info, np.fromfile(path, dtype="<f4").reshape(info["L"], info["T"]))
    return out


# ---- the table -----------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst,L,M", SIX)
def test_table_against_the_formula(tables, src, dst, L, M):
    info, h = tables[(src, dst)]
    assert (info["L"], info["M"], info["Hw"], info["T"]) == ref.ratio(src, dst)
    assert info["T"] <= 576
    h64 = ref.table64(src, dst)
    assert h.shape == h64.shape
    err = np.abs(h.astype(np.float64) - h64)
    assert (err <= 2.0 ** -24 * np.abs(h64) + 1e-12).all(), float((err - 2.0 ** -24 * np.abs(h64)).max())
    assert (np.abs(h.astype(np.float64).sum(axis=1) - 1.0) <= info["T"] * 2.0 ** -24).all()


def test_tap_counts_of_the_two_documented_ratios(tables):
    assert tables[(44100, 48000)][0]["T"] == 48 and tables[(44100, 16000)][0]["T"] == 134
    assert tables[(96000, 8000)][0]["T"] == 576


def test_the_library_gives_the_same_table(tables):
    sys.path.insert(0, os.path.join(HERE, "..", "zig-flac_amd"))
    import flacgpu

    for (src, dst), (info, h) in tables.items():
        L, M, T, got = flacgpu.resample_filter(src, dst)
        assert (L, M, T) == (info["L"], info["M"], info["T"])
        assert got.dtype == np.float32 and (got.view(np.uint32) == h.view(np.uint32)).all()


# ---- the sample rule -----------------------------------------------------------------------------
def signal(total, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, total).astype(np.float32)
    if total > 40:  # the limits, and values a subnormal product comes from
        x[3], x[4], x[17], x[18] = 1.0, -1.0, np.float32(2.0 ** -120), np.float32(-2.0 ** -126)
    return x


def samples(exe, tmp_path, src, dst, x, start, count):
    a, b = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    x.astype("<f4").tofile(a)
    info = run(exe, ["samples", src, dst, start, count, a, b])
    y = np.fromfile(b, dtype="<f4")
    assert len(y) == info["n"]
    return y, info


@pytest.mark.parametrize("src,dst,L,M", SIX)
def test_sample_rule_against_float64(exe, tables, tmp_path, src, dst, L, M):
    info, h = tables[(src, dst)]
    Hw, T = info["Hw"], info["T"]
    cases = []
    for total in (0, 1, Hw - 1, Hw, 5000):
        ot = ref.out_total(total, L, M)
        for start in sorted({0, max(ot - 1, 0), ot, ot + 5}):
            cases.append((total, start, 0))
            cases.append((total, start, 64))
    cases.append((5000, 0, 1 << 63))  # the whole stream
    if ref.out_total(5000, L, M) <= 1024:  # more than one tile for every ratio
        cases.append((20000, 0, 1 << 63))
    cases.append((5000, 1234, 777))
    seen_tiles = 0
    for total, start, count in cases:
        x = signal(total, total + 1)
        y, run_info = samples(exe, tmp_path, src, dst, x, start, count)
        seen_tiles = max(seen_tiles, run_info["tiles"])
        y64, bound = ref.resample64(x, src, dst, start, count, h)
        assert len(y) == len(y64) == ref.delivered(total, L, M, start, count), (total, start, count)
        bad = np.nonzero(np.abs(y.astype(np.float64) - y64) > bound)[0]
        assert len(bad) == 0, (total, start, count, [(int(i), float(y[i]), float(y64[i]), float(bound[i])) for i in bad[:5]])
    assert seen_tiles > 1
    # the zero extension: the first output sees zeros before the stream, not a clamped or mirrored edge
    ones = np.ones(5000, dtype=np.float32)
    y, _ = samples(exe, tmp_path, src, dst, ones, 0, 1 << 63)
    assert abs(float(y[len(y) // 2]) - 1.0) < 1e-5 and 0.3 < float(y[0]) < 0.99


def test_the_library_gives_the_same_samples(exe, tmp_path):
    sys.path.insert(0, os.path.join(HERE, "..", "zig-flac_amd"))
    import flacgpu

    x = signal(5000, 7)
    for src, dst, L, M in SIX:
        for start, count in ((0, None), (1234, 777), (ref.out_total(5000, L, M) - 1, 5), (ref.out_total(5000, L, M), 5), (10, 0)):
            y, _ = samples(exe, tmp_path, src, dst, x, start, (1 << 63) if count is None else count)
            got = flacgpu.resample_f32_host(x, src, dst, start, count)
            assert got.dtype == np.float32 and len(got) == len(y)
            assert (got.view(np.uint32) == y.view(np.uint32)).all(), (src, dst, start, count)
    assert len(flacgpu.resample_f32_host(np.zeros(0, np.float32), 44100, 48000)) == 0


# ---- validity, totals and ranges -------------------------------------------------------------------
def test_grid_of_all_rate_pairs(exe):
    got = run(exe, ["grid"])
    pairs = {(p[0], p[1]): p[2:] for p in got["pairs"]}
    assert len(pairs) == len(ref.RATES) ** 2
    n_valid = 0
    for src in ref.RATES:
        for dst in ref.RATES:
            want = ref.ratio(src, dst)
            valid, L, M, Hw, T = pairs[(src, dst)]
            assert bool(valid) == (want is not None), (src, dst)
            if want:
                assert (L, M, Hw, T) == want and T <= 576
                n_valid += 1
    assert pairs[(44100, 44100)][0] == 0 and pairs[(192000, 8000)][0] == 0 and pairs[(8000, 192000)][0] == 1
    assert pairs[(96000, 8000)][0] == 1 and pairs[(176400, 11025)][0] == 0  # 1/12 is the last decimation served
    assert 100 < n_valid < 156
    rows = got["rows"]
    assert len(rows) == n_valid * 5 * 5 * 4
    kinds = set()
    for src, dst, total, start, count, ot, n, lo, hi in rows:
        L, M, Hw, T = ref.ratio(src, dst)
        assert ot == ref.out_total(total, L, M)
        assert n == ref.delivered(total, L, M, start, count)
        assert (lo, hi) == ref.source_range(total, L, M, Hw, start, n)
        assert lo <= hi <= total
        kinds.add((total in (0, 1, Hw - 1, Hw, 5000), start == 0, ot > 0 and start == ot - 1, start >= ot, count == 0))
    assert any(k[2] for k in kinds) and any(k[3] for k in kinds) and any(k[4] for k in kinds) and all(k[0] for k in kinds)


# ---- narrowing -------------------------------------------------------------------------------------
def test_narrowing_of_values_up_to_four(exe, tmp_path):
    import torch

    rng = np.random.RandomState(5)
    v = [rng.uniform(-4.0, 4.0, 200000).astype(np.float32), np.array([4.0, -4.0, 1.0, -1.0, 2.0, 3.9999998, 0.0], np.float32)]
    for e in range(-2, 2):  # around 2^e and 2^(e+1): the ties of both formats and their neighbours
        for mant_bits in (10, 7):
            ulp = 2.0 ** (e - mant_bits)
            base = 2.0 ** e + ulp * np.arange(0, 2 ** mant_bits + 1, dtype=np.float64)[: 600]
            for off in (0.5, 0.5 - 2.0 ** -12, 0.5 + 2.0 ** -12):
                v.append((base + off * ulp).astype(np.float32))
                v.append((-(base + off * ulp)).astype(np.float32))
        top = np.nextafter(np.float32(2.0 ** (e + 1)), np.float32(0))
        v.append(np.array([top, -top], np.float32))
    x = np.concatenate(v)
    x = x[np.abs(x) <= 4.0]  # a tie above the last power of two is out of the range
    assert np.abs(x).max() == 4.0 and len(x) > 210000
    a, b = os.path.join(str(tmp_path), "v.bin"), os.path.join(str(tmp_path), "n.bin")
    x.astype("<f4").tofile(a)
    assert run(exe, ["narrow", a, b])["count"] == len(x)
    rec = np.fromfile(b, dtype=np.dtype([("f16", "<u2"), ("bf16", "<u2")]))
    want16 = x.astype(np.float16).view(np.uint16)
    wantbf = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (rec["f16"] == want16).all() and (rec["bf16"] == wantbf).all()
    assert rec["f16"][0 + 200000] == 0x4400  # 4.0


# ---- geometry --------------------------------------------------------------------------------------
def test_tile_plans_fit_the_lds(exe):
    plans = run(exe, ["geometry"])["plans"]
    n_valid = sum(1 for s in ref.RATES for d in ref.RATES if ref.ratio(s, d))
    assert len(plans) == n_valid * 8
    skew = lambda i: i + (i >> 5)  # noqa: E731
    span_of = lambda tile, L, M, T: (tile - 1) * M // L + 1 + T  # noqa: E731
    for L, M, T, K, tile, span, plane, lds in plans:
        assert 1 <= tile <= 1024 and span == span_of(tile, L, M, T)
        assert plane == skew(span - 1) + 1 and lds == plane * 4 * K and lds <= 65536
        # the largest such tile
        assert tile == 1024 or (skew(span_of(tile + 1, L, M, T) - 1) + 1) * 4 * K > 65536
    assert min(p[4] for p in plans) >= 64 and max(p[7] for p in plans) > 60000
