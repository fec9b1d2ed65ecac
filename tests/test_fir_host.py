"""The filter rule of the filtered delivery of sample windows (zig-flac_amd/csrc/fg_fir.hpp) on the
host, under AddressSanitizer and UBSan, through the stand-alone program tests/cpp/fir_host_main.cpp,
against tests/fir_ref.py (numpy float64, np.convolve over the zero-extended signal).  No GPU, and
nothing is loaded into python.

`rule`: every element within gamma_T sum |h[k] x[.]| of the float64 convolution (gamma_T = T u /
(1 - T u), u = 2^-24: a chain of T fused multiply-adds, one rounding each), +0.0f past the stream's
end, {1.0} the identity bit for bit.  `tile`: the same windows the way k_window_fir computes them --
the Toeplitz u to k mapping, the chunks of steps, the zero taps on both sides, the clip at the
stream's start -- through the kernel's own index functions in heap blocks of exactly the words it
may read, bit for bit against the rule.  `geometry`: fir_geometry over every T against its LDS bound,
and the layout's 64 banks.  `valid`, `span`: every refusal of a filter and the stage-1 span."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fir_ref as ref  # noqa: E402

TAPS = [1, 2, 15, 16, 17, 31, 33, 255, 256, 257, 4095, 4096]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("firhost")), "fir_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                           os.path.join(HERE, "cpp", "fir_host_main.cpp"), "-o", out])
    return out


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", f"sanitizer / program failure:\n{r.stdout[-500:]}\n{r.stderr[-2000:]}"
    return json.loads(r.stdout)


def window(exe, tmp, mode, x, h, d, start, count):
    px, ph, py = (os.path.join(str(tmp), n) for n in ("x.bin", "h.bin", "y.bin"))
    np.asarray(x, dtype="<f4").tofile(px)
    np.asarray(h, dtype="<f4").tofile(ph)
    res = run(exe, [mode, len(h), d, start, count, px, ph, py])
    return np.fromfile(py, dtype="<f4"), res


def windows_of(T, total):
    """At the start of the stream, across its end, wholly outside it (near and far), and inside."""
    inside = 2100 if T in (33, 257) else 200  # 2100: more than one tile of 2048
    return [(0, 300), (total - 100, 300), (total + 5, 50), (total + T + 10, 20), (T // 2 + 3, inside), (7, 0)]


@pytest.mark.parametrize("T", TAPS)
def test_rule_against_float64_and_the_kernels_indexing(exe, tmp_path, T):
    total = 2600 if T < 1000 else 5000
    x, h = ref.signal(total, T), ref.taps(T, T + 1)
    checked = 0
    for d in sorted({0, (T - 1) // 2, T - 1}):
        for start, count in windows_of(T, total):
            y, res = window(exe, tmp_path, "rule", x, h, d, start, count)
            y64, mag, n = ref.window64(x, h, d, start, count)
            assert res["n"] == n and len(y) == count
            err, bound = np.abs(y[:n].astype(np.float64) - y64), ref.gamma(T) * mag
            assert (err <= bound).all(), (T, d, start, float((err - bound).max()))
            assert (y[n:].view(np.uint32) == 0).all()  # +0.0f past the stream's end
            yt, rt = window(exe, tmp_path, "tile", x, h, d, start, count)
            assert rt["n"] == n and rt["differ"] == 0 and (yt.view(np.uint32) == y.view(np.uint32)).all(), (T, d, start)
            back = T - 1 - d
            assert rt["clip"] == (max(back - start, 0) if count else 0)
            assert rt["s_count"] == (count + T - 1 - rt["clip"] if count else 0)
            if n:
                assert rt["n_chunks"] == -(-((T + 15 + 3) // 4 * 4) // rt["chunk"]) and rt["chunk"] <= 256
            checked += n
    assert checked >= 600  # 300 + 100 + 200 elements a delay


def test_one_tap_of_one_is_the_identity(exe, tmp_path):
    x = ref.signal(500, 3, bits=24)
    x[10] = 0.0
    y, res = window(exe, tmp_path, "rule", x, [1.0], 0, 100, 600)
    assert res["n"] == 400 and (y[:400].view(np.uint32) == x[100:].view(np.uint32)).all() and (y[400:].view(np.uint32) == 0).all()
    yt, rt = window(exe, tmp_path, "tile", x, [1.0], 0, 100, 600)
    assert rt["differ"] == 0 and (yt.view(np.uint32) == y.view(np.uint32)).all()


def test_a_result_that_underflows_to_zero_is_plus_zero(exe, tmp_path):
    # 2^-149 * -2^-15 underflows to -0.0f in the chain, and a zero tap times a negative sample keeps it
    # there: the rule's last clause delivers +0.0f, from the chain and from the tile alike
    x = np.full(64, -2.0 ** -15, dtype=np.float32)
    h = np.array([2.0 ** -149, 0.0, 0.0], dtype=np.float32)
    for mode in ("rule", "tile"):
        y, res = window(exe, tmp_path, mode, x, h, 0, 8, 40)
        assert res["n"] == 40 and (y.view(np.uint32) == 0).all(), mode


def test_geometry_fits_its_lds_bound_for_every_filter(exe):
    # K does not enter: a (channel, tile) item stages one channel's span
    res = run(exe, ["geometry"])
    assert res["bad"] == 0 and res["conflicts"] == 0
    assert res["max_lds"] <= 16384 and res["max_chunk"] == 256 and res["tile"] == 2048
    assert res["edge"] == 241  # T = 241 fills one chunk of 256 steps, T = 242 needs a second


def test_filter_refusals(exe):
    def valid(offset=0, taps=16, delay=0, rows=1, reserved=0, K=2, taps_len=64):
        return run(exe, ["valid", offset, taps, delay, rows, reserved, K, taps_len])["valid"]

    assert valid() == 1 and valid(rows=2) == 1 and valid(taps=4096, taps_len=4096, delay=4095) == 1
    assert valid(taps=0) == 0 and valid(taps=4097, taps_len=1 << 20) == 0
    assert valid(delay=16) == 0 and valid(delay=15) == 1
    assert valid(rows=0) == 0 and valid(rows=3) == 0 and valid(rows=3, K=3) == 1
    assert valid(reserved=1) == 0
    assert valid(offset=48) == 1 and valid(offset=49) == 0 and valid(offset=33, rows=2) == 0 and valid(offset=32, rows=2) == 1
    assert valid(offset=(1 << 64) - 8) == 0 and valid(offset=65) == 0  # no sum wraps


def test_stage_one_span(exe):
    def span(start, count, T, d):
        r = run(exe, ["span", start, count, T, d])
        return r["first"], r["count"], r["clip"], r["valid"]

    assert span(100, 50, 16, 0) == (85, 65, 0, 1)    # [start - 15, start + 50)
    assert span(100, 50, 16, 15) == (100, 65, 0, 1)  # [start, start + 50 + 15)
    assert span(3, 50, 16, 0) == (0, 53, 12, 1)      # 12 samples before the stream
    assert span(0, 50, 16, 7) == (0, 57, 8, 1)
    assert span(0, 0, 16, 0) == (0, 0, 0, 1)
    assert span(0, (1 << 31) - 16, 16, 0)[3] == 1 and span(0, (1 << 31) - 15, 16, 0)[3] == 0
    assert span(0, 1 << 63, 1, 0)[3] == 0
