"""The resampling rule of the delivery (zig-flac_amd/csrc/fg_resample.hpp) in numpy float64: the
ratio and its validity, the filter formula (np.sinc, np.i0), the positions, the source range of a
window, the zero extension, and a float64 evaluation of the sum with its error bound.  Shared by
tests/test_resample_host.py, tests/test_resample_args.py and tests/test_gpu_resample.py; nothing here
calls the library."""
import math

import numpy as np

K_ZERO, K_BETA, K_ROLLOFF = 24, 9.0, 0.95
RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
U = 2.0 ** -24  # the unit roundoff of float32


def ratio(src, dst):
    """(L, M, Hw, T) of src -> dst, or None where the ratio is invalid (equal rates included)."""
    if src <= 0 or dst <= 0 or src == dst:
        return None
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    if not (1 <= L <= 1024 and 1 <= M <= 1024 and M <= 12 * L):
        return None
    Hw = K_ZERO if L >= M else -(-K_ZERO * M // L)
    return L, M, Hw, 2 * Hw


def table64(src, dst):
    """h64[p][k] in float64, every phase normalised to DC gain 1."""
    L, M, Hw, T = ratio(src, dst)
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    d = (k - Hw + 1.0) - p / L
    c = K_ROLLOFF * min(1.0, L / M)
    a = np.maximum(1.0 - (d / Hw) ** 2, 0.0)
    h = c * np.sinc(c * d) * np.i0(K_BETA * np.sqrt(a)) / np.i0(K_BETA)
    return h / h.sum(axis=1, keepdims=True)


def out_total(total, L, M):
    return (total * L + M - 1) // M


def delivered(total, L, M, start, count):
    return max(min(start + count, out_total(total, L, M)) - start, 0)


def source_range(total, L, M, Hw, start, n):
    if n == 0:
        return 0, 0
    return max(0, start * M // L - Hw + 1), min(total, (start + n - 1) * M // L + Hw + 1)


def taps_of(x, i0, Hw, T):
    """x[i0 - Hw + 1 .. + T) with zeros outside x."""
    out = np.zeros(T, dtype=x.dtype)
    a = i0 - Hw + 1
    lo, hi = max(a, 0), min(a + T, len(x))
    if hi > lo:
        out[lo - a:hi - a] = x[lo:hi]
    return out


def resample64(x, src, dst, start, count, table):
    """(y64, bound): output samples [start, start + count) clipped, of the float32 samples x, with
    `table` (the library's float table, or table64) widened to float64 and the sum in float64; and per
    output the bound gamma_T * sum |h| |x| + 1e-12 of a length-T recursive fma sum in float32."""
    L, M, Hw, T = ratio(src, dst)
    n = delivered(len(x), L, M, start, count)
    h = np.asarray(table, dtype=np.float64)
    xd = np.asarray(x, dtype=np.float64)
    gamma = T * U / (1.0 - T * U)
    y, b = np.zeros(n), np.zeros(n)
    for t in range(n):
        j = start + t
        i0, p = (j * M) // L, (j * M) % L
        w = taps_of(xd, i0, Hw, T)
        y[t] = float(np.dot(h[p], w))
        b[t] = gamma * float(np.dot(np.abs(h[p]), np.abs(w))) + 1e-12
    return y, b


def response_db(src, dst, freqs_of_lower_nyquist):
    """The filter's magnitude in dB at the given fractions of the lower of the two Nyquist rates:
    the prototype (all phases interleaved, at rate L * src) evaluated in float64."""
    L, M, Hw, T = ratio(src, dst)
    h = table64(src, dst)
    # prototype tap at time (k - Hw + 1) - p / L source samples
    p = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(T, dtype=np.float64)[None, :]
    t = ((k - Hw + 1.0) - p / L).ravel()
    g = h.ravel() / L
    nyq = 0.5 * min(1.0, L / M)  # cycles per source sample
    out = []
    for f in freqs_of_lower_nyquist:
        w = 2.0 * np.pi * f * nyq
        out.append(20.0 * np.log10(abs(np.sum(g * np.exp(-1j * w * t))) + 1e-300))
    return out
