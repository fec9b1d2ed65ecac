"""The filter rule of zig-flac_amd/csrc/fg_fir.hpp restated in numpy float64, as an independent
reference: np.convolve over the zero-extended signal.  The rule's element t of a window that starts
at `start` is y = sum over k of h[k] x[start + t + d - k], x zero outside [0, total); the float32
chain of T fused multiply-adds is within gamma_T sum |h[k] x[.]| of it, gamma_T = T u / (1 - T u),
u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1: a recursive sum of T products,
each step one rounding)."""
import numpy as np

U = 2.0 ** -24


def gamma(T: int) -> float:
    return T * U / (1.0 - T * U)


def delivered(total: int, start: int, count: int) -> int:
    return max(0, min(count, total - start))


def window64(x, h, d: int, start: int, count: int):
    """(y64, mag, n): the n = delivered elements of the window in float64, and sum |h[k] x[.]| of each."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    T, total = len(h), len(x)
    n = delivered(total, start, count)
    if n == 0:
        return np.zeros(0), np.zeros(0), 0
    lo, hi = start + d - (T - 1), start + n + d  # the samples the n elements read
    seg = np.zeros(hi - lo)
    a, b = max(lo, 0), min(hi, total)
    if b > a:
        seg[a - lo:b - lo] = x[a:b]
    return np.convolve(seg, h, mode="valid"), np.convolve(np.abs(seg), np.abs(h), mode="valid"), n


def taps(T: int, seed: int):
    """T float32 taps of both signs with a decaying envelope, none zero but every 7th."""
    rng = np.random.RandomState(seed)
    h = (rng.uniform(-1.0, 1.0, T) * np.exp(-np.arange(T) / max(T / 3.0, 1.0))).astype(np.float32)
    h[6::7] = 0.0
    if T == 1:
        h[0] = np.float32(-0.75)
    return h


def signal(total: int, seed: int, bits: int = 16):
    """One channel of float32 elements as the delivery gives them: integers of `bits` bits * 2^-(bits-1)."""
    rng = np.random.RandomState(seed)
    s = rng.randint(-(1 << (bits - 1)), 1 << (bits - 1), size=total).astype(np.float64)
    return (s * 2.0 ** -(bits - 1)).astype(np.float32)
