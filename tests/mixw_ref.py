"""The independent expectation of the weighted channel mix (zig-flac_amd/csrc/fg_deliver.hpp:
mixw_value): output channel k of a sample is y = +0.0f, then y = fmaf(W[k][c], x_c, y) for
c = 0 .. C-1 in this order, x_c the float32 element of source channel c.

Method.  Plain float64 arithmetic is not exact here -- product plus accumulator can need more than
53 bits -- so `fma32` is float64 WITH AN EXPLICIT CORRECTION for the double rounding: the product
of two float32 is exact in float64 (48 bits); the sum s = p + y is formed with its exact error term
e (Knuth's two-sum, s + e = p + y exactly); where e != 0 and the significand of s is even, s is
moved one float64 step towards e, which is rounding to odd at 53 bits; a round-to-odd value of 53
bits rounds to the nearest-even float32 exactly as the unrounded sum does (53 >= 24 + 2).  No
intermediate overflows or underflows for valid weights (|w| in [2^-32, 2^32], |x| in [2^-31, 1]).
`fma32_exact` is the same operation in `fractions.Fraction`, one value at a time: the tests check
`fma32` against it on the ties.  Narrowing goes through numpy (f16) and torch on the CPU (bf16), as
in test_mix_host.py.  Nothing here calls the library."""
from fractions import Fraction

import numpy as np


def elements_f32(x, bits):
    """The float32 elements of the integer samples x (any shape): (float)x * 2^-(bits-1), the
    conversion to nearest-even."""
    return np.asarray(x, dtype=np.int64).astype(np.float32) * np.float32(2.0 ** -(bits - 1))


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, correctly rounded (see the module's docstring)."""
    a, b, c = (np.atleast_1d(np.asarray(v, dtype=np.float32)).astype(np.float64) for v in (a, b, c))
    p = a * b  # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # two-sum: s + e == p + c exactly
    assert not ((s == 0) & (e != 0)).any()  # a sum that rounds to zero is zero
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    step = np.where((e > 0) == (s > 0), 1, -1)  # one float64 away from zero where e has the sign of s, else towards it
    return (bits + np.where(fix, step, 0)).view(np.float64).astype(np.float32)


def _frac(v):
    return Fraction(float(np.float32(v)))


def round_f32(q):
    """The Fraction q rounded to the nearest-even float32 (normal range)."""
    if q == 0:
        return np.float32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    scaled = a / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    m, rem = divmod(scaled.numerator, scaled.denominator)
    twice = 2 * rem
    if twice > scaled.denominator or (twice == scaled.denominator and m & 1):
        m += 1
    return np.float32(sign * float(Fraction(m) * Fraction(2) ** (e - 23)))


def fma32_exact(a, b, c):
    """fmaf(a, b, c) of three float32 values in exact rational arithmetic."""
    return round_f32(_frac(a) * _frac(b) + _frac(c))


def mix(x, bits, W):
    """The weighted mix of the integer samples x [n, C] of `bits` bits by W [K, C] (float32):
    float32 [n, K], the chain in channel order from +0.0f."""
    x = np.asarray(x, dtype=np.int64)
    W = np.asarray(W, dtype=np.float32)
    assert x.ndim == 2 and W.ndim == 2 and x.shape[1] == W.shape[1]
    xf = elements_f32(x, bits)
    y = np.zeros((len(x), W.shape[0]), dtype=np.float32)
    for k in range(W.shape[0]):
        acc = np.zeros(len(x), dtype=np.float32)
        for c in range(W.shape[1]):
            acc = fma32(np.full(len(x), W[k, c], dtype=np.float32), xf[:, c], acc)
        y[:, k] = acc
    return y


def mix_exact(row, bits, w):
    """One output channel of one sample in exact rational arithmetic: the cross-check of `mix`."""
    acc = np.float32(0.0)
    for xc, wc in zip(elements_f32(np.asarray(row), bits), np.asarray(w, dtype=np.float32)):
        acc = fma32_exact(wc, xc, acc)
    return acc


def narrow(y):
    """(f32, f16, bf16) bit patterns of the float32 array y: f16 by numpy (infinity past the
    range), bf16 by torch on the CPU."""
    import torch

    y = np.ascontiguousarray(y, dtype=np.float32)
    with np.errstate(over="ignore"):
        f16 = y.astype(np.float16)
    bf16 = torch.from_numpy(y.reshape(-1).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).reshape(y.shape)
    return y.view(np.uint32), f16.view(np.uint16), bf16
