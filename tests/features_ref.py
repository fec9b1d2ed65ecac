"""The feature rule of zig-flac_amd/csrc/fg_features.hpp restated in numpy float64, as an independent
statement of its DEFINITION: the table formula, framing with zero extension, and np.fft.rfft of the
windowed frames -- no table lookup, no chain.  With it, a per-element bound on what the float32
rule may differ from it, derived below from u = 2^-24 and the float64 quantities alone.

The bound.  gamma(k) = k u / (1 - k u) bounds a chain of k fused multiply-adds (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1 with one rounding a step).  For a bin, with c the float64
table and S = sum |c[n]| |xf[n]|:
  * a table entry is rounded once: |c32 - c| <= u |c|, so the exact sum over c32 is within u S;
  * the chain over c32 is within gamma(N) (1 + u) S of that sum;
  * rfft itself is not exact: 8 * 2^-53 * log2(N) * sum |w| |xf| covers it (Higham 24.1, generously);
  * every fused multiply-add may underflow by at most 2^-150.
  E = (u + gamma(N) (1 + u)) S + rfft term + N 2^-150, for re (c = w cos) and for im (c = w sin).
P = fl(im^2 + fl(re^2)) with |re^ - re| <= E_re, |im^ - im| <= E_im: the squares move by
2 |re| E_re + E_re^2 and 2 |im| E_im + E_im^2, the rounded product by u (|re| + E_re)^2, and the fused
multiply-add by u of its exact value:
  E_P = 2 |re| E_re + E_re^2 + 2 |im| E_im + E_im^2 + u (|re| + E_re)^2
        + u ((1 + u) (|re| + E_re)^2 + (|im| + E_im)^2) + 2^-149.
A filter row over F (the same float32 matrix on both sides) is one more chain:
  E_m = sum |F| E_P + gamma(B) sum |F| (P + E_P) + B 2^-150.
No constant here comes from an observed error."""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def bins(n_fft):
    return n_fft // 2 + 1


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def table64(n_fft):
    """[2, B, N] float64: w[n] cos(2 pi ((b n) mod N) / N), then -w[n] sin(...); b n reduced in integers."""
    n = np.arange(n_fft, dtype=np.int64)
    b = np.arange(bins(n_fft), dtype=np.int64)
    a = 2.0 * np.pi * ((b[:, None] * n[None, :]) % n_fft).astype(np.float64) / n_fft
    w = hann(n_fft)
    return np.stack([w * np.cos(a), -w * np.sin(a)])


def delivered(total, start, frames, hop):
    return 0 if start >= total else min(frames, -(-(total - start) // hop))


def frames64(x, n_fft, hop, start, frames):
    """[frames, N] float64: frame t is x[start + t hop - N / 2 + n], zero outside [0, len(x))."""
    x = np.asarray(x, dtype=np.float64)
    idx = start - n_fft // 2 + hop * np.arange(frames, dtype=np.int64)[:, None] + np.arange(n_fft, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    out = np.zeros(idx.shape, dtype=np.float64)
    out[ok] = x[idx[ok]]
    return out


def features64(x, n_fft, hop, start, frames, filters=None):
    """(y, bound, n): y float64 [rows, frames] by the definition, bound the derived per-element bound
    on |float32 rule - y|, n the frames whose centre lies inside x."""
    N, B = n_fft, bins(n_fft)
    xf = frames64(x, N, hop, start, frames)  # [T, N]
    w = hann(N)
    spec = np.fft.rfft(xf * w[None, :], axis=1)  # [T, B]: sum w x e^(-2 pi i b n / N)
    re, im = spec.real.T, spec.imag.T  # [B, T]
    tab = np.abs(table64(N))
    ax = np.abs(xf).T  # [N, T]
    fft_term = 8.0 * 2.0 ** -53 * np.log2(N) * (w[None, :] @ ax)  # [1, T]
    lead = U + gamma(N) * (1.0 + U)
    e_re = lead * (tab[0] @ ax) + fft_term + N * 2.0 ** -150
    e_im = lead * (tab[1] @ ax) + fft_term + N * 2.0 ** -150
    P = re * re + im * im
    are, aim = np.abs(re) + e_re, np.abs(im) + e_im
    e_P = (2.0 * np.abs(re) * e_re + e_re ** 2 + 2.0 * np.abs(im) * e_im + e_im ** 2 + U * are ** 2
           + U * ((1.0 + U) * are ** 2 + aim ** 2) + 2.0 ** -149)
    n = delivered(len(x), start, frames, hop)
    if filters is None:
        return P, e_P, n
    F = np.abs(np.asarray(filters, dtype=np.float64))
    y = np.asarray(filters, dtype=np.float64) @ P
    e_m = F @ e_P + gamma(B) * (F @ (P + e_P)) + B * 2.0 ** -150
    return y, e_m, n


def tone(total, n_fft, k, amp=0.5, seed=0):
    """A bin-centred tone (bin k of n_fft) with a little noise, float32 in [-1, 1)."""
    rng = np.random.RandomState(seed)
    t = np.arange(total)
    x = amp * np.sin(2.0 * np.pi * k * t / n_fft + 0.3) + 0.01 * rng.uniform(-1.0, 1.0, total)
    return x.astype(np.float32)
