"""A seeded, directed generator of frames that make the encoder take every fixed-order and Rice
decision, and a tally of the decisions the CPU restatement (oracle/) reports for them.  Test
infrastructure, in the style of frame_grammar.py and fuzz_blocks.py; pure numpy.

frames(ch, bits): a fixed list of named 4096-sample frames, int64 [4096, ch].
  grid      k-fold integrated noise whose level is redrawn per 4096 >> p samples: one frame per
            fixed order k = 0..4 x partition order p = 0..8 x three of the four stereo relations in
            rotation (independent R, R = L + d, R = -L + d, R = L/2 + d: channel codes 1, 8, 9,
            10); other channel counts take two seeds of the k x p grid with independent channels
  sine      clean and lightly noised sinusoids at 0.002 .. 0.3 rad/sample (fixed orders 2, 3, 4)
  ladder    noise of every amplitude 2^0 .. 2^(bits-1), held and per-16-sample enveloped: every
            Rice parameter the depth reaches (stereo: through every relation, so the 17-bit side too)
  fuzz      every fuzz_blocks kind, plain and under a per-16-sample envelope: escapes, wasted bits,
            constant and verbatim subframes
  edge      all-zero, DC and full-scale white noise
  named     frames for single decisions: two fixed orders' totals tied at the minimum
tails(ch, bits): the grid family drawn at ragged lengths that bracket the tail kernel's partition
  cap (part_cap in fg_device.hpp: ctz(n), log2(n) - log2(kw), n >> P >= kw), noise gated per
  n >> p samples at every partition order, plus noise and sines.
tally(records): what oracle_ref.encode_frame decided, as a Counter.

tests/test_encode_cases_host.py holds the floors the tally must reach (so the GPU module cannot
cover less than it claims) and the SHA-256 pins of every set (tests/golden/encode_cases_sha.json;
`python tests/encode_cases.py` rewrites them).
"""
from __future__ import annotations

import collections
import functools
import hashlib
import json
import os

import numpy as np

import fuzz_blocks

N = 4096
RATE = {(2, 16): 44100, (1, 16): 44100, (3, 16): 48000, (2, 24): 96000, (2, 32): 192000, (8, 24): 96000,
        (1, 8): 8000}
CONFIGS = list(RATE)
TAIL_LENGTHS = [16, 32, 256, 2048, 48, 1152, 3072, 4032, 17, 4095, 1, 2, 3, 4, 5]
# (max_rice_part_order, max_rice_param)
CAPS = [(0, 30), (2, 1), (3, 30), (4, 30), (8, 5), (8, 14), (8, 15)]
RELATIONS = ("indep", "plus", "minus", "half")
# the draws of one (length, fixed order, partition order) cell of tails(): _integrated's `bimodal`
TAIL_DRAWS = (False, "alternate", True, "alternate", True)
SHA_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_cases_sha.json")


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def _range(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def _integrated(rng, n, bits, order, po, bimodal=False):
    """`order`-fold integrated noise whose level is redrawn per n >> po samples, centred and scaled
    into range: fixed order `order` whitens it, and partitions of n >> po samples each want a Rice
    parameter of their own.  bimodal: silence or the highest level, drawn or ("alternate") strictly
    in turn (the contrast that pays for a parameter per partition even where a partition is one or
    two samples, and at 8 bits only where every coarser partition would mix the two)."""
    lo, hi = _range(bits)
    segs = 1 << po
    seg = max(1, n >> po)
    top = max(2, bits - 2 - 3 * order)
    lev = rng.integers(0, top, size=segs + 1)
    amp = 2.0 ** lev
    if bimodal:
        loud = rng.random(segs + 1) < 0.5
        if bimodal == "alternate":
            loud = (np.arange(segs + 1) + int(loud[0])) % 2 == 1
        amp = np.where(loud, 2.0 ** (bits - 2), 0.0)
    amp = np.repeat(amp, seg)[:n]
    if len(amp) < n:
        amp = np.concatenate([amp, np.full(n - len(amp), amp[-1])])
    x = np.rint(rng.normal(0, 1, size=n) * amp)
    for _ in range(order):
        x = np.cumsum(x)
    x = x - np.rint((x.max() + x.min()) / 2)
    m = max(abs(x.max()), abs(x.min()), 1)
    if m > hi:
        x = np.rint(x * (hi / m))
    return np.clip(x, lo, hi).astype(np.int64)


def _related(rng, x, bits, relation, fresh):
    """The second channel of a stereo pair: `fresh()` draws an independent one."""
    lo, hi = _range(bits)
    d = rng.integers(-3, 4, size=len(x))
    if relation == "indep":
        y = fresh()
    elif relation == "plus":
        y = x + d
    elif relation == "minus":
        y = -x + d
    else:
        y = x // 2 + d
    return np.clip(y, lo, hi).astype(np.int64)


def _grid_frame(rng, n, ch, bits, order, po, relation, bimodal=False):
    def fresh():
        return _integrated(rng, n, bits, order, po, bimodal)

    x = fresh()
    cols = [x]
    for _ in range(1, ch):
        cols.append(_related(rng, x, bits, relation, fresh))
    return np.stack(cols, axis=1)


def _sine_frame(rng, n, ch, bits, f, a, nz):
    lo, hi = _range(bits)
    t = np.arange(n)[:, None]
    x = a * hi * np.sin(t * f * (1.0 + 0.3 * np.arange(ch))[None, :] + 0.3)
    if nz:
        x = x + rng.normal(0, nz, size=(n, ch))
    return np.clip(np.rint(x), lo, hi).astype(np.int64)


def _envelope(rng, x, bits, seg=16):
    """Scale every `seg` samples by a power of two of their own."""
    n = len(x)
    env = np.repeat(2.0 ** (-rng.integers(0, bits - 2, size=(n + seg - 1) // seg).astype(np.float64)), seg)[:n, None]
    return np.rint(x * env).astype(np.int64)


def _ladder_frame(rng, n, ch, bits, k, relation, enveloped):
    """White noise of amplitude 2^k; enveloped: amplitude 2^k and 2^(k-3) in alternate runs of 16."""
    lo, hi = _range(bits)

    def fresh():
        amp = np.full(n, float(1 << k))
        if enveloped:
            amp[(np.arange(n) // 16) % 2 == 1] = float(1 << max(k - 3, 0))
        return np.clip(np.rint(rng.uniform(-1, 1, size=n) * amp), lo, hi).astype(np.int64)

    x = fresh()
    cols = [x]
    for _ in range(1, ch):
        cols.append(_related(rng, x, bits, relation, fresh))
    return np.stack(cols, axis=1)


def _gated_frame(rng, n, ch, bits, po, lev):
    """White noise of amplitude 2^lev, on or off per n >> po samples; every channel its own gates."""
    lo, hi = _range(bits)
    seg = max(1, n >> po)
    on = np.repeat(rng.random(((n + seg - 1) // seg, ch)) < 0.5, seg, axis=0)[:n]
    x = np.rint(rng.uniform(-1, 1, size=(n, ch)) * float(1 << lev)) * on
    return np.clip(x, lo, hi).astype(np.int64)


def _check(name, x, n, ch, bits):
    lo, hi = _range(bits)
    assert x.shape == (n, ch) and x.dtype == np.int64, name
    assert x.min() >= lo and x.max() <= hi, name


@functools.lru_cache(maxsize=None)
def frames(ch, bits):
    """[(name, int64 [4096, ch])]: the full frames of one configuration, in a fixed order."""
    out = []
    stereo = ch == 2
    rels = RELATIONS if stereo else ("indep",)
    for rep in range(1 if stereo else 2):
        for order in range(5):
            for po in range(9):
                for r, rel in enumerate(rels):
                    if stereo and r == (order + po) % 4:
                        continue  # three of the four relations per cell, in rotation: 135 frames, not 180
                    rng = _rng(101, ch, bits, rep, order, po, r)
                    out.append((f"grid-k{order}-p{po}-{rel}-{rep}", _grid_frame(rng, N, ch, bits, order, po, rel)))
    i = 0
    for f in (0.002, 0.005, 0.01, 0.02, 0.04, 0.08, 0.15, 0.3):
        for a in (0.9, 0.3, 0.05):
            for nz in (0, 0.5):
                out.append((f"sine-f{f}-a{a}-n{nz}", _sine_frame(_rng(202, ch, bits, i), N, ch, bits, f, a, nz)))
                i += 1
    for k in range(bits):
        rel = rels[k % len(rels)]
        env = (k // len(rels)) % 2 == 1
        rng = _rng(303, ch, bits, k)
        out.append((f"ladder-a{k}-{rel}-{'env' if env else 'flat'}", _ladder_frame(rng, N, ch, bits, k, rel, env)))
    if stereo:  # full-scale L and R = -L: the side at its widest, the largest parameter of the depth
        out.append(("ladder-top-minus", _ladder_frame(_rng(304, ch, bits), N, ch, bits, bits - 1, "minus", False)))
    for i, kind in enumerate(fuzz_blocks.ALL_KINDS):
        for v in range(3):
            rng = _rng(404, ch, bits, i, v)
            x = fuzz_blocks.block(rng, N, ch, bits, kind)
            if stereo and v == 1 and kind != "antiphase":  # the kinds draw channels independently: relate them
                x[:, 1] = _related(rng, x[:, 0], bits, RELATIONS[1 + i % 3], None)
            if v == 2:
                x = _envelope(rng, x, bits)
            out.append((f"fuzz-{kind}-{('plain', 'related', 'env')[v]}", x))
    lo, hi = _range(bits)
    out.append(("edge-zero", np.zeros((N, ch), dtype=np.int64)))
    out.append(("edge-dc", np.tile(_rng(707, ch, bits).integers(lo // 2, hi // 2, size=(1, ch)), (N, 1))))
    out.append(("edge-fullscale-noise", _rng(708, ch, bits).integers(lo, hi + 1, size=(N, ch))))
    out += _named(ch, bits)
    for name, x in out:
        _check(name, x, N, ch, bits)
    assert len({name for name, _ in out}) == len(out)
    return out


def fixed_totals(x):
    """bestOrder's totals (fixed.zig:85-167): the sum of |k-th difference| over samples k .. n - 1."""
    return [int(np.abs(np.diff(x, k)).sum()) for k in range(5)]


def _tie_channel(k):
    """A channel whose totals of fixed orders k and k + 1 (k = 0, 1) are equal and the smallest: runs of
    two +1 and two -1 (every second step flips the sign, so the next difference sums to twice as
    much less the zeros) with zeros put in until the two sums meet; k = 1 integrates it once."""
    for nz in range(1, 64):
        for first in range(4, 400):
            y = np.tile(np.array([1, 1, -1, -1], dtype=np.int64), N // 4)
            y[first:first + 7 * nz:7] = 0
            x = np.cumsum(y) + 40 if k else y
            t = fixed_totals(x)
            if t[k] == t[k + 1] == min(t):
                return x
    raise AssertionError("no tie")


def _named(ch, bits):
    """Frames for single decisions the families do not reach on full frames.
    tie-k01 / tie-k12: the totals of two fixed orders tie at the minimum (the first wins,
    fixed.zig:164) in every channel; the channels are equal, so the side is CONSTANT and the four
    stereo sums tie as well (the first wins again).  Without them no full frame reaches a tie."""
    return [(f"tie-k{k}{k + 1}", np.tile(_tie_channel(k)[:, None], (1, ch))) for k in (0, 1)]


def part_cap(n, kw, max_part_order=8):
    """rice.calcParams' partition-order cap as the tail kernel and the restatement apply it."""
    lim = (n.bit_length() - 1) - (kw.bit_length() - 1) if kw else 15
    ctz = (n & -n).bit_length() - 1
    p = min(max_part_order, ctz, lim)
    while p > 0 and (n >> p) < kw:
        p -= 1
    return p


def allowed_part_orders(n):
    """Every partition order some fixed order's part_cap allows at length n."""
    return sorted({p for kw in range(0, min(5, n + 1)) for p in range(part_cap(n, kw) + 1)})


@functools.lru_cache(maxsize=None)
def tails(ch, bits):
    """[(name, int64 [n, ch])] for n in TAIL_LENGTHS: frames shorter than a block."""
    out = []
    stereo = ch == 2
    rels = RELATIONS if stereo else ("indep",)
    for n in TAIL_LENGTHS:
        j = 0
        for order in range(5):
            cap = part_cap(n, min(order, n))
            for po in range(cap + 1):
                # one graded draw per cell; at the cap (partitions of one or two samples where n is a
                # small power of two) four bimodal ones as well: only a stark contrast pays for a
                # parameter per sample
                for rep, bimodal in enumerate(TAIL_DRAWS if po == cap else TAIL_DRAWS[:1]):
                    rel = rels[j % len(rels)]
                    rng = _rng(505, ch, bits, n, order, po, rep)
                    out.append((f"tail{n}-k{order}-p{po}-{rel}-{rep}",
                                _grid_frame(rng, n, ch, bits, order, po, rel, bimodal=bimodal)))
                    j += 1
        # gated noise at every partition order the length allows and three loudnesses: silence or
        # noise of amplitude 2^lev per n >> po samples (what makes partitions of 2..8 samples pay at
        # 8 bits, where only a near-full-scale contrast does)
        for po in range(part_cap(n, 0) + 1):
            for lev in (bits // 2, bits - 2, bits - 1):
                for rep in range(2 if n <= 256 else 1):  # short frames are cheap and their choices chancier
                    rng = _rng(509, ch, bits, n, po, lev, rep)
                    out.append((f"tail{n}-gated-p{po}-a{lev}-{rep}", _gated_frame(rng, n, ch, bits, po, lev)))
        out.append((f"tail{n}-sine", _sine_frame(_rng(606, ch, bits, n), n, ch, bits, 0.02, 0.8, 0.5)))
        out.append((f"tail{n}-noise", fuzz_blocks.block(_rng(607, ch, bits, n), n, ch, bits, "noise")))
        out.append((f"tail{n}-mixture", fuzz_blocks.block(_rng(608, ch, bits, n), n, ch, bits, "mixture")))
        out.append((f"tail{n}-constant", np.full((n, ch), n % 7 - 3, dtype=np.int64)))
    for name, x in out:
        _check(name, x, len(x), ch, bits)
    assert len({name for name, _ in out}) == len(out)
    return out


def cap_subset(ch, bits):
    """The full frames the capped configurations run on: partition orders on both sides of every cap
    (grid, fixed orders 0 and 2), every Rice parameter (ladder) and the escapes (fuzz)."""
    return [(name, x) for name, x in frames(ch, bits)
            if name.startswith(("grid-k0-", "grid-k2-", "ladder-", "fuzz-mixture", "fuzz-spikes", "fuzz-noise"))
            and not name.endswith("-1")]


def pow2_tails(ch, bits):
    return [(name, x) for name, x in tails(ch, bits) if len(x) in (16, 32, 256, 2048)]


def pcm_bytes(x, bits):
    import synth

    return synth.to_pcm_bytes(x, bits)


def planes(x):
    return [np.ascontiguousarray(x[:, c]).astype(np.int32) for c in range(x.shape[1])]


_oracle_cache = {}


def oracle(ch, bits, name, x, frame_number=0, **kw):
    """(frame bytes, ORec) of the restatement for one generator frame; kept per (frame, settings)."""
    import oracle_ref

    key = (ch, bits, name, len(x), frame_number, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        kw2 = dict(kw)
        block = kw2.pop("block", N)
        _oracle_cache[key] = oracle_ref.encode_frame(planes(x), len(x), frame_number, ch, bits, RATE[(ch, bits)],
                                                     block=block, **kw2)
    return _oracle_cache[key]


def tally(records, block=N):
    """Counter over the decisions in `records` (ORecs of oracle_ref.encode_frame, or (n, ORec) pairs
    for frames of n samples; bare ORecs are full frames), split into "full" frames (n == block ==
    4096) and "tail" frames.  Keys, each counted once per FRAME that holds it in a written subframe:
      (scope, "frames")            (scope, "code", channel code)
      (scope, "type", 0 constant | 1 verbatim | 2 fixed | 3 lpc)
      (scope, "order", fixed order)   (scope, "po", partition order)   (scope, "method", 0 | 1)
      (scope, "escape")  a subframe with an escape partition     (scope, "waste")  wasted bits > 0
    and once per PARTITION:  (scope, "param", Rice parameter)."""
    T = collections.Counter()
    for rec in records:
        n = N
        if isinstance(rec, tuple):
            n, rec = rec
        scope = "full" if n == block == N else "tail"
        seen = {("frames",), ("code", rec.channel_code)}
        for i in range(rec.n_sub):
            w = rec.written[i]
            seen.add(("type", w.type))
            if w.waste:
                seen.add(("waste",))
            if w.type >= 2:
                if w.type == 2:
                    seen.add(("order", w.order))
                seen.add(("po", w.part_order))
                seen.add(("method", w.method))
                for p in list(w.params)[:1 << w.part_order]:
                    if p >= 0x80:
                        seen.add(("escape",))
                    else:
                        T[(scope, "param", p)] += 1
        for k in seen:
            T[(scope,) + k] += 1
    return T


def sha_table():
    """[{"name": ..., "sha256": ...}]: the PCM of every set, frames in order, and their names."""
    rows = []
    for ch, bits in CONFIGS:
        for kind, fs in (("frames", frames(ch, bits)), ("tails", tails(ch, bits))):
            h = hashlib.sha256()
            for name, x in fs:
                h.update(name.encode() + b"\0")
                h.update(pcm_bytes(x, bits))
            rows.append({"name": f"{kind}-{ch}ch{bits}", "sha256": h.hexdigest()})
    return rows


if __name__ == "__main__":  # rewrite the pins (after a deliberate change of the generator)
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zig-flac_amd"))
    with open(SHA_FILE, "w") as f:
        json.dump(sha_table(), f, indent=1)
        f.write("\n")
    print(f"wrote {SHA_FILE}")
