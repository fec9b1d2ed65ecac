"""Frames of more than 4096 samples (RFC 9639's streamable subset goes to 16384) from the seeded
grammar (frame_grammar.py): a spec list fed to frame_grammar._build_case.  Test side only; the
expected PCM of every frame is the generator's own samples.

The decoder cuts a frame of bs samples into 64 segments of seg_len(bs) = 64, 128 or 256 samples (bs
<= 4096, 8192, 16384), so the block sizes sit on both sides of each threshold, and the pinned
subframes are the ones whose restore walks a segment: FIXED orders 1 to 4, LPC at each ring size,
partition order 0 and partitions shorter than a segment.  Free draws often give CONSTANT or
VERBATIM, so every stereo and multichannel case pins FIXED / LPC subframes in its big frames.

Like frame_grammar.cases(), the module asserts what it claims before anybody uses the frames."""
from __future__ import annotations

import functools

import frame_grammar as fg

BIG = 4096  # frames above this are the "big" ones; the bit-list writer is slow on them


def _fixed(order, **kw):
    return dict({"type": "fixed", "order": order}, **kw)


_lpc = fg._lpc

_SPECS = [
    # mono 16-bit on both sides of each segment-length threshold.  4097, 8191, 8193 and 16383 are odd:
    # only partition order 0 divides them.  4608 = 2^9 * 9: order 9 gives 9-sample partitions inside
    # 128-sample segments; 16384 with order 8: 64-sample partitions inside 256-sample segments.
    ("big_mono_a", 1, 16, {"seed": 201, "blocks": [4097, 4608, 8191, 8192], "frames": [
        {"subs": [_fixed(1, kind="walk")]},
        {"subs": [_fixed(2, porder=9, waste=2, kind="sine")]},
        {"subs": [_lpc(8, kind="walk")]},
        {"subs": [_lpc(12, porder=5, kind="sine")]}]}),
    ("big_mono_b", 1, 16, {"seed": 202, "blocks": [8193, 16383, 16384], "frames": [
        {"subs": [_fixed(3, kind="sine")]},
        {"subs": [_fixed(4, kind="walk")]},
        {"subs": [_lpc(32, porder=8, kind="sine")]}]}),
    ("big_mid_side_16", 2, 16, {"seed": 203, "chc": 10, "blocks": [8192, 4608], "frames": [
        {"subs": [_fixed(2, porder=6, kind="walk"), _lpc(8, porder=0)]},
        {"subs": [_lpc(8, porder=9), _fixed(1, porder=4, kind="sine")]}]}),
    ("big_left_side_24", 2, 24, {"seed": 204, "chc": 8, "blocks": [8192, 4608], "frames": [
        {"subs": [_lpc(9, porder=7, kind="sine"), _fixed(4, porder=3)]},
        {"subs": [_fixed(3, porder=8, kind="walk"), _lpc(32, waste=1)]}]}),
    ("big_side_right_32", 2, 32, {"seed": 205, "chc": 9, "blocks": [8192, 4608], "frames": [
        {"subs": [_fixed(4, porder=5), _lpc(13, porder=2, kind="walk")]},
        {"subs": [_lpc(8, porder=9, kind="sine"), _fixed(2)]}]}),
    # 8 x 16-bit at 16384: two 32-bit planes fit at a time, so four rounds in each of two passes
    ("big_eight_by_16", 8, 16, {"seed": 206, "blocks": [16384], "frames": [{"subs": [
        {"type": "verbatim", "kind": "noise"}, _lpc(32, porder=8, kind="walk"), {"type": "constant"},
        _fixed(2, porder=10, kind="sine"), _lpc(9, porder=0), _fixed(4, porder=6, waste=3), {"type": "constant", "waste": 5},
        _lpc(12, porder=3, kind="tiny")]}]}),
    # 5 x 32-bit at 8192, the largest block of 64-bit planes: two fit at a time, three rounds, two passes
    ("big_five_by_32", 5, 32, {"seed": 207, "blocks": [8192], "frames": [{"subs": [
        {"type": "verbatim", "kind": "noise"}, _lpc(13, porder=7, kind="sine"), {"type": "constant"},
        _fixed(4, porder=4, kind="walk"), _lpc(8, waste=5, porder=0)]}]}),
    # variable blocking: the coded number is the first sample's
    ("big_variable", 2, 16, {"seed": 208, "chc": 10, "variable": True, "number": 0, "blocks": [4608, 64, 8192, 4096],
                             "frames": [
        {"subs": [_fixed(3, porder=9, kind="sine"), _lpc(7, porder=1)]},
        {"chc": 8, "subs": [_lpc(5), _fixed(1)]},
        {"chc": 9, "subs": [_lpc(12, porder=6, kind="walk"), _fixed(2, porder=12)]},
        {"chc": 1, "subs": [_fixed(4, porder=8), _lpc(32, porder=4)]}]}),
]

BLOCKS_MONO = {4097, 4608, 8191, 8192, 8193, 16383, 16384}


@functools.lru_cache(maxsize=None)
def cases():
    out = [fg._build_case(s) for s in _SPECS]
    big = [(c, f) for c in out for f in c["frames"] if f["block"] > BIG]
    assert len(big) <= 20
    mono = [f for c, f in big if c["channels"] == 1]
    assert {f["block"] for f in mono} == BLOCKS_MONO
    subs = [s for f in mono for s in f["subs"]]
    assert {s["order"] for s in subs if s["type"] == "fixed"} == {1, 2, 3, 4}
    assert {s["order"] for s in subs if s["type"] == "lpc"} == {8, 12, 32}
    every = [(f, s) for _, f in big for s in f["subs"] if s["type"] in ("fixed", "lpc")]
    assert any(s["psize"] == f["block"] for f, s in every)  # partition order 0
    assert any(s["psize"] == 64 and f["block"] == 16384 for f, s in every)  # partitions shorter than a segment
    assert any(s["psize"] == 9 and f["block"] == 4608 for f, s in every)
    assert any(s["escapes"] for f, s in every)  # an escaped partition
    assert any(s["waste"] for _, f in big for s in f["subs"])
    for c, f in big:  # every stereo and multichannel big frame restores at least one FIXED / LPC subframe
        assert c["channels"] == 1 or any(s["type"] in ("fixed", "lpc") for s in f["subs"]), c["name"]
    assert {(c["channels"], c["bits"], f["chc"]) for c, f in big} >= {(2, 16, 10), (2, 24, 8), (2, 32, 9), (8, 16, 7), (5, 32, 4)}
    var = next(c for c in out if c["name"] == "big_variable")
    assert [f["block"] for f in var["frames"]] == [4608, 64, 8192, 4096] and all(f["variable"] for f in var["frames"])
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)
