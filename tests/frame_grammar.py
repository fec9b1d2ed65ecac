"""A seeded grammar of FLAC frames no encoder here writes, on the frame writer flac_bits.py, from
RFC 9639 section 9.  Test side only, plain Python: it shares nothing with the encoder, the CPU
restatement, the verifier decoder or the decoder under test (fg_dec.hpp).

The generator chooses the SAMPLES first and then writes a frame that codes them, so the expected
PCM of every frame is the generator's own samples (for the stereo layouts undone here with Python
integers) and never a decoder's output.

cases() is a fixed list: seeded cases (everything not pinned by the list is drawn from
random.Random(seed)) and a few directed ones.  Like index_cases.py, the module asserts its
defining properties itself before anybody uses the frames: every frame's CRC-16 is zero, the
residual counts add up (flac_bits.residual), the PCM has the frame's length, and the coverage
table over the case list has no zero entry -- a drift in the grammar or in flac_bits then fails
loudly instead of silently testing less."""
from __future__ import annotations

import functools
import math
import random

import flac_bits as fb

BLOCK_SIZES = [1, 2, 5, 16, 17, 33, 63, 64, 65, 100, 128, 192, 255, 256, 257, 576, 1000, 1024, 1152, 4095, 4096]
KINDS = ("walk", "sine", "noise", "fullscale", "tiny", "spiky")
TYPES = ("constant", "verbatim", "fixed", "lpc")
LAYOUT = {8: "left_side", 9: "side_right", 10: "mid_side"}
MAX_UNARY = 300  # no Rice code's unary run is longer than this
RES_LIMIT = 1 << 31  # 9.2.7.3: a residual fits a signed 32-bit integer and is not the most negative one


def sub_depth(chc: int, c: int, bits: int) -> int:
    """9.1.3: the bit depth of subframe c; the side subframe of the three stereo layouts (the
    second of left/side and mid/side, the first of side/right) has one bit more."""
    side = {8: 1, 9: 0, 10: 1}.get(chc)
    return bits + 1 if c == side else bits


def signed_width(r: int) -> int:
    """The fewest bits that hold r in two's complement (0 for r == 0)."""
    if r == 0:
        return 0
    return (r if r > 0 else -r - 1).bit_length() + 1


# ---- samples ---------------------------------------------------------------------------------
def draw_samples(rng, kind: str, n: int, depth: int, damp: int):
    """n samples of `depth` bits; damp halves the amplitude that many times (redraws)."""
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    amp = 1 << max(depth - 1 - damp, 0)
    a_lo, a_hi = max(lo, -amp), min(hi, amp - 1)

    def clip(v):
        return max(a_lo, min(a_hi, v))

    if kind == "noise":
        return [rng.randint(a_lo, a_hi) for _ in range(n)]
    if kind == "fullscale":
        out = []
        while len(out) < n:
            out += [rng.choice((a_lo, a_hi))] * rng.randint(1, 9)
        return out[:n]
    if kind == "tiny":
        return [clip(rng.randint(-2, 2)) for _ in range(n)]
    if kind == "spiky":
        top = max(depth - 1 - damp, 0)
        return [clip(rng.choice((-1, 1)) << rng.randint(min(6, top), top)) if rng.random() < 1 / 24 else clip(rng.randint(-2, 2))
                for _ in range(n)]
    if kind == "walk":
        step = max(1, amp >> rng.randint(3, 9))
        v, out = rng.randint(a_lo, a_hi), []
        for _ in range(n):
            v = clip(v + rng.randint(-step, step))
            out.append(v)
        return out
    assert kind == "sine"
    a, f, ph = 0.7 * amp, rng.uniform(0.01, 0.5), rng.uniform(0, 6.28)
    noise = max(1, amp >> rng.randint(5, 12))
    return [clip(int(a * math.sin(f * i + ph)) + rng.randint(-noise, noise)) for i in range(n)]


# ---- the coded residual ----------------------------------------------------------------------
def plan_residual(rng, res, bs: int, order: int, force: dict):
    """Partition order, method and per-partition parameters for the residuals of one subframe ->
    (method, porder, params for flac_bits.residual, what was used: a dict for the coverage table)."""
    valid = [p for p in range(16) if bs % (1 << p) == 0 and (bs >> p) >= order]
    want = force.get("porder")
    if want == "max":
        porder = valid[-1]
    elif want == "empty":  # the first partition holds no residual
        porder = next(p for p in valid if (bs >> p) == order)
    elif want is not None:
        porder = want
    else:
        porder = rng.choice(valid)
    assert porder in valid
    psize = bs >> porder
    params, used = [], {"psize": psize, "empty_first": psize == order, "escapes": set(), "max_unary": 0}
    i = 0
    for pt in range(1 << porder):
        cnt = psize - (order if pt == 0 else 0)
        part = res[i:i + cnt]
        i += cnt
        us = [fb.zigzag(r) for r in part]
        need = max((signed_width(r) for r in part), default=0)
        roll = rng.random()
        if need == 0 and roll < 0.5:
            params.append(("esc", 0))
            used["escapes"].add("zero")
        elif roll < 0.10 and 1 <= need <= 31:
            params.append(("esc", need))
            used["escapes"].add("needed")
        elif roll < 0.18 and need < 31:
            params.append(("esc", rng.randint(need + 1, 31)))
            used["escapes"].add("wider")
        else:
            mean = sum(us) // max(cnt, 1)
            k = min(max(mean.bit_length() + rng.choice((-1, 0, 1)), 0), 30)
            top = max(us, default=0)
            if force.get("long_unary") and top >= 256:  # a low k on a large residual: a run of 128 to 255 zeros
                k = top.bit_length() - 8
            while (top >> k) > MAX_UNARY:
                k += 1
            assert k <= 30
            params.append(k)
            used["max_unary"] = max(used["max_unary"], top >> k)
    assert i == len(res) == bs - order  # the residual counts add up
    ks = [p for p in params if not isinstance(p, tuple)]
    method = 1 if any(k > 14 for k in ks) else force.get("method", 1 if rng.random() < 0.3 else 0)
    used["method"] = method
    return method, porder, params, used


# ---- one subframe ----------------------------------------------------------------------------
def _fits(res) -> bool:
    return all(-RES_LIMIT < r < RES_LIMIT for r in res)


def build_subframe(rng, bs: int, sb: int, force: dict, damp: int, given=None):
    """One subframe of sb bits per sample -> {"x": its samples, "write": writer(w), + coverage}.
    force: "type", "order", "waste", "kind", "porder", "method", "prec", "shift", "long_unary" pin what
    the seed would draw.  given: the samples are these (a stereo layout derived from left / right)."""
    typ = force.get("type") or rng.choice(TYPES)
    kind = force.get("kind") or rng.choice(KINDS)
    waste = force.get("waste")
    if waste is None:
        waste = 0 if rng.random() < 0.55 else rng.choice((1, 2, rng.randint(1, sb - 1), sb - 1))
    waste = min(waste, sb - 1)
    if given is not None:
        tz = min(((v & -v).bit_length() - 1 for v in given if v), default=0)
        waste = min(waste, tz)
    depth = sb - waste
    for attempt in range(64):
        d = damp + attempt // 2
        if given is not None:
            x = [v >> waste for v in given]
            if attempt >= 8:
                typ = "verbatim"  # whatever the samples are
        elif typ == "constant":
            x = [draw_samples(rng, kind, 1, depth, d)[0]] * bs
        else:
            x = draw_samples(rng, kind, bs, depth, d)
        full = [v << waste for v in x]
        meta = {"type": typ, "waste": waste, "kind": kind if typ != "constant" and given is None else None, "order": None}
        if typ == "constant":
            if len(set(x)) != 1:
                typ = "verbatim"
                continue
            return dict(meta, x=full, write=lambda w: fb.sub_constant(w, full[0], sb, waste))
        if typ == "verbatim":
            return dict(meta, x=full, write=lambda w: fb.sub_verbatim(w, full, sb, waste))
        if typ == "fixed":
            order = force.get("order")
            if order is None:
                order = rng.randint(0, min(4, bs))
            order = min(order, bs, 4)
            res = fb.fixed_residual(x, order)
            if not _fits(res):
                continue
            method, porder, params, used = plan_residual(rng, res, bs, order, force)
            return dict(meta, order=order, x=full, **used,
                        write=lambda w: fb.sub_fixed(w, full, sb, order, method, porder, params, waste=waste))
        assert typ == "lpc"
        order = force.get("order")
        if order is None:
            order = rng.randint(1, min(32, bs))
        order = min(order, bs, 32)
        prec = force.get("prec") or rng.randint(1, 15)
        shift = force["shift"] if "shift" in force else rng.randint(0, 15)
        down = attempt + (rng.randint(1, prec) if rng.random() < 0.5 else 0)  # sometimes scaled down
        coefs = [rng.randint(-(1 << (prec - 1)), (1 << (prec - 1)) - 1) >> min(down, 15) for _ in range(order)]
        res = fb.lpc_residual(x, coefs, shift)
        if not _fits(res):
            continue
        method, porder, params, used = plan_residual(rng, res, bs, order, force)
        return dict(meta, order=order, prec=prec, shift=shift, x=full, **used,
                    write=lambda w: fb.sub_lpc(w, full, sb, coefs, prec, shift, method, porder, params, waste=waste))
    raise AssertionError("no subframe after 64 redraws")


# ---- one frame -------------------------------------------------------------------------------
def _undo_stereo(chc: int, planes):
    """9.1.3, with exact integers: the left and right channels of a two-subframe stereo layout."""
    a, b = planes
    if chc == 8:  # left, side
        return [a, [l - s for l, s in zip(a, b)]]
    if chc == 9:  # side, right
        return [[s + r for s, r in zip(a, b)], b]
    assert chc == 10  # mid, side: the bit the mid lost in the halving is the side's lowest
    left, right = [], []
    for m, s in zip(a, b):
        m2 = 2 * m + (s & 1)
        assert (m2 + s) % 2 == 0
        left.append((m2 + s) // 2)
        right.append((m2 - s) // 2)
    return [left, right]


def _do_stereo(chc: int, left, right):
    side = [l - r for l, r in zip(left, right)]
    if chc == 8:
        return [left, side]
    if chc == 9:
        return [side, right]
    return [[(l + r) >> 1 for l, r in zip(left, right)], side]


def header_draw(rng, force: dict):
    """The header fields that do not bear on the samples -> (keyword arguments of flac_bits.frame,
    the sample rate they state; None: the stream's)."""
    rc = force.get("rate_code")
    if rc is None:
        rc = rng.choice((0, 12, 13, 14, rng.randint(1, 11), rng.randint(1, 11), 9))
    field, rate = 0, None
    if rc == 12:
        field = rng.randint(1, 255)
        rate = field * 1000
    elif rc == 13:
        field = rng.randint(1, 65535)
        rate = field
    elif rc == 14:
        field = rng.randint(1, 65535)
        rate = field * 10
    elif rc:
        rate = fb.RATE_OF_CODE[rc]
    kw = {"table_bs": force.get("table_bs", rng.random() < 0.6), "rate_code": rc, "rate_field": field,
          "bits_code": 0 if force.get("bits_code0", rng.random() < 0.3) else None}
    return kw, rate


def build_frame(rng, channels: int, bits: int, chc: int, bs: int, number: int, variable: bool, force: dict):
    """force: header pins (header_draw), "lr": derive a stereo layout's subframes from left / right
    samples of these kinds, "subs": [per-subframe force dicts]."""
    nsub = 2 if chc >= 8 else chc + 1
    assert nsub == channels and (chc < 8 or channels == 2)
    sub_force = force.get("subs") or [{}] * nsub
    sub_force = [sub_force[c % len(sub_force)] for c in range(nsub)]
    for damp in range(40):
        given = [None] * nsub
        if chc >= 8 and force.get("lr"):
            kinds = force["lr"]
            w0 = force.get("lr_waste", 0)
            lr = [[v << w0 for v in draw_samples(rng, kinds[c], bs, bits - w0, damp)] for c in range(2)]
            given = _do_stereo(chc, *lr)
        subs = [build_subframe(rng, bs, sub_depth(chc, c, bits), sub_force[c], damp, given[c]) for c in range(nsub)]
        planes = [s["x"] for s in subs]
        out = _undo_stereo(chc, planes) if chc >= 8 else planes
        if all(-(1 << (bits - 1)) <= v < (1 << (bits - 1)) for p in out for v in p):
            break  # else: an undone sample outside the bit depth, the frame is drawn again
    else:
        raise AssertionError("no frame after 40 redraws")
    if chc >= 8 and force.get("lr"):
        assert out == lr
    kw, rate = header_draw(rng, force)
    code = fb.block_size_code(bs) if kw["table_bs"] else (6 if bs <= 256 else 7)

    def write(w):
        for s in subs:
            s["write"](w)

    data = fb.frame(number, bs, chc, bits, write, variable=variable, **kw)
    assert fb.crc16(data) == 0
    nbytes = bits // 8
    pcm = b"".join((out[c][i] & ((1 << bits) - 1)).to_bytes(nbytes, "little") for i in range(bs) for c in range(channels))
    assert len(pcm) == bs * channels * nbytes
    for s in subs:
        del s["write"], s["x"]
    return {"frame": data, "number": number, "block": bs, "chc": chc, "rate": rate, "pcm": pcm, "subs": subs,
            "bs_code": code, "rate_code": kw["rate_code"], "bits_code0": kw["bits_code"] == 0, "variable": variable}


# ---- the case list ---------------------------------------------------------------------------
# (name, channels, bits, pins).  Pins: "chc" (a stereo layout), "blocks" (the frames' block sizes;
# else 3 to 5 drawn from those up to 1152), "variable", "number" (the first frame's), "rate" (the
# stream's), "frames": [per-frame force dicts of build_frame], cycled.
def _seeded(seed, channels, bits, **pins):
    return (f"seed{seed}_{channels}x{bits}", channels, bits, dict(pins, seed=seed))


def _lpc(order, **kw):
    return dict({"type": "lpc", "order": order}, **kw)


_SPECS = [
    _seeded(1, 1, 16), _seeded(2, 1, 16), _seeded(3, 1, 8), _seeded(4, 1, 24), _seeded(5, 1, 32),
    _seeded(6, 2, 16), _seeded(7, 2, 16, chc=8), _seeded(8, 2, 16, chc=9), _seeded(9, 2, 16, chc=10),
    _seeded(10, 2, 24, chc=8), _seeded(11, 2, 24, chc=9), _seeded(12, 2, 24, chc=10), _seeded(13, 2, 8, chc=10),
    _seeded(14, 2, 32, chc=8), _seeded(15, 2, 32, chc=9), _seeded(16, 2, 32, chc=10), _seeded(17, 2, 32),
    _seeded(18, 3, 16), _seeded(19, 3, 8), _seeded(20, 4, 24), _seeded(21, 4, 32), _seeded(22, 5, 16),
    _seeded(23, 6, 24), _seeded(24, 6, 32), _seeded(25, 7, 8), _seeded(26, 7, 32), _seeded(27, 8, 16),
    _seeded(28, 2, 16, chc=10, variable=True), _seeded(29, 1, 16, variable=True, number=(1 << 36) - 6000),
    _seeded(30, 2, 16, chc=8, number=(1 << 31) - 2),
    # directed: the LPC orders at the ring sizes' edges, in every stereo layout
    ("lpc_rings_mono", 1, 16, {"seed": 101, "blocks": [64, 100, 192, 33], "frames": [
        {"subs": [_lpc(1)]}, {"subs": [_lpc(7)]}, {"subs": [_lpc(8)]}, {"subs": [_lpc(9)]}]}),
    ("lpc_rings_mono_b", 1, 16, {"seed": 102, "blocks": [65, 128, 255, 32 * 8], "frames": [
        {"subs": [_lpc(12)]}, {"subs": [_lpc(13)]}, {"subs": [_lpc(31)]}, {"subs": [_lpc(32, porder="empty")]}]}),
    ("lpc_rings_left_side", 2, 16, {"seed": 103, "chc": 8, "blocks": [63, 257, 576], "frames": [
        {"subs": [_lpc(8), _lpc(9, waste=1)]}, {"subs": [_lpc(12), _lpc(13)]}, {"subs": [_lpc(32), _lpc(31, waste=2)]}]}),
    ("lpc_rings_side_right_24", 2, 24, {"seed": 104, "chc": 9, "blocks": [100, 1000, 17], "frames": [
        {"subs": [_lpc(9, waste=3), _lpc(8)]}, {"subs": [_lpc(13), _lpc(12)]}, {"subs": [_lpc(1), _lpc(7)]}]}),
    ("lpc_rings_mid_side_32", 2, 32, {"seed": 105, "chc": 10, "blocks": [192, 64, 1024], "frames": [
        {"subs": [_lpc(12), _lpc(13, waste=1)]}, {"subs": [_lpc(32), _lpc(8)]}, {"subs": [_lpc(9), _lpc(31)]}]}),
    # FIXED orders 1 to 4 with warm-up, in 4096 / 4095-sample blocks and partitions of 1 to 32 samples
    ("fixed_orders_big", 1, 16, {"seed": 106, "blocks": [4096, 4095, 1152, 64, 16], "frames": [
        {"subs": [{"type": "fixed", "order": 4, "porder": 8, "kind": "sine"}]},
        {"subs": [{"type": "fixed", "order": 3, "kind": "walk"}]},
        {"subs": [{"type": "fixed", "order": 2, "porder": 7, "kind": "spiky", "long_unary": True}]},
        {"subs": [{"type": "fixed", "order": 1, "porder": 6, "waste": 2}]},
        {"subs": [{"type": "fixed", "order": 4, "porder": "empty"}]}]}),
    ("fixed_orders_stereo_24", 2, 24, {"seed": 107, "chc": 10, "blocks": [4096, 128, 256], "frames": [
        {"subs": [{"type": "fixed", "order": 4, "kind": "walk"}, {"type": "fixed", "order": 3, "waste": 1, "porder": 7}]},
        {"subs": [{"type": "fixed", "order": 2, "porder": 6}, {"type": "fixed", "order": 1, "porder": 5}]},
        {"subs": [{"type": "fixed", "order": 0, "porder": 4}, {"type": "fixed", "order": 4, "porder": 3}]}]}),
    # left at + full scale, right at - full scale: the side subframe uses all its bits + 1
    ("full_scale_sides", 2, 32, {"seed": 108, "chc": 10, "blocks": [100, 65, 33], "frames": [
        {"lr": ("fullscale", "fullscale"), "subs": [{"type": "verbatim"}]},
        {"lr": ("fullscale", "noise"), "chc": 8, "subs": [{"type": "fixed", "order": 0}]},
        {"lr": ("noise", "fullscale"), "chc": 9, "lr_waste": 3, "subs": [{"type": "verbatim", "waste": 3}]}]}),
    ("full_scale_sides_16", 2, 16, {"seed": 109, "chc": 8, "blocks": [255, 5, 2, 1], "frames": [
        {"lr": ("fullscale", "fullscale"), "subs": [{"type": "fixed", "order": 0}, {"type": "verbatim"}]},
        {"lr": ("walk", "sine"), "chc": 10, "lr_waste": 2, "subs": [{"type": "fixed", "order": 1, "waste": 2}]},
        {"lr": ("tiny", "fullscale"), "chc": 9}, {"lr": ("fullscale", "tiny"), "chc": 10}]}),
    # 5 and 8 channels at 32 bits: more subframes than the 64-bit planes that fit at once
    ("five_by_32", 5, 32, {"seed": 110, "blocks": [257, 576, 63], "frames": [{"subs": [
        {"type": "verbatim", "kind": "noise"}, _lpc(13, kind="sine"), {"type": "constant"}, {"type": "fixed", "order": 4},
        _lpc(8, waste=5)]}]}),
    ("eight_by_32", 8, 32, {"seed": 111, "blocks": [1000, 4096, 17], "frames": [{"subs": [
        {"type": "verbatim", "kind": "fullscale"}, _lpc(32, kind="walk"), {"type": "constant", "waste": 7},
        {"type": "fixed", "order": 2, "kind": "sine"}, _lpc(9), {"type": "verbatim", "waste": 31, "kind": "noise"},
        {"type": "constant"}, _lpc(12, kind="tiny")]}]}),
    # wasted bits up to bps - 1 on every type, low Rice parameters on spikes, method 1
    ("waste_and_unary", 1, 24, {"seed": 112, "blocks": [128, 192, 1152, 256, 100], "frames": [
        {"subs": [{"type": "constant", "waste": 23}]}, {"subs": [{"type": "verbatim", "waste": 23}]},
        {"subs": [{"type": "fixed", "order": 2, "waste": 20, "kind": "noise"}]},
        {"subs": [_lpc(5, waste=23, porder=0)]},
        {"subs": [{"type": "fixed", "order": 1, "kind": "spiky", "porder": 2, "method": 1, "long_unary": True}]}]}),
]


def _build_case(spec):
    name, channels, bits, pins = spec
    rng = random.Random(pins["seed"])
    blocks = pins.get("blocks") or rng.sample([b for b in BLOCK_SIZES if b <= 1152], rng.randint(3, 5))
    variable = pins.get("variable", False)
    number = pins["number"] if "number" in pins else rng.choice((0, 3, 126, 2046, rng.randrange(1 << 20)))
    forces = pins.get("frames") or [{}]
    frames = []
    for j, bs in enumerate(blocks):
        force = forces[j % len(forces)]
        chc = force.get("chc", pins.get("chc", channels - 1))
        frames.append(build_frame(rng, channels, bits, chc, bs, number, variable, force))
        number += bs if variable else 1
    return {"name": name, "channels": channels, "bits": bits, "rate": pins.get("rate", rng.choice((44100, 48000, 96000))),
            "frames": frames}


def coverage(case_list) -> dict:
    """What the frames of case_list exercise; every key below is listed, so a zero entry shows."""
    layouts = ("mono", "independent") + tuple(LAYOUT.values())
    keys = [f"{t}/{l}" for t in TYPES for l in layouts]
    keys += [f"lpc_order_{o}" for o in (1, 7, 8, 9, 12, 13, 31, 32)] + ["lpc_ring_8", "lpc_ring_12", "lpc_ring_32"]
    keys += ["lpc_precision_1", "lpc_precision_15", "lpc_shift_0", "lpc_shift_15", "stereo_independent"]
    keys += [f"fixed_order_{o}" for o in range(5)] + [f"waste/{t}" for t in TYPES] + ["waste/side"]
    keys += [f"waste_max/{t}" for t in TYPES]  # depth - 1 wasted bits: one bit a sample is left
    keys += ["method_0", "method_1", "escape_zero", "escape_needed", "escape_wider", "empty_first_partition"]
    keys += [f"partition_of_{n}" for n in (1, 2, 16, 32)] + ["unary_over_32", "unary_over_64"]
    keys += [f"block_{b}" for b in BLOCK_SIZES] + [f"bs_code_{c}" for c in ("1", "2-5", "6", "7", "8-15")]
    keys += [f"rate_code_{c}" for c in ("0", "1-11", "12", "13", "14")] + ["bits_code_0", "bits_code_own"]
    keys += ["strategy_0", "strategy_1", "number_over_31_bits", "wide_planes_two_passes"]
    keys += [f"channels_{c}" for c in range(1, 9)] + [f"bits_{b}" for b in (8, 16, 24, 32)] + [f"kind_{k}" for k in KINDS]
    cov = dict.fromkeys(keys, 0)
    for case in case_list:
        cov[f"channels_{case['channels']}"] += 1
        cov[f"bits_{case['bits']}"] += 1
        for f in case["frames"]:
            chc = f["chc"]
            layout = LAYOUT.get(chc) or ("mono" if chc == 0 else "independent")
            c = f["bs_code"]
            cov["bs_code_" + ("1" if c == 1 else "2-5" if c <= 5 else str(c) if c <= 7 else "8-15")] += 1
            c = f["rate_code"]
            cov["rate_code_" + (str(c) if c == 0 or c >= 12 else "1-11")] += 1
            cov["bits_code_0" if f["bits_code0"] else "bits_code_own"] += 1
            cov["strategy_1" if f["variable"] else "strategy_0"] += 1
            cov["number_over_31_bits"] += f["number"] >= 1 << 31
            cov["stereo_independent"] += chc == 1
            cov[f"block_{f['block']}"] += 1
            cov["wide_planes_two_passes"] += case["bits"] == 32 and case["channels"] > 4
            for i, s in enumerate(f["subs"]):
                t = s["type"]
                cov[f"{t}/{layout}"] += 1
                if s["waste"]:
                    cov[f"waste/{t}"] += 1
                    cov["waste/side"] += sub_depth(chc, i, case["bits"]) > case["bits"]
                    cov[f"waste_max/{t}"] += s["waste"] == sub_depth(chc, i, case["bits"]) - 1
                if s["kind"]:
                    cov[f"kind_{s['kind']}"] += 1
                if t == "lpc":
                    o = s["order"]
                    if f"lpc_order_{o}" in cov:
                        cov[f"lpc_order_{o}"] += 1
                    cov["lpc_ring_8" if o <= 8 else "lpc_ring_12" if o <= 12 else "lpc_ring_32"] += 1
                    for key, v in (("precision", s["prec"]), ("shift", s["shift"])):
                        if f"lpc_{key}_{v}" in cov:
                            cov[f"lpc_{key}_{v}"] += 1
                if t == "fixed":
                    cov[f"fixed_order_{s['order']}"] += 1
                if t in ("fixed", "lpc"):
                    cov[f"method_{s['method']}"] += 1
                    for e in s["escapes"]:
                        cov[f"escape_{e}"] += 1
                    cov["empty_first_partition"] += s["empty_first"]
                    if f"partition_of_{s['psize']}" in cov:
                        cov[f"partition_of_{s['psize']}"] += 1
                    cov["unary_over_32"] += s["max_unary"] > 32
                    cov["unary_over_64"] += s["max_unary"] > 64
    return cov


@functools.lru_cache(maxsize=None)
def cases():
    """[{"name", "channels", "bits", "rate": the stream's, "frames": [{"frame": bytes, "number",
    "block", "chc", "rate": the header's own or None, "pcm": the generator's samples, ...}]}]"""
    out = [_build_case(s) for s in _SPECS]
    assert len({c["name"] for c in out}) == len(out)
    missing = [k for k, v in coverage(out).items() if v == 0]
    assert not missing, f"the frame grammar's case list no longer covers: {missing}"
    return out


def frame_rate(case, f) -> int:
    return case["rate"] if f["rate"] is None else f["rate"]


def case_pcm(case) -> bytes:
    return b"".join(f["pcm"] for f in case["frames"])


def case_bytes(case) -> bytes:
    return b"".join(f["frame"] for f in case["frames"])
