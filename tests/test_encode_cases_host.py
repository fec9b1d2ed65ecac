"""What tests/encode_cases.py covers, asserted on the CPU restatement alone (no GPU): the floors
below are the condition that keeps tests/test_gpu_encode_cases.py from comparing fewer decisions
than it claims.  A class the generator stops reaching fails here; the remedy is a frame, never a
lower floor.
"""
import hashlib
import json

import pytest

import encode_cases as ec
import oracle_ref

# (channels, bits, stereo decorrelation)
FLOOR_CONFIGS = [(2, 16, True), (2, 16, False), (1, 16, True), (3, 16, True), (2, 24, True), (2, 32, True),
                 (8, 24, True), (1, 8, True)]
CAP_CONFIGS = [(2, 16, True), (2, 16, False), (1, 16, True), (3, 16, True), (2, 32, True), (8, 24, True)]
FLOOR = 2  # full frames per class


def _records(ch, bits, fs, **kw):
    return [ec.oracle(ch, bits, name, x, **kw)[1] for name, x in fs]


def _max_param(T, scope="full"):
    return max(k[2] for k in T if k[:2] == (scope, "param"))


@pytest.mark.parametrize("ch,bits,stereo", FLOOR_CONFIGS)
def test_default_configuration_floors(ch, bits, stereo):
    fs = ec.frames(ch, bits)
    assert 150 <= len(fs) <= 250
    T = ec.tally(_records(ch, bits, fs, stereo=stereo))
    assert T[("full", "frames")] == len(fs) and not any(k[0] == "tail" for k in T)
    need = [("type", 0), ("type", 1), ("type", 2), ("escape",), ("waste",), ("method", 0)]
    need += [("order", k) for k in range(3)] + [("po", p) for p in range(9)]
    if (ch, bits) != (1, 8):
        need += [("order", 3), ("order", 4)]
    else:
        # 8 bits: the rounding noise of a sinusoid is a larger share of so small a signal, and orders 3
        # and 4 amplify it 8- and 16-fold.  The restatement reaches order 3 on 4 full frames and order
        # 4 on 1; no parameter above 6 exists at this depth, so the method bit is always 0.
        need += [("order", 3)]
        assert T[("full", "order", 4)] >= 1
    if bits > 16 or (ch == 2 and stereo):  # a depth, or a 17-bit side, whose parameters pass 14
        need += [("method", 1)]
    else:
        assert T[("full", "method", 1)] == 0
    if ch == 2 and stereo:
        need += [("code", c) for c in (1, 8, 9, 10)]
    short = {k: T[("full",) + k] for k in need if T[("full",) + k] < FLOOR}
    assert not short, f"classes on fewer than {FLOOR} full frames: {short}"
    top = _max_param(T)
    missing = [p for p in range(top + 1) if not T[("full", "param", p)]]
    assert not missing, f"Rice parameters never selected below the largest ({top}): {missing}"
    # the largest parameter is the depth's, not an accident of a tame set
    assert top >= {8: 6, 16: 15 if (ch == 2 and stereo) else 13, 24: 23, 32: 29}[bits]


def _param_cap(bps, max_param):
    """The largest parameter rice.calcParams may select: its search runs over 0 .. cap - 1."""
    return min(max_param, 30 if bps > 16 else 14) - 1


@pytest.mark.parametrize("po,pm", ec.CAPS)
@pytest.mark.parametrize("ch,bits,stereo", CAP_CONFIGS)
def test_floors_under_caps(ch, bits, stereo, po, pm):
    fs = ec.cap_subset(ch, bits)
    assert len(fs) <= 120
    free = [ec.oracle(ch, bits, name, x, stereo=stereo) for name, x in fs]
    capped = [ec.oracle(ch, bits, name, x, stereo=stereo, part_order=po, param=pm) for name, x in fs]
    T, T0 = ec.tally([r for _, r in capped]), ec.tally([r for _, r in free])
    assert max(k[2] for k in T if k[:2] == ("full", "po")) == po
    assert T[("full", "po", po)] >= FLOOR, "partition order at the cap"
    if pm < 30:
        # the largest parameter the cap allows at the configuration's widest subframe (the side of a
        # decorrelated pair has one bit more); the uncapped choice on the same frames goes past it
        want = _param_cap(bits + (1 if ch == 2 and stereo else 0), pm)
        assert _max_param(T0) >= want
        assert _max_param(T) == want
        assert T[("full", "param", want)] >= 2, f"parameter {want} at the cap"
        if ch == 2 and stereo and bits == 16:  # left / right / mid stop at 14 whatever the side may take
            assert T[("full", "param", min(pm, 14) - 1)] >= 2
    else:  # 30 is the default: the depth's own limit (14 at 16 bits and below) is the only one
        assert _max_param(T) <= _max_param(T0)
        if bits > 16:
            # 29 is out of a 16-bit signal's reach, and a 17-bit side's 15 needs small partitions.  At
            # the wider depths the full-scale ladder frames keep the subset's largest parameter under
            # any partition-order cap: 29, the cap itself, at 32 bits; 22 at 24 bits (full-scale
            # white noise; 23 takes first differences of full-scale steps, outside this subset)
            want = {24: 22, 32: 29}[bits]
            assert _max_param(T0) == want == _max_param(T)
            assert T[("full", "param", want)] >= 2, f"parameter {want}, the largest the cap allows"
    rate = ec.RATE[(ch, bits)]
    for (name, x), (frame, _) in zip(fs, capped):  # every capped frame is well-formed
        dec, _ = oracle_ref.decode_frames(frame, ch, bits, rate, ec.N)
        assert dec == ec.pcm_bytes(x, bits), name
    same = sum(a[0] == b[0] for a, b in zip(free, capped))
    assert same >= FLOOR, "frames the cap does not bind"
    if po < 8 or pm < (30 if bits > 16 or (ch == 2 and stereo) else 14):  # else the caps are the defaults
        assert len(fs) - same >= FLOOR, "frames the cap binds"
    else:
        assert same == len(fs)


@pytest.mark.parametrize("ch,bits", ec.CONFIGS)
def test_tails_reach_every_partition_order_the_cap_allows(ch, bits):
    ts = ec.tails(ch, bits)
    assert sorted({len(x) for _, x in ts}) == sorted(ec.TAIL_LENGTHS)
    got = {n: set() for n in ec.TAIL_LENGTHS}
    recs = []
    for name, x in ts:
        rec = ec.oracle(ch, bits, name, x)[1]
        recs.append((len(x), rec))
        got[len(x)] |= {rec.written[i].part_order for i in range(rec.n_sub) if rec.written[i].type >= 2}
    T = ec.tally(recs)
    assert T[("tail", "frames")] == len(ts) and not any(k[0] == "full" for k in T)
    # 8 bits: one-sample partitions (16 at order 4, 32 at 5, 256 at 8) are the one class the
    # restatement does not choose: a 4-bit parameter per sample costs more than the loudest 8-bit
    # sample saves over sharing its neighbour's (thousands of gated draws per length select none).
    # Partitions of two samples and more are reached, as at every other depth.
    unreached = {16: {4}, 32: {5}, 256: {8}} if bits == 8 else {}
    for n in ec.TAIL_LENGTHS:
        if n <= 5:
            continue  # at or below the warm-up count: present, whatever is chosen
        want = set(ec.allowed_part_orders(n)) - unreached.get(n, set())
        assert want <= got[n], f"length {n}: partition orders never selected: {sorted(want - got[n])}"


def test_part_cap_brackets():
    """The listed lengths bracket each clause of the cap."""
    assert ec.part_cap(2048, 0) == 8 and ec.part_cap(256, 0) == 8                  # the configured order
    assert ec.part_cap(48, 0) == 4 and ec.part_cap(1152, 4) == 7 and ec.part_cap(4032, 1) == 6  # ctz(n)
    assert ec.part_cap(17, 0) == 0 and ec.part_cap(4095, 2) == 0
    assert ec.part_cap(16, 2) == 3 and ec.part_cap(16, 4) == 2 and ec.part_cap(32, 2) == 4  # log2(n) - log2(kw)
    assert ec.part_cap(4, 3) == 0 and ec.part_cap(32, 3) == 3 and ec.part_cap(4, 2) == 1  # n >> P >= kw
    assert ec.part_cap(3072, 4, 3) == 3


@pytest.mark.parametrize("ch,bits,stereo", FLOOR_CONFIGS)
def test_every_stream_decodes_to_the_generator_samples(ch, bits, stereo):
    rate = ec.RATE[(ch, bits)]
    fs = ec.frames(ch, bits)
    pcm = b"".join(ec.pcm_bytes(x, bits) for _, x in fs)
    out, sizes, md5 = oracle_ref.encode_stream(pcm, ch, bits, rate, stereo=stereo)
    # the stream is the frames the records were taken from, one by one
    # (frame numbers from 128 take a second byte in the header)
    assert sizes == [len(ec.oracle(ch, bits, name, x, stereo=stereo)[0]) + (i >= 128)
                     for i, (name, x) in enumerate(fs)]
    dec, dsizes = oracle_ref.decode_frames(out, ch, bits, rate, ec.N * len(fs))
    assert dec == pcm and dsizes == sizes and md5 == hashlib.md5(pcm).digest()
    for name, x in ec.tails(ch, bits):
        frame, _ = ec.oracle(ch, bits, name, x, stereo=stereo)
        dec, _ = oracle_ref.decode_frames(frame, ch, bits, rate, len(x))
        assert dec == ec.pcm_bytes(x, bits), name


def test_generator_is_pinned():
    """The PCM of every set against the committed SHA-256: a numpy that draws other frames fails here
    instead of thinning the coverage silently (`python tests/encode_cases.py` rewrites the pins)."""
    with open(ec.SHA_FILE) as f:
        pinned = json.load(f)
    assert pinned == ec.sha_table()
