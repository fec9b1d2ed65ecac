"""GPU encoder against the CPU restatement on tests/encode_cases.py: frames that reach every fixed
order, partition order, method bit, Rice parameter, escape, wasted-bits, CONSTANT / VERBATIM and
channel-code decision (tests/test_encode_cases_host.py asserts that they do, on the restatement
alone).  Every case compares the whole stream's bytes, the per-frame sizes and -- on the
configurations without LPC -- the decision record of every candidate, the losing ones included, so a
wrong estimate that happens not to win still fails.  Records exist for every configuration here,
the 8-channel ones (analysed in channel halves) and block sizes other than 4096 included; the
LPC-on cases compare bytes and sizes only.
"""
import hashlib

import numpy as np
import pytest

import encode_cases as ec
import oracle_ref
from test_gpu_parity import _diff_msg, assert_record_matches
from test_gpu_plan import _layout, _run_plan

pytestmark = pytest.mark.gpu

MAX_FRAMES = 256
# (channels, bits, stereo decorrelation)
CONFIGS = [(2, 16, True), (2, 16, False), (1, 16, True), (3, 16, True), (2, 24, True), (2, 32, True),
           (8, 24, True), (1, 8, True)]
CAP_CONFIGS = [(2, 16, True), (2, 16, False), (1, 16, True), (3, 16, True), (2, 32, True), (8, 24, True)]

_encoders = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for e in _encoders.values():
        e.close()
    _encoders.clear()


def _encoder(ch, bits, **kw):
    """One context per setting, kept for the module (as gpu_encoder of test_gpu_parity does)."""
    import flacgpu

    key = (ch, bits, tuple(sorted(kw.items())))
    if key not in _encoders:
        _encoders[key] = flacgpu.Encoder(ch, bits, ec.RATE[(ch, bits)], max_frames=MAX_FRAMES, **kw)
    return _encoders[key]


def _fresh(ch, bits, **kw):
    import flacgpu

    return flacgpu.Encoder(ch, bits, ec.RATE[(ch, bits)], max_frames=MAX_FRAMES, **kw)


def _oracle_kw(kw):
    names = {"stereo_decorrelation": "stereo", "max_rice_part_order": "part_order", "max_rice_param": "param",
             "lpc_order": "lpc", "block_size": "block"}
    return {names[k]: v for k, v in kw.items()}


def _check(enc, ch, bits, fs, records=True, **kw):
    """Encode the frames `fs` ([(name, samples)], every one but the last a whole block) as one
    stream; bytes, sizes and records against the restatement.  Returns the stream's bytes."""
    okw = _oracle_kw(kw)
    block = okw.get("block", ec.N)
    assert len(fs) <= 2 * MAX_FRAMES and all(len(x) == block for _, x in fs[:-1]) and len(fs[-1][1]) <= block
    pcm = b"".join(ec.pcm_bytes(x, bits) for _, x in fs)
    ref, ref_sizes, _ = oracle_ref.encode_stream(pcm, ch, bits, ec.RATE[(ch, bits)], **okw)
    recs = None
    if records:
        enc.set_records(True)
    try:
        got, sizes = enc.encode_frames(pcm)
        if records:
            recs = enc.records()
    finally:
        if records:
            enc.set_records(False)
    for i, (a, b) in enumerate(zip(sizes, ref_sizes)):
        assert a == b, f"frame {i} ({fs[i][0]}): {a} bytes, the restatement {b}"
    assert sizes == ref_sizes
    assert got == ref, _diff_msg(got, ref)
    if records:
        assert len(recs) == len(fs)
        for i, (name, x) in enumerate(fs):
            assert_record_matches(recs[i], ec.oracle(ch, bits, name, x, **okw)[1], f"frame {i} ({name})")
    return got


def _check_tails(enc, ch, bits, ts, records=True, **kw):
    """Each tail as the last frame of a stream of its own, behind one full frame."""
    full = ec.frames(ch, bits)
    out = []
    for i, t in enumerate(ts):
        out.append(_check(enc, ch, bits, [full[(7 * i) % len(full)], t], records, **kw))
    return out


def _kw(stereo, **kw):
    return dict(kw) if stereo else dict(kw, stereo_decorrelation=False)


# ---- the default configuration
@pytest.mark.parametrize("ch,bits,stereo", CONFIGS)
def test_full_frames(ch, bits, stereo):
    kw = _kw(stereo)
    _check(_encoder(ch, bits, **kw), ch, bits, ec.frames(ch, bits), **kw)


@pytest.mark.parametrize("ch,bits,stereo", CONFIGS)
def test_tails(ch, bits, stereo):
    kw = _kw(stereo)
    _check_tails(_encoder(ch, bits, **kw), ch, bits, ec.tails(ch, bits), **kw)


# ---- the other pack kernels: the same streams, the same bytes
@pytest.mark.parametrize("knob,value,ch,bits", [("FLACGPU_PACK4", "0", 2, 16),       # 2ch16 through k_pack
                                                 ("FLACGPU_PACK_SPLIT", "0", 8, 24),  # 8ch24 through whole-frame k_packw
                                                 ("FLACGPU_PACKW", "1", 2, 24)])      # 2ch24 forced onto k_packw
def test_kernel_variants(monkeypatch, knob, value, ch, bits):
    fs, ts = ec.frames(ch, bits), ec.tails(ch, bits)
    default = _encoder(ch, bits)
    want = [_check(default, ch, bits, fs, records=False)] + _check_tails(default, ch, bits, ts, records=False)
    monkeypatch.setenv(knob, value)
    with _fresh(ch, bits) as enc:
        got = [_check(enc, ch, bits, fs)] + _check_tails(enc, ch, bits, ts)
    assert got == want


# ---- the Rice caps
@pytest.mark.parametrize("po,pm", ec.CAPS)
@pytest.mark.parametrize("ch,bits,stereo", CAP_CONFIGS)
def test_rice_caps(ch, bits, stereo, po, pm):
    kw = _kw(stereo, max_rice_part_order=po, max_rice_param=pm)
    with _fresh(ch, bits, **kw) as enc:
        _check(enc, ch, bits, ec.cap_subset(ch, bits), **kw)
        _check_tails(enc, ch, bits, ec.pow2_tails(ch, bits), **kw)


# ---- uniform blocks other than 4096: every frame on the kernels' general (not full-frame) path
@pytest.mark.parametrize("block", [4096, 2048, 1152, 256, 16])
@pytest.mark.parametrize("ch,bits", [(2, 16), (2, 24)])
def test_block_sizes(ch, bits, block):
    fs = [(name, x[:block]) for name, x in ec.frames(ch, bits)]
    kw = {"block_size": block} if block != 4096 else {}
    with _fresh(ch, bits, **kw) as enc:
        _check(enc, ch, bits, fs, **kw)


# ---- LPC on: 2ch16 leaves k_pack4, and every fixed order 0..4 is a rival of the LPC orders
@pytest.mark.parametrize("ch,bits", [(2, 16), (2, 24)])
def test_lpc_on(ch, bits):
    with _fresh(ch, bits, lpc_order=8) as enc:
        _check(enc, ch, bits, ec.frames(ch, bits), records=False, lpc_order=8)


# ---- the device-resident plan path (the one bench.py times)
@pytest.mark.parametrize("ch,bits", [(2, 16), (8, 24)])
def test_plan_path(ch, bits):
    """The frame set as 16 streams of ragged lengths, cut at non-multiples of 4096 so the frames
    re-block: bytes, sizes and MD5 of every stream."""
    rate = ec.RATE[(ch, bits)]
    fb = ch * (bits // 8)
    pcm = b"".join(ec.pcm_bytes(x, bits) for _, x in ec.frames(ch, bits))
    total = len(pcm) // fb
    rng = np.random.Generator(np.random.PCG64([909, ch, bits]))
    cuts = sorted({int(c) for c in rng.integers(1, total, size=15)} | {0, total})
    lengths = [b - a for a, b in zip(cuts, cuts[1:])]
    assert sum(lengths) == total and any(n % ec.N for n in lengths)
    offs, size = _layout(lengths, fb, (0, 4, 8, 12))
    buf = bytearray(size)
    pcms = []
    for s, (a, n) in enumerate(zip(cuts, lengths)):
        pcms.append(pcm[a * fb:(a + n) * fb])
        buf[offs[s]:offs[s] + n * fb] = pcms[-1]
    res, _ = _run_plan(_encoder(ch, bits), bytes(buf), offs, lengths)
    for s, (got, sizes, md5) in enumerate(res):
        ref, ref_sizes, ref_md5 = oracle_ref.encode_stream(pcms[s], ch, bits, rate)
        assert sizes == ref_sizes, f"stream {s}: frame sizes differ"
        assert got == ref, f"stream {s}: " + _diff_msg(got, ref)
        assert md5 == ref_md5 == hashlib.md5(pcms[s]).digest(), f"stream {s}: MD5"
