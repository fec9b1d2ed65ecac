"""The levels of sample windows on the GPU: flacgpu_levels_windows_device, FlacBank.levels and
FlacBank.crop_levels.

Everything compares bit patterns for equality -- the energies as uint64 views of the doubles --
and there is no tolerance: the rule is exact but for one rounding, which Python's float(int) makes
the same way.  The expectations are the generators' own PCM (synth.synth_pcm for the five stereo
files, the arrays the small banks were built from) reduced with numpy and Python integers; they are
never an output of the decoder.  Every output array is filled with 0xA5 before the call and
compared whole, so a stray write anywhere fails."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_gpu_deliver import _break_first_frame, _case, ints  # noqa: E402
from window_helpers import (BITS, CH, FRAMES, NONE, RATE, Resident, _bare, _blocks, _samples, _torch, cover, odd_layout)  # noqa: E402
from window_helpers import ctx, files, resident  # noqa: E402,F401  (fixtures: the five stereo 16-bit files)
import frame_grammar as fg  # noqa: E402

pytestmark = pytest.mark.gpu

HOPS = [1, 3, 64, 255, 256, 257, 1000, 1024, 1025, 5000, 17920]
A5_32, A5_64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def f64_bits(values):
    """Python integers -> the bit patterns of float(v), which is correctly rounded to nearest-even."""
    return np.array([float(int(v)) for v in values], dtype=np.float64).view(np.uint64)


def reference(x, hop):
    """(peak uint32, sum int64, energy bits uint64), each [blocks, C], of the samples x [n, C]."""
    n, C = x.shape
    blocks = (n + hop - 1) // hop
    if n == 0:
        return np.zeros((0, C), np.uint32), np.zeros((0, C), np.int64), np.zeros((0, C), np.uint64)
    x = x.astype(np.int64)
    at = np.arange(0, n, hop)
    peak = np.maximum.reduceat(np.abs(x), at, axis=0).astype(np.uint32)
    total = np.add.reduceat(x, at, axis=0)
    if int(np.abs(x).max()) < (1 << 23) + 1 and hop <= (1 << 16):  # squares below 2^46 + ..., 2^16 of them: inside int64
        sq = np.add.reduceat(x * x, at, axis=0).reshape(-1)
    else:
        sq = [sum(int(v) * int(v) for v in x[j * hop:(j + 1) * hop, c]) for j in range(blocks) for c in range(C)]
    return peak, total, f64_bits(sq).reshape(blocks, C)


@pytest.fixture(scope="module")
def file_ints(files):
    out = {i: ints(pcm, CH, BITS) for i, (_, pcm) in enumerate(files)}
    for v in out.values():
        v.setflags(write=False)
    return out


_refs = {}


def shared_reference(file_ints, s, start, take, hop):
    key = (s, start, take, hop)
    if key not in _refs:
        _refs[key] = reference(file_ints[s][start:start + take], hop)
    return _refs[key]


def call(d, tables, st, windows, hop, offsets, caps, records):
    """One flacgpu_levels_windows_device call into 0xA5-filled arrays of `records` records ->
    (peak uint32, sum int64, energy bits uint64, [WindowResult])."""
    import flacgpu

    torch, dev = _torch()
    d_peak = torch.full((4 * records,), 0xA5, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8 * records,), 0xA5, dtype=torch.uint8, device=dev)
    d_energy = torch.full((8 * records,), 0xA5, dtype=torch.uint8, device=dev)
    d_res = torch.full((32 * len(windows),), 0xA5, dtype=torch.uint8, device=dev)
    d.levels_windows_device(*tables, windows, hop, d_peak.data_ptr(), d_sum.data_ptr(), d_energy.data_ptr(), offsets, caps,
                            d_res.data_ptr(), stream=st)
    d.sync_check(st)
    res = list((flacgpu.WindowResult * len(windows)).from_buffer_copy(d_res.cpu().numpy().tobytes()))
    return (d_peak.cpu().numpy().view(np.uint32), d_sum.cpu().numpy().view(np.int64), d_energy.cpu().numpy().view(np.uint64), res)


def check(got, windows, takes, refs, C, offsets, records, silent=()):
    """Every record of the three arrays: the expectation of every window not in `silent`, 0xA5 elsewhere."""
    peak, total, energy, _ = got
    want_p = np.full(records, A5_32, np.uint32)
    want_s = np.full(records, A5_64, np.uint64).view(np.int64)
    want_e = np.full(records, A5_64, np.uint64)
    for w in range(len(windows)):
        if w in silent or takes[w] == 0:
            continue
        p, s, e = refs[w]
        o = offsets[w]
        want_p[o:o + p.size], want_s[o:o + s.size], want_e[o:o + e.size] = p.reshape(-1), s.reshape(-1), e.reshape(-1)
    for name, g, want in (("peak", peak, want_p), ("sum", total, want_s), ("energy", energy, want_e)):
        bad = np.nonzero(g != want)[0]
        assert len(bad) == 0, (name, [(int(i), hex(int(g[i]) & A5_64 | 0), hex(int(want[i]) & A5_64 | 0)) for i in bad[:6]], len(bad))


# ---- the five stereo files -------------------------------------------------------------------------
def windows_of_the_files():
    return [
        (0, 0, _samples(0)),        # a whole file: 64 frames, one chunk
        (0, 777, 5001),             # an odd start
        (3, 17001, 5000),           # clipped by the file's end
        (1, 300, 100),              # starts past the end
        (2, 11, 0),                 # count 0
        (3, 513, 3001), (3, 1001, 3001),  # share a stream and overlap
        (4, 0, 10),                 # the file with no frames
        (2, 1, 611),                # into the short last frame
        (3, 0, _samples(3)),        # 70 frames: the covering frames cross the chunk boundary
        (1, 255, 1),
    ]


@pytest.mark.parametrize("hop", HOPS)
def test_windows_of_the_stereo_files(resident, file_ints, hop):
    windows = windows_of_the_files()
    blocks_of = {i: _blocks(i) for i in range(len(FRAMES))}
    covers = [cover(blocks_of[s], start, count) for s, start, count in windows]
    takes = [c[2] for c in covers]
    assert takes[2] == 919 and takes[3] == takes[4] == takes[7] == 0 and sum(c[1] for c in covers) > 128
    caps = [CH * ((t + hop - 1) // hop) for t in takes]
    offs, records = odd_layout(caps)
    got = call(resident.d, resident._tables(), resident.st, windows, hop, offs, caps, records)
    res = got[3]
    for w, (r, c) in enumerate(zip(res, covers)):
        assert (r.status, r.n_samples, r.n_frames, r.first_bad_frame, r.first_bad_status) == (0, c[2], c[1], NONE, 0), w
    refs = [shared_reference(file_ints, s, start, takes[w], hop) for w, (s, start, _) in enumerate(windows)]
    check(got, windows, takes, refs, CH, offs, records)


def test_capacity_one_record_short_and_bad_index_write_nothing(ctx, resident, files, file_ints):
    windows = [(0, 100, 3000), (3, 4000, 6000), (1, 3, 200)]
    hop = 1000
    takes = [3000, 6000, 200]
    refs = [shared_reference(file_ints, s, start, takes[w], hop) for w, (s, start, _) in enumerate(windows)]
    caps = [3 * CH, 6 * CH - 1, 1 * CH]
    offs, records = odd_layout([c + 1 for c in caps])
    got = call(resident.d, resident._tables(), resident.st, windows, hop, offs, caps, records)
    assert [(r.status, r.n_samples) for r in got[3]] == [(0, 3000), (3, 0), (0, 200)]
    check(got, windows, takes, refs, CH, offs, records, silent={1})
    _, ref = resident.decode(windows, [0, 16384, 65536], [3000 * 4, 6000 * 4 - 1, 200 * 4], 70000)
    assert [_fields(a) for a in got[3]] == [_fields(b) for b in ref]  # the results are the byte call's
    caps[1] += 1  # one record more fits
    got = call(resident.d, resident._tables(), resident.st, windows, hop, offs, caps, records)
    assert [(r.status, r.n_samples) for r in got[3]] == [(0, 3000), (0, 6000), (0, 200)]
    check(got, windows, takes, refs, CH, offs, records)

    bad = b"\x00" * 7 + _bare(files[1][0])  # no frame at offset 0
    r = Resident(ctx, [(_bare(files[1][0]), BITS, RATE), (bad, BITS, RATE), (_bare(files[2][0]), BITS, RATE)])
    assert r.index == [(0, 1), (1, 0), (0, 3)]
    windows = [(0, 10, 100), (1, 0, 100), (2, 300, 600)]
    takes = [100, 0, 312]
    refs = [reference(file_ints[1][10:110], 64), None, reference(file_ints[2][300:612], 64)]
    caps = [2 * CH, 2 * CH, 10 * CH]
    offs, records = odd_layout(caps)
    got = call(r.d, r._tables(), r.st, windows, 64, offs, caps, records)
    assert [(x.status, x.n_samples) for x in got[3]] == [(0, 100), (1, 0), (0, 312)]
    check(got, windows, takes, refs, CH, offs, records, silent={1})


def _fields(r):
    return (r.n_samples, r.first_frame, r.n_frames, r.status, r.first_bad_frame, r.first_bad_status)


def test_bad_frame_writes_nothing():
    """The third frame (1152 samples) is above the context's block size of 256: the windows that touch
    it are BAD_FRAME and write nothing; their neighbours are measured."""
    import flacgpu

    c = _case("waste_and_unary")  # 24-bit mono
    blocks = [f["block"] for f in c["frames"]]
    assert blocks == [128, 192, 1152, 256, 100] and (c["channels"], c["bits"]) == (1, 24)
    x = ints(fg.case_pcm(c), 1, 24)
    windows = [(0, 100, 220), (0, 300, 100), (0, 1482, 300), (0, 320, 1), (0, 1472, 356), (0, 1471, 1), (0, 100, 220)]
    hop = 100
    with flacgpu.Decoder(1, 24, c["rate"], device=0, max_frames=64, block_size=256) as d:
        r = Resident(d, [(fg.case_bytes(c), 24, c["rate"])])
        takes = [cover(blocks, s, n)[2] for _, s, n in windows]
        caps = [(t + hop - 1) // hop for t in takes]
        offs, records = odd_layout(caps)
        got = call(d, r._tables(), r.st, windows, hop, offs, caps, records)
    assert [v.status for v in got[3]] == [0, 2, 0, 2, 0, 2, 0]
    assert [(v.n_samples, v.first_bad_frame) for v in got[3] if v.status == 2] == [(0, 2)] * 3
    refs = [reference(x[s:s + takes[w]], hop) for w, (_, s, _) in enumerate(windows)]
    check(got, windows, takes, refs, 1, offs, records, silent={1, 3, 5})


# ---- other formats: small banks built on the device -------------------------------------------------
def _bank(x, bits):
    """A bank of the one stream x [n, C] (int64), blocks of 256."""
    import flacbank

    torch, _ = _torch()
    return flacbank.FlacBank.from_tensors([torch.from_numpy(np.ascontiguousarray(x.T).astype(np.int32))], 44100, bits=bits,
                                          block_size=256, max_frames=64)


def _measure(b, x, windows, hop):
    torch, dev = _torch()
    C, n = x.shape[1], len(x)
    takes = [max(0, min(count, n - start)) for _, start, count in windows]
    caps = [C * ((t + hop - 1) // hop) for t in takes]
    offs, records = odd_layout(caps)
    st = torch.cuda.current_stream(dev).cuda_stream
    got = call(b._dec, b._tables(), st, windows, hop, offs, caps, records)
    assert [(r.status, r.n_samples) for r in got[3]] == [(0, t) for t in takes]
    refs = [reference(x[s:s + takes[w]], hop) for w, (_, s, _) in enumerate(windows)]
    check(got, windows, takes, refs, C, offs, records)
    return refs


def test_mono_8_bit_every_source_alignment():
    rng = np.random.default_rng(8)
    x = rng.integers(-128, 128, size=(9000, 1), dtype=np.int64)
    x[100:120] = -128
    with _bank(x, 8) as b:
        assert b.samples == [9000]
        # per = 1: start mod 8 is the source alignment of the first tile, (start + 4096 k) of the next
        windows = [(0, 1104 + a, 4200 + a) for a in range(16)] + [(0, 0, 9000), (0, 8999, 5)]
        for hop in (3, 100, 4096, 5000):
            _measure(b, x, windows, hop)


def test_three_channels_24_bit():
    """9 bytes a sample: a tile is 455 samples, not a power of two, and samples straddle words."""
    rng = np.random.default_rng(24)
    x = rng.integers(-(1 << 23), 1 << 23, size=(2000, 3), dtype=np.int64)
    x[7], x[8] = -(1 << 23), (1 << 23) - 1
    with _bank(x, 24) as b:
        windows = [(0, 0, 2000), (0, 1, 1999), (0, 333, 911), (0, 1999, 1)]
        for hop in (1, 50, 64, 454, 455, 456, 2000):
            _measure(b, x, windows, hop)


def test_eight_channels_32_bit_worst_cases():
    rng = np.random.default_rng(32)
    x = rng.integers(-(1 << 31), 1 << 31, size=(1000, 8), dtype=np.int64)
    x[200:300] = -(1 << 31)                       # a run of -2^31 in every channel
    x[400:500:2], x[401:500:2] = -(1 << 31), (1 << 31) - 1  # alternating extremes
    # conditions on the expectation itself, before the device is asked
    whole = [sum(int(v) * int(v) for v in x[:, c]) for c in range(8)]
    run8 = sum(int(v) * int(v) for v in x[200:208, 0])
    assert run8 == 1 << 65 and all(e >= 1 << 64 for e in whole)
    assert any(int(float(e)) != e for e in whole)  # not exactly representable
    with _bank(x, 32) as b:
        windows = [(0, 0, 1000), (0, 200, 8), (0, 199, 102), (0, 400, 100), (0, 3, 997)]
        for hop in (1, 8, 100, 127, 128, 129, 1000):  # per = 32: a tile is 128 samples
            refs = _measure(b, x, windows, hop)
            if hop == 8:
                assert refs[1][2][0, 0] == f64_bits([1 << 65])[0] and refs[1][0][0, 0] == 1 << 31
                assert refs[1][1][0, 0] == -(1 << 34)


def test_stereo_24_bit_full_scale_energy_above_2_53():
    rng = np.random.default_rng(2453)
    x = rng.choice(np.array([-(1 << 23), (1 << 23) - 1], dtype=np.int64), size=(9000, 2))
    x[::7] = rng.integers(-(1 << 23), 1 << 23, size=x[::7].shape)
    e = sum(int(v) * int(v) for v in x[:4096, 0])
    assert e > 1 << 53 and int(float(e)) != e  # 4096 full-scale squares are about 2^58: one rounding is made
    with _bank(x, 24) as b:
        _measure(b, x, [(0, 0, 9000), (0, 5, 8192), (0, 4904, 4096)], 4096)


# ---- FlacBank ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bank(files):
    import flacbank

    with flacbank.FlacBank([f for f, _ in files], device=0, max_frames=64) as b:
        yield b


@pytest.mark.parametrize("hop,span,scratch", [(441, 2000, 40000), (5000, 100, 1), (64, 1 << 20, 1 << 30), (20000, 1, 1 << 30)])
def test_flacbank_levels_over_whole_files(bank, file_ints, hop, span, scratch, monkeypatch):
    torch, _ = _torch()
    made = []
    inner = bank._dec.levels_windows_device
    monkeypatch.setattr(bank._dec, "levels_windows_device", lambda *a, **k: (made.append(len(a[7])), inner(*a, **k))[1])
    lv = bank.levels(hop, span=span, scratch_bytes=scratch)
    win = max(span, hop) // hop * hop
    assert sum(made) == sum((_samples(i) + win - 1) // win for i in range(5))
    if scratch == 40000:
        assert len(made) > 3 and max(made) > 1  # several calls, several windows a call
    if scratch == 1:
        assert set(made) == {1}                  # a call holds one window at least
    assert lv.hop == hop and lv.blocks == [(_samples(i) + hop - 1) // hop for i in range(5)]
    assert lv.first == [sum(lv.blocks[:i]) for i in range(5)]
    assert lv.peak.dtype == torch.int64 and lv.sum.dtype == torch.int64 and lv.energy.dtype == torch.float64
    assert tuple(lv.peak.shape) == tuple(lv.sum.shape) == tuple(lv.energy.shape) == (sum(lv.blocks), CH)
    for i in range(5):
        p, s, e = lv.file(i)
        wp, ws, we = shared_reference(file_ints, i, 0, _samples(i), hop)
        assert (p.cpu().numpy() == wp.astype(np.int64)).all() and (s.cpu().numpy() == ws).all(), i
        assert (e.cpu().numpy().view(np.uint64) == we).all(), i


def test_rms_and_active_on_a_file_with_a_silent_stretch():
    import flacbank

    torch, _ = _torch()
    rng = np.random.default_rng(5)
    x = rng.integers(-20000, 20000, size=(5000, 2), dtype=np.int64)
    x[1000:3500] = 0          # digital silence: blocks 2..5 of 500, and block 6 but for
    x[3000:3500, 0] = 3       # one very quiet channel
    x[4000:4500] = 32767
    with flacbank.FlacBank.from_tensors([torch.from_numpy(np.ascontiguousarray(x.T).astype(np.int32))], 44100, bits=16,
                                        block_size=256, max_frames=64) as b:
        lv = b.levels(500, span=1024)
        db = lv.rms_dbfs(0).cpu().numpy()
        act = lv.active(0, -60.0).cpu().numpy()
        short = b.levels(1500, span=1).rms_dbfs(0).cpu().numpy()  # the last block holds 500 samples
    e = np.array([[float(sum(int(v) ** 2 for v in x[j * 500:(j + 1) * 500, c])) for c in range(2)] for j in range(10)])
    with np.errstate(divide="ignore"):
        want = 10.0 * np.log10(e / 500.0 / 4.0 ** 15)
    assert db.shape == (10, 2) and np.isneginf(db[2:6]).all() and np.isneginf(db[6, 1]) and np.isfinite(db[6, 0])
    finite = np.isfinite(want)
    assert (np.isfinite(db) == finite).all() and np.allclose(db[finite], want[finite], rtol=0, atol=1e-9)  # torch's log10, not the rule
    assert abs(db[8, 0] - 20.0 * np.log10(32767 / 32768)) < 1e-9
    assert act.tolist() == [True, True, False, False, False, False, False, True, True, True]
    last = float(sum(int(v) ** 2 for v in x[4500:, 0]))
    assert short.shape == (4, 2) and abs(short[3, 0] - 10.0 * np.log10(last / 500.0 / 4.0 ** 15)) < 1e-9


CROPS = [(0, 300), (2, 600), (3, 4000), (1, 250), (4, 0), (2, 668), (3, 17919 - 300), (0, 16383), (3, 17920)]


@pytest.mark.parametrize("length", [300, 5000])
def test_crop_levels_against_crops_reduced_by_numpy(bank, file_ints, length):
    torch, _ = _torch()
    file, start = [c[0] for c in CROPS], [c[1] for c in CROPS]
    x, n = bank.crops(file, start, length, dtype=torch.int32, planar=False)
    x = x.cpu().numpy().astype(np.int64)  # [W, length, C]
    assert n == [min(length, max(0, _samples(f) - s)) for f, s in CROPS] and 0 in n
    for strict in (True, False):
        out = bank.crop_levels(file, start, length, strict=strict)
        assert len(out) == (4 if strict else 5) and out[3] == n
        if not strict:
            assert out[4] == [0] * len(CROPS)
        p, s, e = (t.cpu().numpy() for t in out[:3])
        assert p.shape == s.shape == e.shape == (len(CROPS), CH) and p.dtype == np.int64 and e.dtype == np.float64
        for w in range(len(CROPS)):
            crop = x[w, :n[w]]
            assert (crop == file_ints[file[w]][start[w]:start[w] + n[w]]).all()  # the expectation is the generator's PCM
            for c in range(CH):
                col = [int(v) for v in crop[:, c]]
                assert p[w, c] == max([abs(v) for v in col], default=0) and s[w, c] == sum(col), (w, c)
                assert e[w, c].view(np.uint64) == f64_bits([sum(v * v for v in col)])[0], (w, c)
    assert bank.crop_levels([], [], 10)[3] == [] and bank.crop_levels([0], [5], 0)[3] == [0]


def test_crop_levels_names_the_crop_of_a_damaged_file(files):
    import flacbank
    import flacgpu

    damaged = _break_first_frame(files[3][0])
    with flacbank.FlacBank([files[0][0], damaged, files[2][0]], device=0, max_frames=64) as b:
        with pytest.raises(flacgpu.FlacGpuError, match=r"crop 1 \(file 1, start 200\) is BAD_FRAME, frame 0"):
            b.crop_levels([0, 1, 2, 1], [200, 200, 200, 300], 100)
        p, s, e, n, statuses = b.crop_levels([0, 1, 2, 1], [200, 200, 200, 300], 100, strict=False)
        assert statuses == [0, flacgpu.WINDOW_BAD_FRAME, 0, 0] and n == [100, 0, 100, 100]
        assert p[1].tolist() == [0, 0] and s[1].tolist() == [0, 0] and e[1].tolist() == [0.0, 0.0] and p[0].min() > 0
        with pytest.raises(flacgpu.FlacGpuError, match="FlacBank.levels: file 1 from sample 0 is BAD_FRAME"):
            b.levels(256)
