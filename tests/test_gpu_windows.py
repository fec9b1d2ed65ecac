"""The sample-window decode on the GPU: flacgpu_flac_positions_streams_device,
flacgpu_decode_windows_device and flacgpu_decode_files_windows.

Everything compares bytes for equality.  The expected bytes are the generators' own PCM
(synth.synth_pcm for the encoded files, frame_grammar.case_pcm for the grammar streams), sliced
here; they are never another output of the decoder.  The files are those of
test_gpu_decode_files.py: stereo 16-bit, blocks of 256, [64, 1, 3, 70, 0] frames, decoded by a
context that holds 64 frames per call, so the covering frames of one call cross chunk boundaries."""
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import frame_grammar as fg  # noqa: E402
import synth  # noqa: E402
from window_helpers import (BITS, BLOCK, CH, FRAMES, GUARD, NONE, PER, RATE, Resident, _bare, _blocks, _samples,  # noqa: E402
                            _torch, check_windows, cover, grammar_call, odd_layout)
from window_helpers import ctx, files, resident  # noqa: E402,F401  (fixtures: the five stereo 16-bit files)

pytestmark = pytest.mark.gpu

FILL64 = 0xA5A5A5A5A5A5A5A5
DEC_RANGE = 7


def test_positions_are_the_prefix_sums(resident):
    assert resident.index == [(0, n) for n in FRAMES]
    owned = np.zeros(resident.entries, dtype=bool)
    for i in range(len(FRAMES)):
        b = _blocks(i)
        assert resident.positions(i) == [sum(b[:k]) for k in range(len(b))], i
        assert resident.totals[i] == _samples(i), i
        owned[resident.first[i]:resident.first[i] + FRAMES[i]] = True
    assert (resident.pos[~owned] == FILL64).all()  # the guard entries and those past every n_frames


def test_invalid_index_leaves_its_slice_alone(ctx, files):
    bad = b"\x00" * 7 + _bare(files[1][0])  # no frame at offset 0
    r = Resident(ctx, [(_bare(files[1][0]), BITS, RATE), (bad, BITS, RATE), (_bare(files[2][0]), BITS, RATE)])
    assert r.index == [(0, 1), (1, 0), (0, 3)]
    assert r.totals == [_samples(1), 0, _samples(2)]
    assert r.positions(0) == [0] and r.positions(2) == [0, 256, 512]
    assert (r.pos[r.first[1] - GUARD:r.first[1] + r.caps[1] + GUARD] == FILL64).all()
    # its windows are BAD_INDEX and write nothing; the neighbours' are delivered
    windows = [(0, 10, 100), (1, 0, 100), (2, 300, 300)]
    offs, size = odd_layout([400, 400, 1200])
    out, res = r.decode(windows, offs, [400, 400, 1200], size)
    blocks_of = {0: _blocks(1), 1: [], 2: _blocks(2)}
    check_windows(out, res, windows, blocks_of, {0: files[1][1], 2: files[2][1]}, PER, offs, [400, 400, 1200],
                  expect_status={1: (1, NONE, 0)})


def forty_windows():
    w = [
        (0, 300, 50),                 # inside one frame
        (0, 512, 256),                # exactly one frame
        (0, 767, 2),                  # the last sample of a frame and the first of the next
        (0, 0, _samples(0)),          # a whole file
        (2, 500, 1000),               # clipped by the end of the file with the short last frame
        (2, _samples(2), 10),         # at the end
        (2, _samples(2) + 88, 10),    # past the end
        (2, 5, 0),                    # no samples
        (3, 1000, 5000), (3, 3000, 5000), (3, 4000, 9000),  # three overlapping windows
        (4, 0, 100),                  # the file with no frames
        (1, 0, 256), (1, 255, 1), (1, 0, (1 << 64) - 1), (2, 511, (1 << 64) - 1),
    ]
    rng = random.Random("windows")
    while len(w) < 40:
        s = rng.choice((0, 1, 2, 3))
        start = rng.randrange(_samples(s))
        w.append((s, start, rng.choice((1, 2, 255, 256, 257, 700))))
    return w


def test_forty_windows_in_one_call(resident, files):
    windows = forty_windows()
    blocks_of = {i: _blocks(i) for i in range(len(FRAMES))}
    pcm_of = {i: files[i][1] for i in range(len(FRAMES))}
    takes = [cover(blocks_of[s], start, count) for s, start, count in windows]
    assert sum(t[1] for t in takes) > 128  # the cut of the covering frames crosses two chunk boundaries
    sizes = [t[2] * PER for t in takes]
    offs, size = odd_layout(sizes)
    assert all(o % 2 == 1 for o in offs) and len({o % 16 for o in offs}) >= 6
    out, res = resident.decode(windows, offs, sizes, size)
    assert [r.status for r in res] == [0] * len(windows)
    assert sum(r.n_frames for r in res) == sum(t[1] for t in takes)
    check_windows(out, res, windows, blocks_of, pcm_of, PER, offs, sizes)
    assert [r.n_samples for r in res[4:8]] == [112, 0, 0, 0] and res[11].n_samples == 0 and res[11].n_frames == 0


def test_capacity_one_byte_short(resident, files):
    windows = [(0, 100, 300), (3, 4000, 600), (1, 3, 200)]
    sizes = [300 * PER, 600 * PER - 1, 200 * PER]
    offs, size = odd_layout(sizes)
    out, res = resident.decode(windows, offs, sizes, size)
    assert [r.status for r in res] == [0, 3, 0]
    check_windows(out, res, windows, {i: _blocks(i) for i in range(5)}, {i: files[i][1] for i in range(5)}, PER, offs, sizes,
                  expect_status={1: (3, NONE, 0)})


def _case(name):
    return next(c for c in fg.cases() if c["name"] == name)


def test_alignment_sweep_mono_8_bit():
    """per = 1: a window for every (source mod 16, destination mod 16) pair at lengths 1, 15, 16, 17
    and 47.  The source of a copy starts `skip` bytes into 16-byte aligned scratch, and skip = start
    here (frame 0), so start mod 16 is the source alignment; the longest windows run on into frame 1."""
    c = _case("seed3_1x8")
    assert [f["block"] for f in c["frames"]][:2] == [1152, 1024]
    windows, dst = [], []
    for sa in range(16):
        for da in range(16):
            for n in (1, 15, 16, 17, 47):
                start = 1104 + sa
                assert start % 16 == sa
                windows.append((0, start, n))
                dst.append(64 * len(dst) + da)
    assert len(windows) == 1280 and any(s + n > 1152 for _, s, n in windows)
    grammar_call(c, windows, lambda sizes: (dst, 64 * len(dst) + 64))


def test_24_bit_mono():
    c = _case("waste_and_unary")  # blocks 128, 192, 1152, 256, 100; per = 3
    windows = [(0, 0, 1828), (0, 127, 2), (0, 5, 7), (0, 319, 1153), (0, 1700, 500), (0, 1471, 2), (0, 1828, 3)]
    grammar_call(c, windows, odd_layout)


def test_eight_channels_32_bit():
    c = _case("eight_by_32")  # blocks 1000, 4096, 17; per = 32: a checking and a writing pass of two rounds
    windows = [(0, 999, 2), (0, 0, 5113), (0, 5095, 100), (0, 1003, 10), (0, 3, 1)]
    grammar_call(c, windows, odd_layout)


def test_frames_outside_a_window_are_not_decoded():
    """The third frame (1152 samples) is above the context's block size of 256.  A window before it
    and one after it deliver the generator's samples -- the later one only if the oversized frame's
    samples were counted; a window that touches it is BAD_FRAME and writes nothing."""
    c = _case("waste_and_unary")
    assert [f["block"] for f in c["frames"]] == [128, 192, 1152, 256, 100]
    windows = [(0, 100, 220), (0, 1482, 300), (0, 300, 100), (0, 320, 1), (0, 1471, 1), (0, 1472, 356)]
    res = grammar_call(c, windows, odd_layout, block_size=256,
                        expect_status={2: (2, 2, DEC_RANGE), 3: (2, 2, DEC_RANGE), 4: (2, 2, DEC_RANGE)})
    assert [r.status for r in res] == [0, 0, 2, 2, 2, 0]
    assert (res[0].first_frame, res[0].n_frames) == (0, 2) and (res[1].first_frame, res[1].n_frames) == (3, 2)


def test_decode_files_windows(ctx, files):
    flacs = [f for f, _ in files]
    for f, pcm in files:
        assert ctx.decode_file(f) == (pcm, True)
    windows = [(0, 300, 50), (3, 255, 2), (3, 0, _samples(3)), (2, 500, 1000), (4, 0, 10), (1, 17, 100), (0, 16000, 5000),
               (2, 700, 1), (1, 0, 0)]
    got = ctx.decode_files_windows(flacs, windows, guard=64)
    assert [g[0] for g in got] == [0] * len(windows)
    for (i, start, count), (st, pcm, guard) in zip(windows, got):
        whole = ctx.decode_file(flacs[i])[0]
        assert whole == files[i][1]
        n = min(count, max(_samples(i) - start, 0))
        assert pcm == whole[start * PER:(start + n) * PER], (i, start, count)
        assert guard == b"\xA5" * 64
    # one byte short: that window alone
    caps = [w[2] * PER for w in windows]
    caps[1] -= 1
    got = ctx.decode_files_windows(flacs, windows, guard=64, pcm_caps=caps)
    assert [g[0] for g in got] == [0, -4] + [0] * (len(windows) - 2)
    assert got[1][1] == b"" and got[1][2] == b"\xA5" * 64 and got[2][1] == files[3][1]


def test_decode_files_windows_bad_files(ctx, files):
    import flacgpu

    pcm24 = synth.synth_pcm(300, CH, 24, RATE, stream=3)
    with flacgpu.Encoder(CH, 24, RATE, device=0, max_frames=64, block_size=BLOCK) as enc:
        other = enc.encode_file(pcm24)
    first = flacgpu.flac_index(files[3][0])[1]
    bad = bytearray(files[3][0])
    bad[first + 40] ^= 0x10  # inside the body of the damaged file's first frame
    flacs = [files[0][0], other, bytes(bad), files[2][0], b"fLaX"]
    windows = [(0, 10, 700), (1, 0, 100), (2, 5000, 100), (3, 100, 500), (2, 0, 10), (0, 16383, 1), (4, 0, 1)]
    got = ctx.decode_files_windows(flacs, windows, guard=16)
    assert [g[0] for g in got] == [0, -2, -2, 0, -2, 0, -2]
    assert got[0][1] == files[0][1][10 * PER:710 * PER] and got[3][1] == files[2][1][100 * PER:600 * PER]
    assert got[5][1] == files[0][1][16383 * PER:]
    for st, pcm, guard in got:
        assert guard == b"\xA5" * 16 and (st == 0 or pcm == b"")
