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

pytestmark = pytest.mark.gpu

CH, BITS, RATE, BLOCK, PER = 2, 16, 44100, 256, 4
FRAMES = [64, 1, 3, 70, 0]
SHORT_LAST = {2: 100}  # file 2's last frame has 100 samples
GUARD = 5  # table entries before the first slice, between two slices and after the last
FILL64 = 0xA5A5A5A5A5A5A5A5
NONE = 0xFFFFFFFF
DEC_RANGE = 7


def _torch():
    import torch

    return torch, torch.device("cuda", 0)


def _samples(i):
    n = FRAMES[i] * BLOCK
    return n - (BLOCK - SHORT_LAST[i]) if i in SHORT_LAST else n


def _blocks(i):
    b = [BLOCK] * FRAMES[i]
    if i in SHORT_LAST:
        b[-1] = SHORT_LAST[i]
    return b


@pytest.fixture(scope="module")
def files():
    """[(flac file, its PCM)], made once by the encoder on the GPU."""
    import flacgpu

    pcms = [synth.synth_pcm(_samples(i), CH, BITS, RATE, stream=10 + i) if FRAMES[i] else b"" for i in range(len(FRAMES))]
    with flacgpu.Encoder(CH, BITS, RATE, device=0, max_frames=128, block_size=BLOCK) as enc:
        flacs = enc.encode_files(pcms)
    assert [len(flacgpu.flac_index(f)[2]) for f in flacs] == FRAMES
    return list(zip(flacs, pcms))


@pytest.fixture(scope="module")
def ctx():
    import flacgpu

    with flacgpu.Decoder(CH, BITS, RATE, device=0, max_frames=64, block_size=BLOCK) as d:
        yield d


def _bare(flac):
    import flacgpu

    return flac[flacgpu.flac_index(flac)[1]:]


class Resident:
    """Streams [(bare frames, bits, rate)] at odd offsets of one device buffer, indexed and their
    positions scanned once; the tables stay on the device for any number of window calls."""

    def __init__(self, d, streams):
        import flacgpu

        torch, dev = _torch()
        self.d, self.n = d, len(streams)
        blob, self.offs = bytearray(b"\xA5" * 3), []
        for data, _, _ in streams:
            if len(blob) % 2 == 0:
                blob += b"\xA5"
            self.offs.append(len(blob))
            blob += data
        blob += b"\xA5" * 16
        self.caps = [len(s[0]) // 8 + 1 for s in streams]
        self.first, at = [], GUARD
        for c in self.caps:
            self.first.append(at)
            at += c + GUARD
        self.entries = at
        self.st = torch.cuda.current_stream(dev).cuda_stream
        self.d_buf = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
        self.d_off = torch.full((8 * at,), 0xA5, dtype=torch.uint8, device=dev)
        self.d_fb = torch.full((4 * at,), 0xA5, dtype=torch.uint8, device=dev)
        self.d_ires = torch.full((16 * self.n,), 0xA5, dtype=torch.uint8, device=dev)
        self.d_pos = torch.full((8 * at,), 0xA5, dtype=torch.uint8, device=dev)  # poisoned
        self.d_tot = torch.full((8 * self.n,), 0xA5, dtype=torch.uint8, device=dev)
        bits, rates = [s[1] for s in streams], [s[2] for s in streams]
        d.flac_index_streams_device(self.d_buf.data_ptr(), self.offs, [len(s[0]) for s in streams], self.first, self.caps,
                                    self.d_off.data_ptr(), self.d_fb.data_ptr(), self.d_ires.data_ptr(), stream_bits=bits,
                                    stream_rates=rates, stream=self.st)
        d.flac_positions_streams_device(self.d_buf.data_ptr(), self.first, self.caps, self.d_off.data_ptr(),
                                        self.d_fb.data_ptr(), self.d_ires.data_ptr(), self.d_pos.data_ptr(),
                                        self.d_tot.data_ptr(), stream_bits=bits, stream_rates=rates, stream=self.st)
        d.sync_check(self.st)
        self.index = [(r.status, r.n_frames) for r in
                      (flacgpu.IndexResult * self.n).from_buffer_copy(self.d_ires.cpu().numpy().tobytes())]
        self.pos = np.frombuffer(self.d_pos.cpu().numpy().tobytes(), dtype=np.uint64)
        self.totals = [int(v) for v in np.frombuffer(self.d_tot.cpu().numpy().tobytes(), dtype=np.uint64)]

    def positions(self, s):
        return [int(v) for v in self.pos[self.first[s]:self.first[s] + self.index[s][1]]]

    def decode(self, windows, offsets, caps, size):
        """One flacgpu_decode_windows_device call into a 0xA5-filled buffer of `size` bytes ->
        (the buffer's bytes, [WindowResult])."""
        import flacgpu

        torch, dev = _torch()
        n = len(windows)
        d_out = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
        assert d_out.data_ptr() % 16 == 0
        d_res = torch.full((32 * n,), 0xA5, dtype=torch.uint8, device=dev)
        self.d.decode_windows_device(self.d_buf.data_ptr(), self.first, self.d_off.data_ptr(), self.d_fb.data_ptr(),
                                     self.d_ires.data_ptr(), self.d_pos.data_ptr(), self.d_tot.data_ptr(), windows,
                                     d_out.data_ptr(), offsets, caps, d_res.data_ptr(), stream=self.st)
        self.d.sync_check(self.st)
        res = list((flacgpu.WindowResult * n).from_buffer_copy(d_res.cpu().numpy().tobytes()))
        return d_out.cpu().numpy().tobytes(), res


def cover(blocks, start, count):
    """(first covering frame, covering frames, samples delivered) by a plain loop."""
    total = sum(blocks)
    take = min(count, max(total - start, 0))
    hit, at = [], 0
    for i, b in enumerate(blocks):
        if take and at + b > start and at < start + take:
            hit.append(i)
        at += b
    return (hit[0] if hit else 0, len(hit), take)


def odd_layout(sizes, gaps=(7, 9, 13, 3, 11, 5, 15, 1)):
    """Regions of the given sizes at odd offsets with odd gaps between them -> ([offset], total)."""
    offs, at = [], 1
    for k, n in enumerate(sizes):
        if at % 2 == 0:
            at += 1
        offs.append(at)
        at += n + gaps[k % len(gaps)]
    return offs, at + 16


def check_windows(out, res, windows, blocks_of, pcm_of, per, offsets, caps, expect_status=None):
    """Every result and every byte of the output buffer, for windows whose expected status is OK
    but for those in expect_status {window: (status, first_bad_frame, first_bad_status)}."""
    expect_status = expect_status or {}
    want = bytearray(b"\xA5" * len(out))
    for w, ((s, start, count), r) in enumerate(zip(windows, res)):
        first, frames, take = cover(blocks_of[s], start, count)
        if w in expect_status:
            st, bad, bad_st = expect_status[w]
            assert (r.status, r.n_samples, r.first_bad_frame, r.first_bad_status) == (st, 0, bad, bad_st), w
            continue
        assert (r.status, r.n_samples, r.n_frames, r.first_bad_frame, r.first_bad_status) == (0, take, frames, NONE, 0), w
        if frames:
            assert r.first_frame == first, w
        assert take * per <= caps[w]
        want[offsets[w]:offsets[w] + take * per] = pcm_of[s][start * per:(start + take) * per]
    assert out == bytes(want)  # the delivered bytes, and 0xA5 everywhere else


@pytest.fixture(scope="module")
def resident(ctx, files):
    return Resident(ctx, [(_bare(f), BITS, RATE) for f, _ in files])


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


def _grammar_call(c, windows, offsets_of, block_size=4096, expect_status=None):
    """The grammar case as the one stream of a context of its own; windows [(0, start, count)]."""
    import flacgpu

    per = c["channels"] * (c["bits"] // 8)
    blocks = [f["block"] for f in c["frames"]]
    with flacgpu.Decoder(c["channels"], c["bits"], c["rate"], device=0, max_frames=64, block_size=block_size) as d:
        r = Resident(d, [(fg.case_bytes(c), c["bits"], c["rate"])])
        assert r.index == [(0, len(blocks))] and r.totals == [sum(blocks)]
        assert r.positions(0) == [sum(blocks[:k]) for k in range(len(blocks))]
        sizes = [cover(blocks, s, n)[2] * per for _, s, n in windows]
        offs, size = offsets_of(sizes)
        out, res = r.decode(windows, offs, sizes, size)
    if expect_status is None:
        assert [x.status for x in res] == [0] * len(windows)
    check_windows(out, res, windows, {0: blocks}, {0: fg.case_pcm(c)}, per, offs, sizes, expect_status=expect_status)
    return res


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
    _grammar_call(c, windows, lambda sizes: (dst, 64 * len(dst) + 64))


def test_24_bit_mono():
    c = _case("waste_and_unary")  # blocks 128, 192, 1152, 256, 100; per = 3
    windows = [(0, 0, 1828), (0, 127, 2), (0, 5, 7), (0, 319, 1153), (0, 1700, 500), (0, 1471, 2), (0, 1828, 3)]
    _grammar_call(c, windows, odd_layout)


def test_eight_channels_32_bit():
    c = _case("eight_by_32")  # blocks 1000, 4096, 17; per = 32: a checking and a writing pass of two rounds
    windows = [(0, 999, 2), (0, 0, 5113), (0, 5095, 100), (0, 1003, 10), (0, 3, 1)]
    _grammar_call(c, windows, odd_layout)


def test_frames_outside_a_window_are_not_decoded():
    """The third frame (1152 samples) is above the context's block size of 256.  A window before it
    and one after it deliver the generator's samples -- the later one only if the oversized frame's
    samples were counted; a window that touches it is BAD_FRAME and writes nothing."""
    c = _case("waste_and_unary")
    assert [f["block"] for f in c["frames"]] == [128, 192, 1152, 256, 100]
    windows = [(0, 100, 220), (0, 1482, 300), (0, 300, 100), (0, 320, 1), (0, 1471, 1), (0, 1472, 356)]
    res = _grammar_call(c, windows, odd_layout, block_size=256,
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
