"""What the GPU tests of the sample-window decode share (test_gpu_windows.py, test_gpu_deliver.py,
test_gpu_mix.py, test_gpu_bigblock.py): the five stereo files, the resident streams with poisoned
and guarded tables, and the expectation of the byte call.  A plain module: the fixtures `files`,
`ctx` and `resident` are imported by name by the test modules that use them.

The files are those of test_gpu_decode_files.py: stereo 16-bit, blocks of 256, [64, 1, 3, 70, 0]
frames, decoded by a context that holds 64 frames per call, so the covering frames of one call
cross chunk boundaries."""
import numpy as np
import pytest

import frame_grammar as fg
import synth

CH, BITS, RATE, BLOCK, PER = 2, 16, 44100, 256, 4
FRAMES = [64, 1, 3, 70, 0]
SHORT_LAST = {2: 100}  # file 2's last frame has 100 samples
GUARD = 5  # table entries before the first slice, between two slices and after the last
NONE = 0xFFFFFFFF


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

    def _call(self, windows, size, call):
        import flacgpu

        torch, dev = _torch()
        n = len(windows)
        d_out = torch.full((size,), 0xA5, dtype=torch.uint8, device=dev)
        assert d_out.data_ptr() % 16 == 0
        d_res = torch.full((32 * n,), 0xA5, dtype=torch.uint8, device=dev)
        call(d_out.data_ptr(), d_res.data_ptr())
        self.d.sync_check(self.st)
        res = list((flacgpu.WindowResult * n).from_buffer_copy(d_res.cpu().numpy().tobytes()))
        return d_out.cpu().numpy().tobytes(), res

    def _tables(self):
        return (self.d_buf.data_ptr(), self.first, self.d_off.data_ptr(), self.d_fb.data_ptr(), self.d_ires.data_ptr(),
                self.d_pos.data_ptr(), self.d_tot.data_ptr())

    def deliver(self, windows, fmt, flags, offsets, caps, size):
        """One flacgpu_decode_windows_device_as call into a 0xA5-filled buffer of `size` bytes ->
        (the buffer's bytes, [WindowResult]); offsets and caps in elements."""
        return self._call(windows, size, lambda out, res: self.d.decode_windows_device_as(
            *self._tables(), windows, fmt, flags, out, offsets, caps, res, stream=self.st))

    def decode(self, windows, offsets, caps, size):
        """The byte call, flacgpu_decode_windows_device, the same way; offsets and caps in bytes."""
        return self._call(windows, size, lambda out, res: self.d.decode_windows_device(
            *self._tables(), windows, out, offsets, caps, res, stream=self.st))


@pytest.fixture(scope="module")
def resident(ctx, files):
    return Resident(ctx, [(_bare(f), BITS, RATE) for f, _ in files])


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


def grammar_call(c, windows, offsets_of, block_size=4096, expect_status=None):
    """The grammar case as the one stream of a context of its own, through the byte call; windows
    [(0, start, count)]."""
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
