"""FlacBank: FLAC files kept compressed in device memory, random crops of them as torch tensors.

The files' frames are uploaded once into one uint8 tensor, indexed and their sample positions
scanned once (flacgpu_flac_index_streams_device, flacgpu_flac_positions_streams_device); every
`crops` call then decodes only the frames that hold the requested samples and delivers them as
[crop, channel, time] (or [crop, time, channel]) elements in one pass
(flacgpu_decode_windows_device_as), on the caller's current torch stream.  Plumbing over the C ABI:
there is no CPU path.  A bank takes no locks: one bank per thread, like a context."""
from __future__ import annotations

from typing import Optional, Sequence

import flacgpu

MAX_WINDOWS = 65535  # of one flacgpu_decode_windows_device_as call
WINDOW_STATUS = {flacgpu.WINDOW_BAD_INDEX: "BAD_INDEX", flacgpu.WINDOW_BAD_FRAME: "BAD_FRAME",
                 flacgpu.WINDOW_TOO_SMALL: "TOO_SMALL"}


def _formats():
    import torch

    return {torch.int32: flacgpu.SAMPLE_I32, torch.float32: flacgpu.SAMPLE_F32, torch.float16: flacgpu.SAMPLE_F16,
            torch.bfloat16: flacgpu.SAMPLE_BF16}


class FlacBank:
    def __init__(self, files: Sequence[bytes], device: int = 0, max_frames: int = 4096):
        if len(files) == 0:
            raise ValueError("FlacBank: no files")
        if len(files) > 65535:
            raise ValueError("FlacBank: more than 65535 files")
        infos, bare = [], []
        for i, f in enumerate(files):
            try:
                si, first, _ = flacgpu.flac_index(f)
            except flacgpu.FlacGpuError as e:
                raise ValueError(f"FlacBank: file {i} is not a FLAC file this library indexes ({e})") from None
            if infos and (si.channels, si.bit_depth) != (infos[0].channels, infos[0].bit_depth):
                raise ValueError(f"FlacBank: file {i} has {si.channels} channels of {si.bit_depth} bits, file 0 has "
                                 f"{infos[0].channels} of {infos[0].bit_depth}: one bank holds one channel count and depth")
            infos.append(si)
            bare.append(bytes(f[first:]))
        self._dec = None
        self.channels, self.bits = int(infos[0].channels), int(infos[0].bit_depth)
        self.sample_rates = [int(si.sample_rate) for si in infos]
        self.compressed_bytes = sum(len(b) for b in bare)
        stated = [int(si.interchannel_samples) for si in infos]
        # the context decodes the largest block any file states; a larger one than the decoder takes
        # would only show as BAD_FRAME at crop time
        most = flacgpu.decoder_max_block(self.bits)
        for i, si in enumerate(infos):
            if int(si.max_block_size) > most:
                raise ValueError(f"FlacBank: file {i} states blocks of {int(si.max_block_size)} samples, the decoder takes "
                                 f"at most {most} at {self.bits} bits")

        # ---- everything below needs the device
        import numpy as np
        import torch

        self.device = torch.device("cuda", device)
        block = max([int(si.max_block_size) for si in infos] + [16])
        self._dec = flacgpu.Decoder(self.channels, self.bits, self.sample_rates[0], device=device, max_frames=max_frames,
                                    block_size=block)
        n = len(files)
        offs, at = [], 0
        for b in bare:  # stream offsets need no alignment
            offs.append(at)
            at += len(b)
        blob = np.frombuffer(b"".join(bare) + bytes(16), dtype=np.uint8)
        self._caps = [len(b) // 8 + 1 for b in bare]  # a frame is at least 9 bytes
        self._first, entries = [], 0
        for c in self._caps:
            self._first.append(entries)
            entries += c
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            self._data = torch.from_numpy(blob.copy()).to(self.device)
            self._off = torch.zeros(entries, dtype=torch.int64, device=self.device)
            self._fbytes = torch.zeros(entries, dtype=torch.int32, device=self.device)
            self._ires = torch.zeros(16 * n, dtype=torch.uint8, device=self.device)
            self._pos = torch.zeros(entries, dtype=torch.int64, device=self.device)
            self._totals = torch.zeros(n, dtype=torch.int64, device=self.device)
            bits = [self.bits] * n
            self._dec.flac_index_streams_device(self._data.data_ptr(), offs, [len(b) for b in bare], self._first, self._caps,
                                                self._off.data_ptr(), self._fbytes.data_ptr(), self._ires.data_ptr(),
                                                stream_bits=bits, stream_rates=self.sample_rates, stream=st)
            self._dec.flac_positions_streams_device(self._data.data_ptr(), self._first, self._caps, self._off.data_ptr(),
                                                    self._fbytes.data_ptr(), self._ires.data_ptr(), self._pos.data_ptr(),
                                                    self._totals.data_ptr(), stream_bits=bits,
                                                    stream_rates=self.sample_rates, stream=st)
            self._dec.sync_check(st)  # the one wait
            ires = (flacgpu.IndexResult * n).from_buffer_copy(self._ires.cpu().numpy().tobytes())
            self.samples = [int(v) for v in self._totals.cpu().tolist()]
        for i in range(n):
            if ires[i].status != flacgpu.INDEX_OK:
                self.close()
                raise flacgpu.FlacGpuError(-2, f"FlacBank: the device index refuses file {i} (status {ires[i].status})")
            if stated[i] and self.samples[i] != stated[i]:
                self.close()
                raise ValueError(f"FlacBank: file {i} holds {self.samples[i]} samples, its STREAMINFO states {stated[i]}")

    def close(self) -> None:
        if getattr(self, "_dec", None) is not None:
            self._dec.close()
            self._dec = None
        self._data = self._off = self._fbytes = self._ires = self._pos = self._totals = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return len(self.sample_rates)

    def crops(self, file: Sequence[int], start: Sequence[int], length: int, dtype=None, planar: bool = True,
              pad: bool = True, out=None, strict: bool = True):
        """Samples [start[w], start[w] + length) of file[w] for every w -> (x, n): x of shape
        [W, channels, length] (planar) or [W, length, channels] in dtype (torch.float32 -- the
        default --, float16, bfloat16: sample * 2^-(bits-1); int32: the sample), n[w] the samples
        crop w really holds (fewer where it runs into the end of its file; the rest of x is zero,
        written by the kernel with pad=True, by a memset before it with pad=False).  The work is
        queued on torch.cuda.current_stream(device); the call waits for it.  strict: raise
        FlacGpuError for the first crop whose status is not OK; strict=False returns
        (x, n, statuses) instead.  out: a contiguous tensor of x's shape, dtype and device to fill."""
        import torch

        if self._dec is None:
            raise ValueError("FlacBank: closed")
        dtype = torch.float32 if dtype is None else dtype
        fmt = _formats().get(dtype)
        if fmt is None:
            raise ValueError(f"FlacBank: dtype {dtype} is none of float32, float16, bfloat16, int32")
        W, C, length = len(file), self.channels, int(length)
        if len(start) != W:
            raise ValueError("FlacBank: file and start differ in length")
        if length < 0 or any(not 0 <= int(f) < len(self) for f in file) or any(int(s) < 0 for s in start):
            raise ValueError("FlacBank: a file index, a start or the length is out of range")
        shape = (W, C, length) if planar else (W, length, C)
        with torch.cuda.device(self.device):
            if out is not None:
                if (tuple(out.shape) != shape or out.dtype != dtype or out.device != self.device or not out.is_contiguous()):
                    raise ValueError(f"FlacBank: out must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
                x = out
                if not pad:
                    x.zero_()
            else:
                x = torch.empty(shape, dtype=dtype, device=self.device) if pad else torch.zeros(shape, dtype=dtype,
                                                                                                 device=self.device)
            flags = (flacgpu.DELIVER_PLANAR if planar else 0) | (flacgpu.DELIVER_PAD if pad else 0)
            st = torch.cuda.current_stream(self.device).cuda_stream
            d_res = torch.empty(32 * max(W, 1), dtype=torch.uint8, device=self.device)
            per_crop = C * length
            for w0 in range(0, W, MAX_WINDOWS):
                w1 = min(W, w0 + MAX_WINDOWS)
                windows = [(int(file[w]), int(start[w]), length) for w in range(w0, w1)]
                self._dec.decode_windows_device_as(
                    self._data.data_ptr(), self._first, self._off.data_ptr(), self._fbytes.data_ptr(), self._ires.data_ptr(),
                    self._pos.data_ptr(), self._totals.data_ptr(), windows, fmt, flags, x.data_ptr(),
                    [w * per_crop for w in range(w0, w1)], [per_crop] * (w1 - w0), d_res.data_ptr() + 32 * w0, stream=st)
            res = (flacgpu.WindowResult * max(W, 1)).from_buffer_copy(d_res.cpu().numpy().tobytes())  # waits for st
        n = [int(res[w].n_samples) for w in range(W)]
        statuses = [int(res[w].status) for w in range(W)]
        if strict:
            for w, s in enumerate(statuses):
                if s != flacgpu.WINDOW_OK:
                    bad = f", frame {res[w].first_bad_frame}" if s == flacgpu.WINDOW_BAD_FRAME else ""
                    raise flacgpu.FlacGpuError(-2, f"FlacBank.crops: crop {w} (file {int(file[w])}, start {int(start[w])}) is "
                                                   f"{WINDOW_STATUS.get(s, s)}{bad}")
            return x, n
        return x, n, statuses
