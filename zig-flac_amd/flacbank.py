"""FlacBank: FLAC files kept compressed in device memory, random crops of them as torch tensors.

The files' frames are uploaded once into one uint8 tensor, indexed and their sample positions
scanned once (flacgpu_flac_index_streams_device, flacgpu_flac_positions_streams_device); every
`crops` call then decodes only the frames that hold the requested samples and delivers them as
[crop, channel, time] (or [crop, time, channel]) elements in one pass
(flacgpu_decode_windows_device_as), on the caller's current torch stream.  Plumbing over the C ABI:
there is no CPU path.  A bank takes no locks: one bank per thread, like a context.  With a `rate`
the crops are stated and delivered at that sample rate: those of files at another rate go through
flacgpu_decode_windows_device_resample, one call per source rate.  FlacBank.from_tensors builds the
same bank from tensors on the device (flacgpu_pcm_from_elements_device, flacgpu_encode_plan_device);
file_bytes writes a bank's file back out as a .flac.  FlacBank.levels and crop_levels measure instead
of delivering: peak, sum and energy of every block of a hop (flacgpu_levels_windows_device).

FlacBank holds files of one channel count and depth.  FlacMixBank holds any, as one FlacBank per
(channels, bits), and delivers every crop with the bank's one channel count through
flacgpu_decode_windows_device_mix (channel masks) or, where a group's mix is a weight matrix
(a surround downmix, mid/side, a mean of three), flacgpu_decode_windows_device_to.  With a FirBank
(`crops(fir=, fir_index=)`) every crop is delivered convolved with the filter of its choice, over the
file's own samples around it, through flacgpu_decode_windows_device_fir."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import flacgpu

MAX_WINDOWS = 65535  # of one flacgpu_decode_windows_device_as call
WINDOW_STATUS = {flacgpu.WINDOW_BAD_INDEX: "BAD_INDEX", flacgpu.WINDOW_BAD_FRAME: "BAD_FRAME",
                 flacgpu.WINDOW_TOO_SMALL: "TOO_SMALL"}


def _formats():
    import torch

    return {torch.int32: flacgpu.SAMPLE_I32, torch.float32: flacgpu.SAMPLE_F32, torch.float16: flacgpu.SAMPLE_F16,
            torch.bfloat16: flacgpu.SAMPLE_BF16}


def _parse(who: str, i: int, f: bytes):
    """File i's STREAMINFO and its bare frames, parsed on the host."""
    try:
        si, first, _ = flacgpu.flac_index(f)
    except flacgpu.FlacGpuError as e:
        raise ValueError(f"{who}: file {i} is not a FLAC file this library indexes ({e})") from None
    return si, bytes(f[first:])


def _check_blocks(who: str, i: int, si) -> None:
    """The block-size rule: a larger block than the decoder takes would only show as BAD_FRAME at crop time."""
    most = flacgpu.decoder_max_block(int(si.bit_depth))
    if int(si.max_block_size) > most:
        raise ValueError(f"{who}: file {i} states blocks of {int(si.max_block_size)} samples, the decoder takes "
                         f"at most {most} at {int(si.bit_depth)} bits")


def _rate_error(who: str, i: int, src: int, rate: int) -> Optional[str]:
    """Why file i of rate src cannot be delivered at `rate`, or None (equal rates need no filter)."""
    if src == rate or flacgpu.resample_ratio(src, rate) is not None:
        return None
    return (f"{who}: file {i} is at {src} Hz, and {src} -> {rate} is not a ratio the resampler serves "
            f"(up and down factors of at most 1024, at most 12 to 1 down)")


def _out_samples(samples: int, src: int, rate: int) -> int:
    if src == rate:
        return samples
    L, M, _ = flacgpu.resample_ratio(src, rate)
    return (samples * L + M - 1) // M


def _crops(who, device, n_files, K, groups, where, check, file, start, length, dtype, planar, pad, out, strict,
           rate=None, rate_of=None, feat=None, fir=None, fir_index=None):
    """The one body of FlacBank.crops and FlacMixBank.crops: crops of K channels from `groups` =
    [(FlacBank, its channel masks, its [K, C] float32 weight matrix or None)], file f being file where(f)[1] of group where(f)[0];
    check(fmt): the caller's own refusals of a format, raised between the dtype's and the crops'.
    rate: start and length are in samples at that rate, rate_of(f) being file f's own: the crops of
    files at another rate are resampled, one call per group and source rate.
    feat: the body of the two `features` as well -- (n_fft, hop, filters or None, rows) after
    flacgpu.features_params: `length` is then the frame count, a crop is [K, rows, length] and its
    calls are flacgpu_decode_windows_device_features, routed as the crops' are.
    fir: a FirBank, fir_index[w] the filter crop w goes through: the calls are
    flacgpu_decode_windows_device_fir, routed as the crops' are; without it nothing here changes."""
    import torch

    dtype = torch.float32 if dtype is None else dtype
    fmt = _formats().get(dtype)
    if fmt is None:
        raise ValueError(f"{who}: dtype {dtype} is none of float32, float16, bfloat16, int32")
    check(fmt)
    if rate is not None and fmt == flacgpu.SAMPLE_I32:
        raise ValueError(f"{who}: int32 crops at a sample rate: a resampled sample has no integer value to deliver")
    W, length = len(file), int(length)
    if len(start) != W:
        raise ValueError(f"{who}: file and start differ in length")
    if length < 0 or any(not 0 <= int(f) < n_files for f in file) or any(int(s) < 0 for s in start):
        raise ValueError(f"{who}: a file index, a start or the length is out of range")
    if fir is not None:
        fir._check_crops(who, device, K, fmt, W, fir_index, length)
    elif fir_index is not None:
        raise ValueError(f"{who}: fir_index without fir")
    shape = (W, K, length) if planar else (W, length, K)
    if feat is not None:
        shape = (W, K, feat[3], length)
    routed = [[] for _ in groups]  # group -> its crops, in the caller's order
    for w in range(W):
        routed[where(int(file[w]))[0]].append(w)
    calls = []  # (bank, masks, the source rate to resample from or None, its crops): one library call per 65535
    for (bank, masks), ws in zip(groups, routed):
        if rate is None:
            calls.append((bank, masks, None, ws))
            continue
        by_rate: dict = {}
        for w in ws:
            by_rate.setdefault(rate_of(int(file[w])), []).append(w)
        for src, part in by_rate.items():
            why = _rate_error(who, int(file[part[0]]), src, rate)
            if why:
                raise ValueError(why)
            calls.append((bank, masks, None if src == rate else src, part))
    order = [w for c in calls for w in c[3]]  # row r of d_res is crop order[r]
    with torch.cuda.device(device):
        if out is not None:
            if (tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous()):
                raise ValueError(f"{who}: out must be a contiguous {dtype} tensor of shape {shape} on {device}")
            x = out
            if not pad:
                x.zero_()
        else:
            x = torch.empty(shape, dtype=dtype, device=device) if pad else torch.zeros(shape, dtype=dtype, device=device)
        flags = (flacgpu.DELIVER_PLANAR if planar else 0) | (flacgpu.DELIVER_PAD if pad else 0)
        st = torch.cuda.current_stream(device).cuda_stream
        d_res = torch.empty(32 * max(W, 1), dtype=torch.uint8, device=device)
        per_crop, row = K * length * (feat[3] if feat is not None else 1), 0
        for bank, masks, src, ws in calls:
            for w0 in range(0, len(ws), MAX_WINDOWS):
                part = ws[w0:w0 + MAX_WINDOWS]
                windows = [(where(int(file[w]))[1], int(start[w]), length) for w in part]
                tables = (bank._data.data_ptr(), bank._first, bank._off.data_ptr(), bank._fbytes.data_ptr(),
                          bank._ires.data_ptr(), bank._pos.data_ptr(), bank._totals.data_ptr(), windows, fmt, flags)
                to = (x.data_ptr(), [w * per_crop for w in part], [per_crop] * len(part), d_res.data_ptr() + 32 * row)
                if fir is not None:
                    weighted = _is_weights(masks)
                    bank._dec.decode_windows_device_fir(*tables, fir.taps.data_ptr(), fir.taps.numel(), fir.table,
                                                        [int(fir_index[w]) for w in part], *to,
                                                        channel_masks=None if weighted else masks,
                                                        channel_weights=masks if weighted else None, src_rate=src or 0,
                                                        dst_rate=rate if src else 0, stream=st)
                elif _is_weights(masks):
                    bank._dec.decode_windows_device_to(*tables[:8], fmt, 0 if feat is not None else flags, *to,
                                                       channel_weights=masks, src_rate=src or 0, dst_rate=rate if src else 0,
                                                       n_fft=feat[0] if feat is not None else None,
                                                       hop=feat[1] if feat is not None else None,
                                                       filters=feat[2] if feat is not None else None, stream=st)
                elif feat is not None:
                    bank._dec.decode_windows_device_features(*tables[:-1], masks, src or 0, rate if src else 0, *feat[:3], *to,
                                                             stream=st)
                elif src is not None:
                    bank._dec.decode_windows_device_resample(*tables, masks, src, rate, *to, stream=st)
                elif masks is None:
                    bank._dec.decode_windows_device_as(*tables, *to, stream=st)
                else:
                    bank._dec.decode_windows_device_mix(*tables, masks, *to, stream=st)
                row += len(part)
        rows = (flacgpu.WindowResult * max(W, 1)).from_buffer_copy(d_res.cpu().numpy().tobytes())  # waits for st
    res = [None] * W
    for r, w in enumerate(order):
        res[w] = rows[r]
    n = [int(res[w].n_samples) for w in range(W)]
    statuses = [int(res[w].status) for w in range(W)]
    if strict:
        for w, s in enumerate(statuses):
            if s != flacgpu.WINDOW_OK:
                bad = f", frame {res[w].first_bad_frame}" if s == flacgpu.WINDOW_BAD_FRAME else ""
                raise flacgpu.FlacGpuError(-2, f"{who}.{'features' if feat is not None else 'crops'}: crop {w} (file {int(file[w])}, start {int(start[w])}) is "
                                               f"{WINDOW_STATUS.get(s, s)}{bad}")
        return x, n
    return x, n, statuses


def _features(who, device, n_files, K, groups, where, file, start, frames, n_fft, hop, filters, log, floor, dtype, out, strict,
              rate, rate_of):
    """FlacBank.features and FlacMixBank.features over _crops: the checks, and the logarithm, which
    is torch's over the kernel's float32 (it is not part of the library's rule)."""
    import torch

    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"{who}.features: dtype {dtype} is none of float32, float16, bfloat16")
    if log not in (None, "ln", "log10"):
        raise ValueError(f"{who}.features: log is None, 'ln' or 'log10', not {log!r}")
    ft, f, rows = flacgpu.features_params(n_fft, hop, filters)
    frames = int(frames)
    if frames and (frames - 1) * ft.hop + ft.n_fft >= flacgpu.FEATURES_MAX_SPAN:
        raise ValueError(f"{who}.features: {frames} frames span 2^31 samples or more")
    feat = (ft.n_fft, ft.hop, f, rows)
    if log is None:
        return _crops(who, device, n_files, K, groups, where, lambda fmt: None, file, start, frames, dtype, True, False, out,
                      strict, rate=rate, rate_of=rate_of, feat=feat)
    shape = (len(file), K, rows, max(frames, 0))
    if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous {dtype} tensor of shape {shape} on {device}")
    res = _crops(who, device, n_files, K, groups, where, lambda fmt: None, file, start, frames, torch.float32, True, False,
                 out if dtype == torch.float32 else None, strict, rate=rate, rate_of=rate_of, feat=feat)
    x = res[0].clamp_min_(float(floor))
    x = torch.log_(x) if log == "ln" else torch.log10_(x)
    if out is not None and out is not x:
        out.copy_(x)
        x = out
    elif dtype != torch.float32:
        x = x.to(dtype)
    return (x,) + tuple(res[1:])


def _hz_to_mel(f, scale: str):
    import numpy as np

    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0), lin)


def _mel_to_hz(m, scale: str):
    import numpy as np

    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filters(sample_rate: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None,
                scale: str = "slaney", norm: Optional[str] = "slaney"):
    """A mel filter bank for `features`: float32 numpy [n_mels, n_fft // 2 + 1], computed in float64.

    The mel scale: scale="htk": mel(f) = 2595 * log10(1 + f / 700).  scale="slaney": mel(f) =
    3 f / 200 below 1000 Hz, and 15 + 27 * ln(f / 1000) / ln(6.4) from 1000 Hz on (linear, then
    logarithmic with 27 steps to the factor 6.4).  With m_0 < m_1 < ... < m_{n_mels + 1} equally
    spaced from mel(fmin) to mel(fmax) (fmax None: sample_rate / 2) and f_i = hz(m_i), bin b sits at
    g_b = b * sample_rate / n_fft and row r is the triangle
        F[r][b] = max(0, min((g_b - f_r) / (f_{r+1} - f_r), (f_{r+2} - g_b) / (f_{r+2} - f_{r+1}))),
    which peaks at the centre f_{r+1}.  norm="slaney" multiplies row r by 2 / (f_{r+2} - f_r), so that
    every triangle has area 1 over frequency in Hz; norm=None leaves the peaks at 1."""
    import numpy as np

    sample_rate, n_fft, n_mels = int(sample_rate), int(n_fft), int(n_mels)
    fmax = sample_rate / 2.0 if fmax is None else float(fmax)
    if scale not in ("slaney", "htk") or norm not in ("slaney", None):
        raise ValueError("mel_filters: scale is 'slaney' or 'htk', norm 'slaney' or None")
    if sample_rate <= 0 or not (16 <= n_fft <= 2048 and n_fft % 2 == 0) or not 1 <= n_mels <= 256:
        raise ValueError("mel_filters: sample_rate > 0, n_fft even in 16..2048, n_mels in 1..256")
    if not 0.0 <= float(fmin) < fmax <= sample_rate / 2.0:
        raise ValueError("mel_filters: 0 <= fmin < fmax <= sample_rate / 2")
    edges = _mel_to_hz(np.linspace(_hz_to_mel(float(fmin), scale), _hz_to_mel(fmax, scale), n_mels + 2), scale)
    g = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / n_fft)
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    F = np.maximum(0.0, np.minimum((g[None, :] - lo) / (mid - lo), (hi - g[None, :]) / (hi - mid)))
    if norm == "slaney":
        F *= 2.0 / (hi - lo)
    return np.ascontiguousarray(F, dtype=np.float32)


def fir_windowed_sinc(sample_rate: int, f_lo: float, f_hi: Optional[float], taps: int):
    """(h, delay): a Kaiser-windowed (beta 9, as the resampler's) band-pass of `taps` taps that passes
    f_lo .. f_hi Hz at sample_rate, as a float32 numpy array, and its delay (taps - 1) // 2, which
    re-centres it.  f_lo = 0 gives a low-pass; f_hi = None a high-pass from f_lo (odd `taps` only: an
    even-length symmetric filter has a zero at half the rate).  Computed in numpy float64 -- the ideal
    response 2 f2 sinc(2 f2 m) - 2 f1 sinc(2 f1 m), m = n - (taps - 1) / 2, f in cycles a sample, times
    np.kaiser(taps, 9) -- and rounded once."""
    import numpy as np

    sample_rate, taps = int(sample_rate), int(taps)
    if sample_rate < 1 or not 1 <= taps <= flacgpu.FIR_MAX_TAPS:
        raise ValueError(f"fir_windowed_sinc: a sample rate of at least 1 and 1 to {flacgpu.FIR_MAX_TAPS} taps")
    nyq = sample_rate / 2.0
    if f_hi is None and taps % 2 == 0:
        raise ValueError("fir_windowed_sinc: a high-pass (f_hi=None) needs an odd number of taps")
    hi = nyq if f_hi is None else float(f_hi)
    lo = float(f_lo)
    if not (0.0 <= lo < hi <= nyq) or (f_hi is None and lo == 0.0):
        raise ValueError(f"fir_windowed_sinc: 0 <= f_lo < f_hi <= {nyq} Hz (f_hi=None: f_lo > 0)")
    m = np.arange(taps, dtype=np.float64) - (taps - 1) / 2.0
    f1, f2 = lo / sample_rate, hi / sample_rate
    ideal = 2.0 * f2 * np.sinc(2.0 * f2 * m) - 2.0 * f1 * np.sinc(2.0 * f1 * m)
    return (ideal * np.kaiser(taps, 9.0)).astype(np.float32), (taps - 1) // 2


class FirBank:
    """FIR filters for `crops(fir=, fir_index=)`, packed once into one float32 tensor on the device.

    filters: a sequence of [T] or [K, T] arrays or tensors, 1 <= T <= 4096 finite taps at the
    delivered rate: one row serves every output channel, K rows one each (K the channels of the
    crops: binaural or array responses; a bank serves crops of K channels only where every filter has
    1 or K rows).  delays: one per filter, 0 .. T - 1 (default 0): element t of
    a crop is the sum over k of h[k] x[start + t + delay - k], so delay = (T - 1) // 2 re-centres a
    linear-phase filter and a response's direct-path index keeps labels aligned.  `table` is the host
    side of flacgpu_decode_windows_device_fir: [(offset, taps, delay, rows)]."""

    def __init__(self, filters: Sequence, delays: Optional[Sequence[int]] = None, device=0):
        import numpy as np
        import torch

        who = "FirBank"
        if len(filters) == 0:
            raise ValueError(f"{who}: no filters")
        if delays is not None and len(delays) != len(filters):
            raise ValueError(f"{who}: {len(delays)} delays for {len(filters)} filters")
        rows_of, self.table, offset = [], [], 0
        for i, f in enumerate(filters):
            if isinstance(f, torch.Tensor):
                f = f.detach().cpu().numpy()
            h = np.ascontiguousarray(f, dtype=np.float32)
            if h.ndim == 1:
                h = h[None, :]
            if h.ndim != 2 or not 1 <= h.shape[0] <= 8:
                raise ValueError(f"{who}: filter {i} is not [T] or [K, T] with 1 to 8 rows")
            T = h.shape[1]
            if not 1 <= T <= flacgpu.FIR_MAX_TAPS:
                raise ValueError(f"{who}: filter {i} has {T} taps, not 1 to {flacgpu.FIR_MAX_TAPS}")
            if not np.isfinite(h).all():
                raise ValueError(f"{who}: filter {i} has a tap that is not finite")
            d = 0 if delays is None else int(delays[i])
            if not 0 <= d < T:
                raise ValueError(f"{who}: filter {i} has delay {d}, not 0 to {T - 1}")
            rows_of.append(h)
            self.table.append((offset, T, d, h.shape[0]))
            offset += h.size
        # ---- everything below needs the device
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.taps = torch.from_numpy(np.concatenate([h.reshape(-1) for h in rows_of])).to(self.device)

    def __len__(self) -> int:
        return len(self.table)

    def _check_crops(self, who, device, K, fmt, W, fir_index, length) -> None:
        if fmt == flacgpu.SAMPLE_I32:
            raise ValueError(f"{who}: int32 crops through a filter: a filtered sample has no integer value to deliver")
        if self.device != device:
            raise ValueError(f"{who}: the FirBank is on {self.device}, the bank on {device}")
        if fir_index is None or len(fir_index) != W:
            raise ValueError(f"{who}: fir needs fir_index, one filter index a crop")
        for i, (_, _, _, rows) in enumerate(self.table):  # the call refuses a table with such a filter, used or not
            if rows not in (1, K):
                raise ValueError(f"{who}: filter {i} has {rows} rows, the crops {K} channels")
        for i in set(int(i) for i in fir_index):
            if not 0 <= i < len(self.table):
                raise ValueError(f"{who}: filter index {i} is not in 0..{len(self.table) - 1}")
            T = self.table[i][1]
            if length + T - 1 >= flacgpu.FIR_MAX_SPAN:
                raise ValueError(f"{who}: {length} samples through {T} taps span 2^31 samples or more")


class FlacBank:
    def __init__(self, files: Sequence[bytes], device: int = 0, max_frames: int = 4096, _group=None):
        # _group: (who, [the caller's file index], [(STREAMINFO, bare frames)]) from FlacMixBank, whose
        # files are parsed and checked already and whose messages name its caller's indices
        who, names, parsed = _group if _group else ("FlacBank", range(len(files)), None)
        if len(files) == 0:
            raise ValueError("FlacBank: no files")
        if len(files) > 65535:
            raise ValueError("FlacBank: more than 65535 files")
        infos, bare = [], []
        for i, f in enumerate(files):
            si, frames = parsed[i] if parsed else _parse(who, i, f)
            if infos and (si.channels, si.bit_depth) != (infos[0].channels, infos[0].bit_depth):
                raise ValueError(f"FlacBank: file {i} has {si.channels} channels of {si.bit_depth} bits, file 0 has "
                                 f"{infos[0].channels} of {infos[0].bit_depth}: one bank holds one channel count and depth")
            infos.append(si)
            bare.append(frames)
        self._dec = None
        # the context decodes the largest block any file states
        for i, si in enumerate(infos):
            _check_blocks(who, names[i], si)

        # ---- everything below needs the device
        import numpy as np
        import torch

        offs, at = [], 0
        for b in bare:  # stream offsets need no alignment
            offs.append(at)
            at += len(b)
        blob = np.frombuffer(b"".join(bare) + bytes(16), dtype=np.uint8)
        self.clipped = None  # elements clipped per file: of a bank built from tensors only
        self._heads = [bytes(f[:len(f) - len(b)]) for f, b in zip(files, bare)]  # the metadata, as given
        self._index(who, names, torch.from_numpy(blob.copy()), offs, [len(b) for b in bare], infos, device, max_frames)

    def _index(self, who, names, data, offs, lens, infos, device, max_frames) -> None:
        """What a bank is once its frames are in HBM, however they got there: data, a uint8 tensor
        that holds stream i's bare frames at [offs[i], offs[i] + lens[i]) and 16 zero bytes after the
        last -- on the device, or on the host and uploaded here once the context is open; infos, their
        STREAMINFOs.  Opens the decode context, indexes the streams on the device (every frame's CRCs
        are checked there), scans their sample positions and checks the totals against what the
        STREAMINFOs state."""
        import torch

        self._dec = None
        self.channels, self.bits = int(infos[0].channels), int(infos[0].bit_depth)
        self.sample_rates = [int(si.sample_rate) for si in infos]
        self.compressed_bytes = sum(lens)
        stated = [int(si.interchannel_samples) for si in infos]
        self._infos, self._offs, self._lens = list(infos), list(offs), list(lens)
        self.device = torch.device("cuda", device)
        block = max([int(si.max_block_size) for si in infos] + [16])
        self._dec = flacgpu.Decoder(self.channels, self.bits, self.sample_rates[0], device=device, max_frames=max_frames,
                                    block_size=block)
        n = len(infos)
        self._caps = [b // 8 + 1 for b in lens]  # a frame is at least 9 bytes
        self._first, entries = [], 0
        for c in self._caps:
            self._first.append(entries)
            entries += c
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            self._data = data.to(self.device)
            self._off = torch.zeros(entries, dtype=torch.int64, device=self.device)
            self._fbytes = torch.zeros(entries, dtype=torch.int32, device=self.device)
            self._ires = torch.zeros(16 * n, dtype=torch.uint8, device=self.device)
            self._pos = torch.zeros(entries, dtype=torch.int64, device=self.device)
            self._totals = torch.zeros(n, dtype=torch.int64, device=self.device)
            bits = [self.bits] * n
            self._dec.flac_index_streams_device(self._data.data_ptr(), offs, lens, self._first, self._caps,
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
                raise flacgpu.FlacGpuError(-2, f"{who}: the device index refuses file {names[i]} (status {ires[i].status})")
            if stated[i] and self.samples[i] != stated[i]:
                self.close()
                raise ValueError(f"{who}: file {names[i]} holds {self.samples[i]} samples, its STREAMINFO states {stated[i]}")

    @classmethod
    def from_tensors(cls, tensors, sample_rate, bits: int = 16, device: int = 0, block_size: int = 4096,
                     prediction: int = 0, planar: bool = True, max_frames: int = 4096, scratch_bytes: int = 1 << 30):
        """A bank of the audio in `tensors`, compressed on the device: a sequence of [C, T_i] tensors
        ([T_i, C] with planar=False) or one [N, C, T] ([N, T, C]) tensor, of one channel count (1..8)
        and one dtype out of float32, float16, bfloat16 (a sample is the element times 2^(bits-1),
        rounded to nearest-even and clamped: the inverse of `crops`) and int32 (the sample itself,
        clamped); tensors on the CPU are moved to the device.  sample_rate: an int, or one per tensor.
        bits (8, 16, 24, 32), block_size (16..4096) and prediction (0: fixed predictors, 1..12: LPC up
        to that order) are the encoder's.  The tensors are taken in groups whose PCM and frame bound
        fit scratch_bytes (a larger tensor is a group alone): each group is quantised
        (flacgpu_pcm_from_elements_device) and encoded with its MD5 (flacgpu_encode_plan_device) on
        torch.cuda.current_stream(device), the call waits once per group, and only the group's frames
        are kept.  The result is an ordinary FlacBank, indexed on the device as one built from files
        is; `clipped` holds the elements per tensor that the clamp changed or that were NaN.  What
        is wrong with the arguments raises ValueError before any device use."""
        import torch

        who = "FlacBank.from_tensors"
        if isinstance(tensors, torch.Tensor):
            if tensors.dim() != 3:
                raise ValueError(f"{who}: one tensor holds [N, C, T] (or [N, T, C]), not {tensors.dim()} dimensions")
            tensors = tensors.unbind(0)
        tensors = list(tensors)
        n = len(tensors)
        if n == 0:
            raise ValueError(f"{who}: no tensors")
        if n > 65535:
            raise ValueError(f"{who}: more than 65535 tensors")
        bits, block_size, prediction, scratch_bytes = int(bits), int(block_size), int(prediction), int(scratch_bytes)
        if bits not in (8, 16, 24, 32):
            raise ValueError(f"{who}: bits is {bits}, not 8, 16, 24 or 32")
        if not 16 <= block_size <= 4096:
            raise ValueError(f"{who}: block_size is {block_size}, not in 16..4096")
        if not 0 <= prediction <= 12:
            raise ValueError(f"{who}: prediction is {prediction}, not in 0..12")
        rates = [int(r) for r in sample_rate] if isinstance(sample_rate, (list, tuple)) else [int(sample_rate)] * n
        if len(rates) != n or any(not 0 < r < (1 << 20) for r in rates):
            raise ValueError(f"{who}: sample_rate is one rate in 1..2^20-1, or one for each of the {n} tensors")
        fmt, C, Ts = None, None, []
        for i, x in enumerate(tensors):
            if not isinstance(x, torch.Tensor) or x.dim() != 2:
                raise ValueError(f"{who}: tensor {i} is not a tensor of two dimensions")
            c, t = (x.shape[0], x.shape[1]) if planar else (x.shape[1], x.shape[0])
            f = _formats().get(x.dtype)
            if f is None:
                raise ValueError(f"{who}: tensor {i} has dtype {x.dtype}, none of float32, float16, bfloat16, int32")
            if i == 0:
                fmt, C = f, int(c)
                if not 1 <= C <= 8:
                    raise ValueError(f"{who}: tensor 0 has {C} channels, not 1 to 8")
            elif int(c) != C or f != fmt:
                raise ValueError(f"{who}: tensor {i} has {int(c)} channels of {x.dtype}, tensor 0 has {C} of "
                                 f"{tensors[0].dtype}: one bank holds one channel count and one dtype")
            if int(t) == 0:
                raise ValueError(f"{who}: tensor {i} holds no samples")
            Ts.append(int(t))
        B = bits // 8
        # the bytes a tensor needs in a group: its PCM and its frames' share of the plan's output bound
        cfg = flacgpu.Config(rates[0], block_size, C, bits, 1, 8, 30, prediction)
        image = (flacgpu.load_library().flacgpu_frame_bound_bytes(ctypes.byref(cfg)) + 16 + 15) // 16 * 16
        pcm_len = [(T * C * B + 3) // 4 * 4 for T in Ts]
        need = [p + (T + block_size - 1) // block_size * image for p, T in zip(pcm_len, Ts)]
        groups, used = [[]], 0
        for i in range(n):
            if groups[-1] and used + need[i] > scratch_bytes:
                groups.append([])
                used = 0
            groups[-1].append(i)
            used += need[i]

        # ---- everything below needs the device
        dev = torch.device("cuda", device)
        encoders: dict = {}  # rate -> Encoder: the rate is in every frame header
        kept, offs, lens, infos, clipped = [], [0] * n, [0] * n, [None] * n, [0] * n
        at = 0
        try:
            for rate in dict.fromkeys(rates):
                encoders[rate] = flacgpu.Encoder(C, bits, rate, device=device, max_frames=max_frames, block_size=block_size,
                                                 lpc_order=prediction)
            with torch.cuda.device(dev):
                st = torch.cuda.current_stream(dev).cuda_stream
                for group in groups:
                    by_rate: dict = {}
                    for i in group:
                        by_rate.setdefault(rates[i], []).append(i)
                    for rate, idx in by_rate.items():  # one quantise and one encode per rate of the group
                        enc = encoders[rate]
                        src = []
                        for i in idx:
                            x = tensors[i].to(dev)
                            ok = x.is_contiguous() or (planar and x.stride(1) == 1 and (C == 1 or x.stride(0) >= Ts[i]))
                            src.append(x if ok else x.contiguous())
                        strides = [x.stride(0) if planar and C > 1 else Ts[i] for x, i in zip(src, idx)]
                        p_off, total_pcm = [], 0
                        for i in idx:
                            p_off.append(total_pcm)
                            total_pcm += pcm_len[i]
                        d_pcm = torch.empty(total_pcm, dtype=torch.uint8, device=dev)
                        d_clip = torch.empty(len(idx), dtype=torch.int64, device=dev)
                        enc.pcm_from_elements_device([x.data_ptr() for x in src], [Ts[i] for i in idx], strides, fmt,
                                                     flacgpu.DELIVER_PLANAR if planar else 0, d_pcm.data_ptr(), p_off,
                                                     total_pcm, d_clip.data_ptr(), stream=st)
                        plan = enc.plan(p_off, [Ts[i] for i in idx])
                        try:
                            nf, bound = int(plan.n_frames), int(plan.out_bound)
                            d_out = torch.empty(bound, dtype=torch.uint8, device=dev)
                            d_fb = torch.empty(nf, dtype=torch.int32, device=dev)
                            d_fo = torch.empty(nf + 1, dtype=torch.int64, device=dev)  # the last entry: the total
                            d_md5 = torch.empty(16 * len(idx), dtype=torch.uint8, device=dev)
                            enc.encode_plan_device(plan, d_pcm.data_ptr(), d_out.data_ptr(), bound, d_fb.data_ptr(),
                                                   d_fo.data_ptr(), d_fo.data_ptr() + 8 * nf, d_md5=d_md5.data_ptr(), stream=st)
                            firsts = [int(f) for f in plan.first_frame] + [nf]
                            d_cut = d_fo[torch.tensor(firsts, dtype=torch.int64).to(dev, non_blocking=True)]
                            enc.sync_check(st)  # the one wait of the group (one per rate in it)
                            cut = [int(v) for v in d_cut.cpu().tolist()]  # where every stream's bytes begin, and the total
                        finally:
                            plan.close()
                        md5 = d_md5.cpu().numpy().tobytes()
                        clip = d_clip.cpu().tolist()
                        kept.append(d_out[:cut[-1]].clone())  # the compact frames: the bound's slack goes with d_out
                        for j, i in enumerate(idx):
                            offs[i], lens[i], clipped[i] = at + cut[j], cut[j + 1] - cut[j], int(clip[j])
                            si = flacgpu.StreamInfo.new(rate, C, bits, Ts[i], block_size)
                            ctypes.memmove(si.md5, md5[16 * j:16 * j + 16], 16)
                            infos[i] = si
                        at += cut[-1]
                        del d_pcm, d_out, d_fb, d_fo, d_md5, d_clip, src
                data = torch.cat(kept + [torch.zeros(16, dtype=torch.uint8, device=dev)])
        finally:
            for enc in encoders.values():
                enc.close()
        del kept
        bank = cls.__new__(cls)
        bank.clipped, bank._heads = clipped, None
        bank._index("FlacBank.from_tensors", range(n), data, offs, lens, infos, device, max_frames)
        return bank

    def file_bytes(self, i: int) -> bytes:
        """File i as a valid .flac: of a bank built from files the metadata it was given, up to the
        first frame, then the frames as the bank holds them; of one built from tensors the 73-byte
        header flacgpu_encode_file writes (STREAMINFO with the block size, the samples, the MD5 of
        the PCM and the frame sizes replayed through flacgpu_streaminfo_update_frame_size; the vendor
        comment), then the frames.  Copies the file's frames to the host: not a hot path."""
        if self._dec is None:
            raise ValueError("FlacBank: closed")
        i = int(i)
        if not 0 <= i < len(self):
            raise ValueError(f"FlacBank.file_bytes: file {i} is not in 0..{len(self) - 1}")
        frames = self._data[self._offs[i]:self._offs[i] + self._lens[i]].cpu().numpy().tobytes()
        if self._heads is not None:
            return self._heads[i] + frames
        src = self._infos[i]
        si = flacgpu.StreamInfo.new(int(src.sample_rate), self.channels, self.bits, int(src.interchannel_samples),
                                    int(src.max_block_size))
        ctypes.memmove(si.md5, src.md5, 16)
        first = self._first[i]
        n_frames = flacgpu.IndexResult.from_buffer_copy(self._ires[16 * i:16 * i + 16].cpu().numpy().tobytes()).n_frames
        for size in self._fbytes[first:first + n_frames].cpu().tolist():
            si.update_frame_size(int(size))
        return flacgpu.header_bytes(si, False) + flacgpu.vorbis_comment_bytes(True) + frames

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

    def samples_at(self, rate: int) -> list:
        """The samples every file holds when delivered at `rate` (ceil(samples * rate / its own rate));
        ValueError naming the first file whose ratio to `rate` the resampler does not serve."""
        rate = int(rate)
        for i, src in enumerate(self.sample_rates):
            why = _rate_error("FlacBank", i, src, rate)
            if why:
                raise ValueError(why)
        return [_out_samples(n, src, rate) for n, src in zip(self.samples, self.sample_rates)]

    def crops(self, file: Sequence[int], start: Sequence[int], length: int, dtype=None, planar: bool = True,
              pad: bool = True, out=None, strict: bool = True, rate: Optional[int] = None, fir: Optional["FirBank"] = None,
              fir_index: Optional[Sequence[int]] = None):
        """Samples [start[w], start[w] + length) of file[w] for every w -> (x, n): x of shape
        [W, channels, length] (planar) or [W, length, channels] in dtype (torch.float32 -- the
        default --, float16, bfloat16: sample * 2^-(bits-1); int32: the sample), n[w] the samples
        crop w really holds (fewer where it runs into the end of its file; the rest of x is zero,
        written by the kernel with pad=True, by a memset before it with pad=False).  The work is
        queued on torch.cuda.current_stream(device); the call waits for it.  strict: raise
        FlacGpuError for the first crop whose status is not OK; strict=False returns
        (x, n, statuses) instead.  out: a contiguous tensor of x's shape, dtype and device to fill.
        rate: start and length are in samples at that sample rate (samples_at(rate) per file) and x is
        at that rate: crops of files already at it are delivered as without it, bit for bit, the
        others through the polyphase filter of flacgpu_decode_windows_device_resample, one call per
        source rate (and per 65535 crops); float dtypes only; a file whose ratio to `rate` is not
        served raises ValueError when a crop names it.
        fir, fir_index: a FirBank and one filter index a crop: crop w is delivered convolved with that
        filter (its taps at the delivered rate) by the rule of flacgpu_decode_windows_device_fir, over
        the file's own samples before and after the crop, zeros only past the file's ends; float
        dtypes only.  A filter of one tap 1.0 delivers the crop as without `fir`, bit for bit."""
        if self._dec is None:
            raise ValueError("FlacBank: closed")
        return _crops("FlacBank", self.device, len(self), self.channels, [(self, None)], lambda f: (0, f), lambda fmt: None,
                      file, start, length, dtype, planar, pad, out, strict,
                      rate=None if rate is None else int(rate), rate_of=self.sample_rates.__getitem__, fir=fir,
                      fir_index=fir_index)

    def features(self, file: Sequence[int], start: Sequence[int], frames: int, n_fft: int, hop: int, filters=None,
                 log: Optional[str] = None, floor: float = 1e-10, dtype=None, out=None, strict: bool = True,
                 rate: Optional[int] = None):
        """`frames` short-time power frames of file[w] for every w, frame t centred at sample
        start[w] + t * hop -> (x, n), or (x, n, statuses) with strict=False: x of shape
        [W, channels, rows, frames]; n[w] the frames whose centre lies inside the file.  Frames are
        computed from the stream's own samples around the crop (zeros only past the file's ends), by
        the rule of flacgpu_decode_windows_device_features: a periodic Hann window of n_fft, the
        power of the n_fft // 2 + 1 bins, and with `filters` (float32 [rows, bins], mel_filters for
        one) their sums over the bins.  log: None (linear power), "ln" or "log10": the kernel then
        delivers float32 and x is torch.log / torch.log10 of clamp_min(floor), cast to dtype.
        dtype: torch.float32 (default), float16 (linear power above 65504 becomes inf), bfloat16.
        rate, out, strict and the stream semantics are those of crops."""
        if self._dec is None:
            raise ValueError("FlacBank: closed")
        return _features("FlacBank", self.device, len(self), self.channels, [(self, None)], lambda f: (0, f), file, start, frames,
                         n_fft, hop, filters, log, floor, dtype, out, strict, None if rate is None else int(rate),
                         self.sample_rates.__getitem__)

    def _tables(self):
        return (self._data.data_ptr(), self._first, self._off.data_ptr(), self._fbytes.data_ptr(), self._ires.data_ptr(),
                self._pos.data_ptr(), self._totals.data_ptr())

    def levels(self, hop: int, span: int = 1 << 20, scratch_bytes: int = 1 << 30) -> "BankLevels":
        """The levels of the whole bank in one pass, nothing delivered: every file cut into blocks of
        `hop` samples (the last perhaps short), and of every block and channel the peak max |x|, the
        exact sum and the energy -- the exact sum of squares rounded once to float64 -- by the rule of
        flacgpu_levels_windows_device -> BankLevels.  A file is measured in windows of the largest
        multiple of hop that is not above max(span, hop) samples, so every block lies in one window;
        the windows go in calls of at most 65535 whose covering frames fit scratch_bytes of decoded
        PCM (a call holds one window at least), queued on torch.cuda.current_stream(device); the
        method waits for them and raises FlacGpuError for a window that is not OK."""
        import torch

        if self._dec is None:
            raise ValueError("FlacBank: closed")
        hop, span, scratch_bytes = int(hop), int(span), int(scratch_bytes)
        if not 1 <= hop <= flacgpu.LEVELS_MAX_HOP:
            raise ValueError(f"FlacBank.levels: the hop is 1 to 2^31 - 1 samples, not {hop}")
        if span < 1 or scratch_bytes < 1:
            raise ValueError("FlacBank.levels: span and scratch_bytes are at least 1")
        C, per = self.channels, self.channels * (self.bits // 8)
        win = max(span, hop) // hop * hop
        first, blocks, at = [], [], 0
        for n in self.samples:
            first.append(at)
            blocks.append((n + hop - 1) // hop)
            at += blocks[-1]
        calls, cur, used = [], [], 0  # a call: [(file, start, count, first record, records)]
        for i, n in enumerate(self.samples):
            slack = 2 * int(self._infos[i].max_block_size)  # the covering frames reach a block past either end at most
            for s in range(0, n, win):
                count = min(win, n - s)
                need = (count + slack) * per + 16
                if cur and (len(cur) == MAX_WINDOWS or used + need > scratch_bytes):
                    calls.append(cur)
                    cur, used = [], 0
                cur.append((i, s, count, (first[i] + s // hop) * C, (count + hop - 1) // hop * C))
                used += need
        if cur:
            calls.append(cur)
        W = sum(len(c) for c in calls)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            peak = torch.zeros((at, C), dtype=torch.int32, device=self.device)  # the kernel's uint32
            total = torch.zeros((at, C), dtype=torch.int64, device=self.device)
            energy = torch.zeros((at, C), dtype=torch.float64, device=self.device)
            d_res = torch.empty(32 * max(W, 1), dtype=torch.uint8, device=self.device)
            row = 0
            for c in calls:
                self._dec.levels_windows_device(*self._tables(), [w[:3] for w in c], hop, peak.data_ptr(), total.data_ptr(),
                                                energy.data_ptr(), [w[3] for w in c], [w[4] for w in c],
                                                d_res.data_ptr() + 32 * row, stream=st)
                row += len(c)
            rows = (flacgpu.WindowResult * max(W, 1)).from_buffer_copy(d_res.cpu().numpy().tobytes())  # waits for st
            row = 0
            for c in calls:
                for i, s, count, _, _ in c:
                    r = rows[row]
                    row += 1
                    if r.status != flacgpu.WINDOW_OK or r.n_samples != count:
                        raise flacgpu.FlacGpuError(-2, f"FlacBank.levels: file {i} from sample {s} is "
                                                       f"{WINDOW_STATUS.get(int(r.status), int(r.status))} ({r.n_samples} of {count} samples)")
            peak = peak.to(torch.int64) & 0xFFFFFFFF
        return BankLevels(peak, total, energy, first, blocks, hop, list(self.samples), self.bits)

    def crop_levels(self, file: Sequence[int], start: Sequence[int], length: int, strict: bool = True):
        """The levels of samples [start[w], start[w] + length) of file[w], one block a crop ->
        (peak, sum, energy, n): int64, int64 and float64 tensors [W, channels] by the rule of
        flacgpu_levels_windows_device with hop = length, and n[w] the samples crop w really holds, as
        in crops (a crop that holds none gives zeros).  strict and the stream semantics are those of
        crops: strict=False returns (peak, sum, energy, n, statuses)."""
        import torch

        if self._dec is None:
            raise ValueError("FlacBank: closed")
        W, length = len(file), int(length)
        if len(start) != W:
            raise ValueError("FlacBank.crop_levels: file and start differ in length")
        if (not 0 <= length <= flacgpu.LEVELS_MAX_HOP or any(not 0 <= int(f) < len(self) for f in file)
                or any(int(s) < 0 for s in start)):
            raise ValueError("FlacBank.crop_levels: a file index, a start or the length (at most 2^31 - 1) is out of range")
        C = self.channels
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            peak = torch.zeros((W, C), dtype=torch.int32, device=self.device)  # the kernel's uint32
            total = torch.zeros((W, C), dtype=torch.int64, device=self.device)
            energy = torch.zeros((W, C), dtype=torch.float64, device=self.device)
            d_res = torch.zeros(32 * max(W, 1), dtype=torch.uint8, device=self.device)  # length 0: OK, no samples
            for w0 in range(0, W if length else 0, MAX_WINDOWS):
                part = range(w0, min(w0 + MAX_WINDOWS, W))
                self._dec.levels_windows_device(*self._tables(), [(int(file[w]), int(start[w]), length) for w in part], length,
                                                peak.data_ptr(), total.data_ptr(), energy.data_ptr(), [w * C for w in part],
                                                [C] * len(part), d_res.data_ptr() + 32 * w0, stream=st)
            rows = (flacgpu.WindowResult * max(W, 1)).from_buffer_copy(d_res.cpu().numpy().tobytes())  # waits for st
            peak = peak.to(torch.int64) & 0xFFFFFFFF
        n = [int(rows[w].n_samples) for w in range(W)]
        statuses = [int(rows[w].status) for w in range(W)]
        if strict:
            for w, s in enumerate(statuses):
                if s != flacgpu.WINDOW_OK:
                    bad = f", frame {rows[w].first_bad_frame}" if s == flacgpu.WINDOW_BAD_FRAME else ""
                    raise flacgpu.FlacGpuError(-2, f"FlacBank.crop_levels: crop {w} (file {int(file[w])}, start {int(start[w])}) is "
                                                   f"{WINDOW_STATUS.get(s, s)}{bad}")
            return peak, total, energy, n
        return peak, total, energy, n, statuses


class BankLevels:
    """What FlacBank.levels returns: device tensors peak (int64), sum (int64) and energy (float64) of
    shape [blocks, channels] over all files' blocks, file i's being rows first[i] to first[i] +
    blocks[i]; block j of a file holds its samples [j * hop, min((j + 1) * hop, samples))."""

    def __init__(self, peak, total, energy, first, blocks, hop, samples, bits):
        self.peak, self.sum, self.energy = peak, total, energy
        self.first, self.blocks, self.hop, self.samples, self.bits = first, blocks, hop, samples, bits

    def file(self, i: int):
        """(peak, sum, energy) of file i: views [blocks[i], channels]."""
        i = int(i)
        if not 0 <= i < len(self.first):
            raise ValueError(f"BankLevels: file {i} is not in 0..{len(self.first) - 1}")
        a, b = self.first[i], self.first[i] + self.blocks[i]
        return self.peak[a:b], self.sum[a:b], self.energy[a:b]

    def block_samples(self, i: int):
        """The samples every block of file i holds: hop, the last block's perhaps fewer (float64 [blocks[i]])."""
        import torch

        n = torch.full((self.blocks[int(i)],), float(self.hop), dtype=torch.float64, device=self.energy.device)
        if self.blocks[int(i)]:
            n[-1] = float(self.samples[int(i)] - (self.blocks[int(i)] - 1) * self.hop)
        return n

    def rms_dbfs(self, i: int):
        """10 * log10(energy / samples in the block / 4^(bits - 1)) of file i, float64 [blocks[i], channels]:
        0 dB is a full-scale square wave; -inf is digital silence.  Torch's arithmetic over the exact
        energies: not part of the library's rule."""
        import torch

        e = self.file(i)[2]
        return 10.0 * torch.log10(e / self.block_samples(i)[:, None] / float(4 ** (self.bits - 1)))

    def active(self, i: int, threshold_db: float):
        """The blocks of file i where any channel's RMS reaches threshold_db: bool [blocks[i]]."""
        return (self.rms_dbfs(i) >= float(threshold_db)).any(dim=1)


MIX_MAX_CHANNELS = 8


def _is_weights(mix) -> bool:
    """A group's mix is a list of channel masks, or a [K, C] float32 numpy array of weights."""
    return mix is not None and not isinstance(mix, list)


def _mix_entry(given):
    """A channel_map entry as ("masks", [int]) or ("weights", float32 [K, C]); ValueError(why) for
    an entry that is neither K integers nor K rows of numbers."""
    import numpy as np

    if hasattr(given, "detach") and hasattr(given, "numpy"):  # a torch tensor
        if getattr(given, "is_cuda", False):
            raise ValueError("it is a tensor on a device; weights are given on the CPU")
        given = given.detach().numpy()
    if isinstance(given, np.ndarray):
        if given.ndim == 1:
            return "masks", [int(m) for m in given]
        if given.ndim != 2:
            raise ValueError(f"it has {given.ndim} dimensions; masks have one, weights two")
        rows = list(given)
    else:
        rows = list(given)
        nested = [isinstance(r, (list, tuple, np.ndarray)) or (hasattr(r, "detach") and hasattr(r, "numpy")) for r in rows]
        if not any(nested):
            return "masks", [int(m) for m in rows]
        if not all(nested):
            raise ValueError("it mixes masks and rows of weights: give K integers, or K rows of numbers")
    try:
        w = np.ascontiguousarray(np.asarray([np.asarray(r, dtype=np.float64) for r in rows]), dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("its rows are not numbers, or differ in length") from None
    if w.ndim != 2:
        raise ValueError("its rows are not rows of numbers of one length")
    return "weights", w


def _weights_error(C: int, K: int, w) -> Optional[str]:
    """Why the float32 matrix w is no valid weighted mix of C channels to K (the library's
    flacgpu_mix_weights_valid decides), or None."""
    import numpy as np

    if w.shape != (K, C):
        return f"it has {w.shape[0]} rows of {w.shape[1]} weights, not {K} rows of {C}"
    if flacgpu.mix_weights_valid(w):
        return None
    for k in range(K):
        for c in range(C):
            if not flacgpu.mix_weights_valid(w[k:k + 1, c:c + 1]):
                return (f"weight [{k}][{c}] ({float(w[k, c])!r}) is neither 0 nor a finite number of magnitude "
                        f"2^-32 to 2^32")
    return "the library refuses it"


_ITU = {  # RFC 9639's channel orders: l / r own front, c centre, f LFE, bl / br own-side back or side, bc back centre
    3: ("l", "r", "c"), 4: ("l", "r", "bl", "br"), 5: ("l", "r", "c", "bl", "br"), 6: ("l", "r", "c", "f", "bl", "br"),
    7: ("l", "r", "c", "f", "bc", "bl", "br"), 8: ("l", "r", "c", "f", "bl", "br", "bl", "br")}


def _downmix(C: int, K: int, kind: str):
    """The float32 [K, C] matrix of downmix `kind` for C channels to K, or None where it has none."""
    import math

    import numpy as np

    if kind == "mean":
        if K != 1 or not 1 <= C <= MIX_MAX_CHANNELS:
            return None
        return np.full((1, C), np.float32(1.0 / C), dtype=np.float32)
    if kind != "itu" or K not in (1, 2) or C not in _ITU:
        return None
    a = math.sqrt(0.5)
    left = {"l": 1.0, "r": 0.0, "c": a, "f": 0.0, "bl": a, "br": 0.0, "bc": 0.5}
    right = {"l": 0.0, "r": 1.0, "c": a, "f": 0.0, "bl": 0.0, "br": a, "bc": 0.5}
    rows = [[left[r] for r in _ITU[C]], [right[r] for r in _ITU[C]]]
    if K == 1:
        rows = [[x + y for x, y in zip(*rows)]]
    return np.array([[v / math.fsum(row) for v in row] for row in rows], dtype=np.float64).astype(np.float32)


def downmix_matrix(C: int, K: int, kind: str):
    """The K rows of C float32 weights FlacMixBank(downmix=kind) uses for sources of C channels.

    "mean": K = 1, any C in 1..8: every weight is (float)(1 / C).  "itu": K = 1 or 2, C = 3..8 in
    RFC 9639's channel order (L R C; FL FR BL BR; FL FR FC BL BR; FL FR FC LFE BL BR; FL FR FC LFE
    BC SL SR; FL FR FC LFE BL BR SL SR).  The left row, unnormalised, with a = sqrt(0.5): the own
    front 1, FC a, LFE 0, every back or side channel of its own side a, BC 0.5, the other side 0;
    the right row mirrors it; K = 1 is the sum of the two.  Every row is divided by its own sum in
    double and rounded once to float32, so a full-scale input stays in [-1, 1] up to rounding.
    ValueError for any other (C, K, kind)."""
    C, K = int(C), int(K)
    if kind not in ("mean", "itu"):
        raise ValueError(f"downmix_matrix: kind is 'mean' or 'itu', not {kind!r}")
    w = _downmix(C, K, kind)
    if w is None:
        raise ValueError(f"downmix_matrix: there is no {kind!r} mix of {C} channels to {K}")
    return w


def _mix_error(C: int, masks: Sequence[int], integers: bool = False) -> Optional[str]:
    """Why `masks` is no valid mix of a source of C channels (the rule of
    flacgpu_decode_windows_device_mix, checked here so that it is a ValueError before any call), or None."""
    for k, m in enumerate(masks):
        if not 0 <= m <= 255:
            return f"mask {k} is not an integer in 0..255"
        if m >> C:
            return f"mask {k} ({m:#x}) names a channel at or above {C}"
        count = bin(m).count("1")
        if count not in (0, 1, 2, 4, 8):
            return f"mask {k} ({m:#x}) is a mean of {count} channels; 2, 4 and 8 are offered"
        if integers and count > 1:
            return f"mask {k} ({m:#x}) is a mean, which int32 cannot deliver"
    return None


def _default_masks(C: int, K: int) -> Optional[list]:
    if C == K:
        return [1 << k for k in range(K)]
    if C == 1:
        return [1] * K
    if K == 1 and C in (2, 4, 8):
        return [(1 << C) - 1]
    return None


class FlacMixBank:
    """FLAC files of any channel counts and depths, crops of any of them as `channels` channels.

    The files are grouped by (channels, bits), in file order; every group is a FlacBank of its own
    -- one decode context, one upload, one index -- and a crop is delivered by its group through
    flacgpu_decode_windows_device_mix with the group's channel masks: channel_map[C], a list of
    `channels` masks (bit c: source channel c; 0, 1, 2, 4 or 8 bits) for sources of C channels,
    or else the default: identity where C == channels, the one channel to every output where
    C == 1, the mean of all where channels == 1 and C is 2, 4 or 8.  channel_map[C] may instead be
    `channels` rows of C numbers (nested sequences, a [channels, C] numpy array or CPU tensor): a
    weight matrix, converted to float32, every weight 0 or of magnitude 2^-32 to 2^32; output
    channel k of such a group is the fused multiply-add chain of row k over the source channels
    (flacgpu_decode_windows_device_to), e.g. {2: [[0.5, 0.5], [0.5, -0.5]]} for mid/side.  downmix
    ("mean" or "itu", see downmix_matrix) gives such a matrix to the (C, channels) pairs for which
    neither channel_map nor the default has a mix; without it they are refused.  Without sample_rate, rates
    are reported, never converted.  With it every crop is stated and delivered at that rate: files
    at another rate go through flacgpu_decode_windows_device_resample (float dtypes only); `samples`
    stays in source samples, `out_samples` counts them at sample_rate.  A bank takes no locks: one
    bank per thread."""

    def __init__(self, files: Sequence[bytes], channels: int, device: int = 0, max_frames: int = 4096,
                 channel_map: Optional[dict] = None, sample_rate: Optional[int] = None, downmix: Optional[str] = None):
        who, K = "FlacMixBank", int(channels)
        if downmix not in (None, "mean", "itu"):
            raise ValueError(f"{who}: downmix is None, 'mean' or 'itu', not {downmix!r}")
        self._groups: list = []
        if len(files) == 0:
            raise ValueError(f"{who}: no files")
        if len(files) > 65535:
            raise ValueError(f"{who}: more than 65535 files")
        if not 1 <= K <= MIX_MAX_CHANNELS:
            raise ValueError(f"{who}: channels is {K}, not 1 to {MIX_MAX_CHANNELS}")
        parsed = [_parse(who, i, f) for i, f in enumerate(files)]
        self.channels = K
        self.file_channels = [int(si.channels) for si, _ in parsed]
        self.file_bits = [int(si.bit_depth) for si, _ in parsed]
        self.sample_rates = [int(si.sample_rate) for si, _ in parsed]
        self.compressed_bytes = sum(len(b) for _, b in parsed)
        members: dict = {}  # (channels, bits) -> the caller's file indices, in order
        for i in range(len(files)):
            members.setdefault((self.file_channels[i], self.file_bits[i]), []).append(i)
        masks_of = {}
        for (C, bits), idx in members.items():
            if C in masks_of:
                continue
            given = channel_map.get(C) if channel_map else None
            if given is not None:
                try:
                    form, given = _mix_entry(given)
                    why = _weights_error(C, K, given) if form == "weights" else None
                except ValueError as e:
                    form, why = "weights", str(e)
                if form == "weights":
                    if why:
                        raise ValueError(f"{who}: channel_map[{C}], which file {idx[0]} needs, is not valid: {why}")
                    masks_of[C] = given
                    continue
            masks = given if given is not None else _default_masks(C, K)
            if masks is None and downmix is not None:
                masks_of[C] = _downmix(C, K, downmix)
                if masks_of[C] is not None:
                    continue
            if masks is None:
                raise ValueError(f"{who}: file {idx[0]} has {C} channels and there is no default mix of {C} channels "
                                 f"to {K}: give channel_map[{C}]")
            why = f"it has {len(masks)} masks, not {K}" if len(masks) != K else _mix_error(C, masks)
            if why:
                raise ValueError(f"{who}: channel_map[{C}], which file {idx[0]} needs, is not valid: {why}")
            masks_of[C] = masks
        for i, (si, _) in enumerate(parsed):
            _check_blocks(who, i, si)
        self.sample_rate = None if sample_rate is None else int(sample_rate)
        if self.sample_rate is not None:
            for i, src in enumerate(self.sample_rates):
                why = _rate_error(who, i, src, self.sample_rate)
                if why:
                    raise ValueError(why)

        # ---- everything below needs the device
        self._where = [None] * len(files)  # file -> (group, its index there)
        self.samples = [0] * len(files)
        try:
            for g, ((C, bits), idx) in enumerate(members.items()):
                bank = FlacBank([files[i] for i in idx], device=device, max_frames=max_frames,
                                _group=(who, idx, [parsed[i] for i in idx]))
                self._groups.append((bank, masks_of[C]))
                for j, i in enumerate(idx):
                    self._where[i] = (g, j)
                    self.samples[i] = bank.samples[j]
        except Exception:
            self.close()
            raise
        self.device = self._groups[0][0].device
        self.bits = sorted(set(self.file_bits))  # the depths the bank holds
        if self.sample_rate is not None:
            self.out_samples = [_out_samples(n, src, self.sample_rate) for n, src in zip(self.samples, self.sample_rates)]

    def close(self) -> None:
        for bank, _ in getattr(self, "_groups", []):
            bank.close()
        self._groups = []

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
              pad: bool = True, out=None, strict: bool = True, fir: Optional["FirBank"] = None,
              fir_index: Optional[Sequence[int]] = None):
        """FlacBank.crops over the mixed bank -> (x, n), or (x, n, statuses) with strict=False: x of
        shape [W, channels, length] (planar) or [W, length, channels], every crop mixed to the bank's
        channels by its file's masks; n and the statuses in the caller's order.  float dtypes scale
        each file by its own depth; dtype=torch.int32 needs a bank of one depth (the integers of two
        depths have different scales) and masks without a mean.  The crops are routed to their
        format groups; every group queues its calls (at most 65535 windows each) on
        torch.cuda.current_stream(device) into the one x, and the call waits once per such call of
        a group that has crops, then once for the results.  A damaged frame in one file harms no
        crop of another.  In a bank with a sample_rate, start and length are in samples at that rate
        (out_samples per file), a group's crops go in one call per source rate, and int32 is refused.
        fir, fir_index: as in FlacBank.crops, the filter over the mixed (and resampled) channels."""
        who = "FlacMixBank"
        if not self._groups:
            raise ValueError(f"{who}: closed")

        def check(fmt):
            if fmt != flacgpu.SAMPLE_I32:
                return
            for bank, masks in self._groups:
                if _is_weights(masks):
                    raise ValueError(f"{who}: int32 crops of {bank.channels}-channel files, which are mixed by weights: "
                                     f"a weighted sample has no integer value to deliver")
            if len(self.bits) > 1:
                raise ValueError(f"{who}: int32 crops of a bank that holds depths {self.bits}: the integers would have "
                                 f"different scales")
            for bank, masks in self._groups:
                why = _mix_error(bank.channels, masks, integers=True)
                if why:
                    raise ValueError(f"{who}: int32 crops of {bank.channels}-channel files: {why}")

        return _crops(who, self.device, len(self), self.channels, self._groups, self._where.__getitem__, check, file, start,
                      length, dtype, planar, pad, out, strict, rate=self.sample_rate, rate_of=self.sample_rates.__getitem__,
                      fir=fir, fir_index=fir_index)

    def features(self, file: Sequence[int], start: Sequence[int], frames: int, n_fft: int, hop: int, filters=None,
                 log: Optional[str] = None, floor: float = 1e-10, dtype=None, out=None, strict: bool = True):
        """FlacBank.features over the mixed bank -> (x, n), or (x, n, statuses) with strict=False: x of
        shape [W, channels, rows, frames], every crop mixed to the bank's channels by its file's masks
        before it is framed; in a bank with a sample_rate, start and hop are in samples at that rate
        and files at another go through the resampler first.  Routed and queued as crops are."""
        if not self._groups:
            raise ValueError("FlacMixBank: closed")
        return _features("FlacMixBank", self.device, len(self), self.channels, self._groups, self._where.__getitem__, file, start,
                         frames, n_fft, hop, filters, log, floor, dtype, out, strict, self.sample_rate,
                         self.sample_rates.__getitem__)
