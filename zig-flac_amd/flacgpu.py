"""ctypes binding of libflacgpu.so (include/flacgpu.h) for tests and the benchmark.

This is plumbing over the C ABI: every encode runs in the gfx950 HIP kernels
of libflacgpu.so.  There is no CPU fallback -- if the library or a gfx950
device is missing, construction raises.

The class names mirror the reference's Zig interface (src/lib.zig):
`Encoder.write_frame` is `Encoder.writeFrame` (src/lib/encoder.zig:234),
`Config.default` is `Config.default` (encoder.zig:642-655).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLACGPU_LIB", os.path.join(HERE, "build", "libflacgpu.so"))

OK = 0
ERRORS = {
    -1: "InvalidConfig",
    -2: "InvalidInput",
    -3: "OutOfMemory",
    -4: "WriteFailed (output too small)",
    -5: "DeviceError",
    -6: "InternalError",
}

K_ANALYZE, K_ANALYZE_TAIL, K_SCAN, K_PACK, K_MD5 = range(5)
MD5_HOST, MD5_DEVICE = 0, 1
KERNEL_NAMES = ["analyze", "analyze_tail", "scan", "pack", "md5"]


class FlacGpuError(RuntimeError):
    def __init__(self, code: int, where: str):
        super().__init__(f"{where}: {ERRORS.get(code, code)} ({code})")
        self.code = code


class Config(ctypes.Structure):
    """flacgpu_config == Encoder.Config + Feature (encoder.zig:609-656)."""

    _fields_ = [
        ("sample_rate", ctypes.c_uint32),
        ("block_size", ctypes.c_uint16),
        ("channels", ctypes.c_uint8),
        ("bits_per_sample", ctypes.c_uint8),
        ("stereo_decorrelation", ctypes.c_uint8),
        ("max_rice_part_order", ctypes.c_uint8),
        ("max_rice_param", ctypes.c_uint8),
        ("prediction", ctypes.c_uint8),
    ]

    @classmethod
    def default(cls, channels: int, bits: int, sample_rate: int) -> "Config":
        return cls(sample_rate, 4096, channels, bits, 1, 8, 30, 0)


class SubframeRecord(ctypes.Structure):
    _fields_ = [
        ("type", ctypes.c_uint8),
        ("waste", ctypes.c_uint8),
        ("bits", ctypes.c_uint8),
        ("order", ctypes.c_uint8),
        ("part_order", ctypes.c_uint8),
        ("method", ctypes.c_uint8),
        ("written", ctypes.c_uint8),
        ("pad", ctypes.c_uint8),
        ("pad2", ctypes.c_uint32),
        ("estimate", ctypes.c_uint64),
        ("constant", ctypes.c_int64),
        ("params", ctypes.c_uint8 * 256),
        ("lpc_precision", ctypes.c_uint8),
        ("lpc_shift", ctypes.c_int8),
        ("pad3", ctypes.c_uint8 * 6),
        ("lpc_coefs", ctypes.c_int32 * 32),
    ]


class FrameRecord(ctypes.Structure):
    _fields_ = [
        ("channel_code", ctypes.c_uint32),
        ("n_cand", ctypes.c_uint32),
        ("frame_bytes", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
        ("cand", SubframeRecord * 8),
    ]


class Md5State(ctypes.Structure):
    """flacgpu_md5_state: one stream's MD5 chaining value carried across calls."""
    _fields_ = [("h", ctypes.c_uint32 * 4), ("bytes", ctypes.c_uint64), ("finished", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def md5_states(n: int) -> bytes:
    """n freshly initialised flacgpu_md5_state records (32 bytes each), ready to upload."""
    arr = (Md5State * max(n, 1))()
    load_library().flacgpu_md5_state_init(arr, n)
    return bytes(arr)[: 32 * n]


def md5_many(chunks: Sequence, final: Optional[Sequence[bool]] = None, states=None) -> list:
    """flacgpu_md5_many: advance len(chunks) independent MD5 chains on the library's host pool
    (md5.zig:3-31).  `states` (an (Md5State * n) array, or None for fresh chains) is updated in
    place; returns the digests (16 bytes each; None for a chain that is not final)."""
    import numpy as np

    n = len(chunks)
    views = [np.frombuffer(c, dtype=np.uint8) if len(c) else np.zeros(1, np.uint8) for c in chunks]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[v.ctypes.data for v in views])
    lens = (ctypes.c_uint64 * max(n, 1))(*[len(c) for c in chunks])
    fin = (ctypes.c_uint8 * max(n, 1))(*[1 if f else 0 for f in final]) if final is not None else None
    dig = (ctypes.c_uint8 * max(16 * n, 1))()
    _check(load_library().flacgpu_md5_many(n, ptrs, lens, fin, states, dig), "md5_many")
    raw = bytes(dig)
    return [raw[16 * i:16 * i + 16] if final is None or final[i] else None for i in range(n)]


class Md5Rates(ctypes.Structure):
    """flacgpu_md5_rates: the rates the MD5 engine choice is priced with (bytes/s)."""
    _fields_ = [("host_chain", ctypes.c_double * 4), ("host_chains", ctypes.c_uint32 * 4), ("device_lane", ctypes.c_double),
                ("device_chip", ctypes.c_double), ("host_workers", ctypes.c_int32), ("measured", ctypes.c_int32)]

    def as_dict(self) -> dict:
        return {"host_chain": list(self.host_chain), "host_chains": list(self.host_chains), "device_lane": self.device_lane, "device_chip": self.device_chip,
                "host_workers": self.host_workers, "measured": self.measured}


def md5_rates() -> Md5Rates:
    r = Md5Rates()
    _check(load_library().flacgpu_md5_get_rates(ctypes.byref(r)), "md5_get_rates")
    return r


def set_md5_rates(r: Optional[Md5Rates]) -> None:
    _check(load_library().flacgpu_md5_set_rates(ctypes.byref(r) if r is not None else None), "md5_set_rates")


def md5_engine_for(n_streams: int, max_len: int, total_len: int) -> int:
    return int(load_library().flacgpu_md5_engine_for(n_streams, max_len, total_len))


class WavInfo(ctypes.Structure):
    """flacgpu_wav_info: WavReader's view of a WAV header (wav_reader.zig:116-170)."""
    _fields_ = [("sample_rate", ctypes.c_uint32), ("channels", ctypes.c_uint16), ("bits_per_sample", ctypes.c_uint16),
                ("bytes_per_sample", ctypes.c_uint16), ("pad", ctypes.c_uint16), ("samples", ctypes.c_uint64),
                ("data_offset", ctypes.c_uint64), ("data_bytes", ctypes.c_uint64)]


class StreamInfo(ctypes.Structure):
    """flacgpu_streaminfo == metadata.StreamInfo (metadata.zig:18-33)."""
    _fields_ = [("md5", ctypes.c_uint8 * 16), ("interchannel_samples", ctypes.c_uint64),
                ("min_frame_size", ctypes.c_uint32), ("max_frame_size", ctypes.c_uint32),
                ("sample_rate", ctypes.c_uint32), ("min_block_size", ctypes.c_uint16),
                ("max_block_size", ctypes.c_uint16), ("channels", ctypes.c_uint8), ("bit_depth", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 6)]

    def update_frame_size(self, size: int) -> None:
        load_library().flacgpu_streaminfo_update_frame_size(ctypes.byref(self), size)

    def bytes(self) -> bytes:
        out = ctypes.create_string_buffer(34)
        load_library().flacgpu_streaminfo_bytes(ctypes.byref(self), out)
        return out.raw

    @classmethod
    def new(cls, sample_rate: int, channels: int, bit_depth: int, samples: int, block_size: int = 4096):
        si = cls()
        load_library().flacgpu_streaminfo_init(ctypes.byref(si), sample_rate, channels, bit_depth, samples, block_size)
        return si


def wav_parse(wav: bytes) -> WavInfo:
    info = WavInfo()
    _check(load_library().flacgpu_wav_parse(wav, len(wav), ctypes.byref(info)), "wav_parse")
    return info


def header_bytes(si: StreamInfo, last: bool) -> bytes:
    out = ctypes.create_string_buffer(42)
    n = load_library().flacgpu_header_bytes(ctypes.byref(si), 1 if last else 0, out)
    return out.raw[:n]


def vorbis_comment_bytes(last: bool) -> bytes:
    out = ctypes.create_string_buffer(31)
    n = load_library().flacgpu_vorbis_comment_bytes(1 if last else 0, out)
    return out.raw[:n]


def wav_to_flac(wav: bytes, device: int = 0) -> bytes:
    """wav2flac (wav2flac.zig:10-97) of an in-memory WAV file on the GPU."""
    info = wav_parse(wav)
    cfg = Config.default(info.channels, info.bits_per_sample, info.sample_rate)
    cap = 200 + ((info.samples + 4095) // 4096 + 1) * load_library().flacgpu_frame_bound_bytes(ctypes.byref(cfg))
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_size_t(0)
    _check(load_library().flacgpu_wav_to_flac(device, wav, len(wav), out, cap, ctypes.byref(n)), "wav_to_flac")
    return out.raw[: n.value]


class Comm:
    """flacgpu_comm: one rank of a multi-GPU communicator (RCCL over xGMI inside libflacgpu.so):
    the bitstream gather of the sharded encode (wav2flac.zig:66-97 cut into
    ranks, updateFrameSize replayed in frame order on rank 0, metadata.zig:35-40)."""

    ID_BYTES = 128

    def __init__(self, comm_id: bytes, world: int, rank: int, device: int):
        self.world, self.rank, self.device = world, rank, device
        self.comm = ctypes.c_void_p()
        cid = (ctypes.c_uint8 * self.ID_BYTES).from_buffer_copy(comm_id)
        _check(load_library().flacgpu_comm_init(cid, world, rank, device, ctypes.byref(self.comm)), "comm_init")

    @staticmethod
    def unique_id() -> bytes:
        cid = (ctypes.c_uint8 * Comm.ID_BYTES)()
        _check(load_library().flacgpu_comm_unique_id(cid), "comm_unique_id")
        return bytes(cid)

    @classmethod
    def from_process_group(cls, dist, group=None, device: int = 0) -> "Comm":
        """Rank 0 of `group` makes the id, torch.distributed hands it to every rank (any backend)."""
        rank = dist.get_rank(group)
        box = [cls.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return cls(box[0], dist.get_world_size(group), rank, device)

    def gather_device(self, d_frames: int, nbytes: int, d_sizes: int, n_frames: int, d_recv: int = 0,
                      recv_cap: int = 0, d_recv_sizes: int = 0, recv_sizes_cap: int = 0, d_nbytes: int = 0,
                      stream=None):
        """flacgpu_gather_frames_device -> (total bytes, total frames) gathered on rank 0."""
        tb, tf = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(load_library().flacgpu_gather_frames_device(
            self.comm, d_frames or None, nbytes, d_nbytes or None, d_sizes or None, n_frames, d_recv or None,
            recv_cap, d_recv_sizes or None, recv_sizes_cap, ctypes.byref(tb), ctypes.byref(tf), stream),
            "gather_frames_device")
        return tb.value, tf.value

    def encode_frames_sharded(self, enc, pcm: bytes, first_frame: int = 0):
        """flacgpu_encode_frames_sharded: every rank passes the whole stream; rank 0 gets (frames,
        sizes) exactly as flacgpu_encode_frames would write them, the others (b"", [])."""
        B = enc.bits // 8
        n = len(pcm) // (enc.channels * B)
        nf = (n + enc.block_size - 1) // enc.block_size
        cap = max(nf, 1) * enc.frame_bound() + 64 if self.rank == 0 else 0
        out = ctypes.create_string_buffer(max(cap, 1))
        fb = (ctypes.c_uint32 * max(nf, 1))()
        n_out = ctypes.c_size_t(0)
        _check(load_library().flacgpu_encode_frames_sharded(enc.ctx, self.comm, pcm, B, n, first_frame, out, cap,
                                                            ctypes.byref(n_out), fb), "encode_frames_sharded")
        if self.rank != 0:
            return b"", []
        return out.raw[: n_out.value], list(fb)[:nf]

    def close(self):
        if self.comm:
            load_library().flacgpu_comm_destroy(self.comm)
            self.comm = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libflacgpu.so; raise (never fall back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `make -C zig-flac_amd` (or __graft_entry__.build())")
    # PyTorch-ROCm bundles its own HIP/HSA runtime under the same SONAME (libamdhip64.so.7).
    # Loaded first, it is the one libflacgpu.so binds to, so device pointers and streams of
    # torch tensors and of this library share one runtime.  Loaded after /opt/rocm's copy,
    # it would start a second HSA runtime on the same device, which fails to initialise
    # ("No HIP GPUs are available").  So torch, when present, is imported before the library.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    P, U32, U64, I32, SZ = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
    sig = {
        "flacgpu_config_default": (Config, [U32, U32, U32]),
        "flacgpu_open": (I32, [I32, ctypes.POINTER(Config), U32, ctypes.POINTER(P)]),
        "flacgpu_open_decoder": (I32, [I32, U32, ctypes.c_uint8, ctypes.c_uint8, U32, U32, ctypes.POINTER(P)]),
        "flacgpu_close": (None, [P]),
        "flacgpu_strerror": (ctypes.c_char_p, [I32]),
        "flacgpu_abi_version": (I32, []),
        "flacgpu_build_flags": (U32, []),
        "flacgpu_md5_get_rates": (I32, [P]),
        "flacgpu_md5_set_rates": (I32, [P]),
        "flacgpu_md5_engine_for": (I32, [U32, U64, U64]),
        "flacgpu_reference_max_frame_bytes": (SZ, [ctypes.POINTER(Config)]),
        "flacgpu_frame_bound_bytes": (SZ, [ctypes.POINTER(Config)]),
        "flacgpu_encode_frames": (I32, [P, P, U32, U64, U64, P, SZ, ctypes.POINTER(SZ), P]),
        "flacgpu_encode_frame_planar": (I32, [P, P, U32, U64, P, SZ, ctypes.POINTER(U32)]),
        "flacgpu_md5_init": (I32, [P]),
        "flacgpu_md5_update": (I32, [P, P, SZ]),
        "flacgpu_md5_final": (I32, [P, P]),
        "flacgpu_plan_create": (I32, [P, U32, P, P, U32, ctypes.POINTER(P)]),
        "flacgpu_plan_create_segments": (I32, [P, U32, P, P, U32, P, P, ctypes.POINTER(P)]),
        "flacgpu_plan_advance": (I32, [P, U64, P]),
        "flacgpu_encode_plan_device_ex": (I32, [P, P, P, P, U64, P, P, P, P, P, P, P]),
        "flacgpu_sync_check": (I32, [P, P]),
        "flacgpu_streaminfo_replay_device": (I32, [P, P, U64, P, P]),
        "flacgpu_md5_set_engine": (I32, [P, I32]),
        "flacgpu_md5_get_engine": (I32, [P]),
        "flacgpu_md5_state_init": (None, [P, SZ]),
        "flacgpu_md5_many": (I32, [U32, P, P, P, P, P]),
        "flacgpu_md5_plan_host": (I32, [P, P, P, P]),
        "flacgpu_plan_md5_engine": (I32, [P]),
        "flacgpu_plan_destroy": (None, [P]),
        "flacgpu_plan_frames": (U64, [P]),
        "flacgpu_plan_out_bound": (U64, [P]),
        "flacgpu_plan_stream_first_frame": (U64, [P, U32]),
        "flacgpu_encode_plan_device": (I32, [P, P, P, P, U64, P, P, P, P, P]),
        "flacgpu_encode_plan_device_md5_async": (I32, [P, P, P, P, U64, P, P, P, P, P, P]),
        "flacgpu_set_timing": (I32, [P, I32]),
        "flacgpu_kernel_time": (I32, [P, I32, ctypes.POINTER(U64), ctypes.POINTER(ctypes.c_double)]),
        "flacgpu_reset_timing": (I32, [P]),
        "flacgpu_set_records": (I32, [P, I32]),
        "flacgpu_set_overlap": (I32, [P, U32, U32, U32, U32]),
        "flacgpu_get_records": (I32, [P, P, U64, ctypes.POINTER(U64)]),
        "flacgpu_get_config": (I32, [P, ctypes.POINTER(Config)]),
        "flacgpu_wav_parse": (I32, [P, SZ, ctypes.POINTER(WavInfo)]),
        "flacgpu_streaminfo_init": (None, [ctypes.POINTER(StreamInfo), U32, U32, U32, U64, U32]),
        "flacgpu_streaminfo_update_frame_size": (None, [ctypes.POINTER(StreamInfo), U32]),
        "flacgpu_streaminfo_bytes": (None, [ctypes.POINTER(StreamInfo), P]),
        "flacgpu_header_bytes": (SZ, [ctypes.POINTER(StreamInfo), I32, P]),
        "flacgpu_vorbis_comment_bytes": (SZ, [I32, P]),
        "flacgpu_encode_file": (I32, [P, P, U32, U64, P, SZ, ctypes.POINTER(SZ)]),
        "flacgpu_encode_files": (I32, [P, U32, P, U32, P, P, P, P]),
        "flacgpu_wav_to_flac": (I32, [I32, P, SZ, P, SZ, ctypes.POINTER(SZ)]),
        "flacgpu_open_multi": (I32, [I32, P, ctypes.POINTER(Config), U32, ctypes.POINTER(P)]),
        "flacgpu_close_multi": (None, [P]),
        "flacgpu_multi_encode_frames": (I32, [P, P, U32, U64, U64, P, SZ, ctypes.POINTER(SZ), P]),
        "flacgpu_comm_unique_id": (I32, [P]),
        "flacgpu_comm_init": (I32, [P, I32, I32, I32, ctypes.POINTER(P)]),
        "flacgpu_comm_destroy": (None, [P]),
        "flacgpu_comm_rank": (I32, [P]),
        "flacgpu_comm_size": (I32, [P]),
        "flacgpu_gather_frames_device": (I32, [P, P, U64, P, P, U64, P, U64, P, U64, ctypes.POINTER(U64),
                                               ctypes.POINTER(U64), P]),
        "flacgpu_encode_frames_sharded": (I32, [P, P, P, U32, U64, U64, P, SZ, ctypes.POINTER(SZ), P]),
        "flacgpu_decode_frames_device": (I32, [P, P, P, P, U64, P, P, U64, P, P, P, P]),
        "flacgpu_verify_plan_device": (I32, [P, P, P, P, P, P, P, P, P]),
        "flacgpu_decode_frames": (I32, [P, P, P, U64, P, SZ, ctypes.POINTER(U64), P]),
        "flacgpu_flac_index": (I32, [P, SZ, P, ctypes.POINTER(SZ), P, SZ, ctypes.POINTER(SZ)]),
        "flacgpu_decode_file": (I32, [P, P, SZ, P, SZ, ctypes.POINTER(U64), ctypes.POINTER(I32)]),
        "flacgpu_flac_index_device": (I32, [P, P, U64, U32, U32, P, P, U64, P, P]),
        "flacgpu_flac_index_streams_device": (I32, [P, P, U32, P, P, P, P, P, P, P, P, P, P]),
        "flacgpu_decode_streams_device": (I32, [P, P, U32, P, P, P, P, P, P, P, P, P, P]),
        "flacgpu_decode_files": (I32, [P, U32, P, P, P, P, P, P, P]),
        "flacgpu_flac_positions_streams_device": (I32, [P, P, U32, P, P, P, P, P, P, P, P, P, P]),
        "flacgpu_decode_windows_device": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, P, P, P, P, P]),
        "flacgpu_decode_files_windows": (I32, [P, U32, P, P, U32, P, P, P, P, P, P, P]),
        "flacgpu_decode_windows_device_as": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, U32, U32, P, P, P, P, P]),
        "flacgpu_decode_windows_device_mix": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, U32, U32, U32, P, P, P, P, P, P]),
        "flacgpu_resample_filter": (I32, [U32, U32, ctypes.POINTER(U32), ctypes.POINTER(U32), ctypes.POINTER(U32), P, SZ,
                                          ctypes.POINTER(SZ)]),
        "flacgpu_resample_f32_host": (I32, [P, U64, U32, U32, U64, U64, P, ctypes.POINTER(U64)]),
        "flacgpu_decode_windows_device_resample": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, U32, U32, U32, P, U32, U32,
                                                         P, P, P, P, P]),
        "flacgpu_features_table": (I32, [U32, P, SZ, ctypes.POINTER(SZ)]),
        "flacgpu_features_f32_host": (I32, [P, U64, P, P, U64, U64, P, ctypes.POINTER(U64)]),
        "flacgpu_decode_windows_device_features": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, U32, U32, P, U32, U32,
                                                         P, P, P, P, P, P, P]),
        "flacgpu_mix_weights_valid": (I32, [U32, U32, P, U32]),
        "flacgpu_mix_weights_f32_host": (I32, [P, U64, U32, U32, U32, P, P]),
        "flacgpu_decode_windows_device_to": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, P, P, P, P, P, P]),
        "flacgpu_pcm_from_elements_device": (I32, [P, U32, P, P, P, U32, U32, P, P, U64, P, P]),
        "flacgpu_pcm_from_elements_host": (I32, [P, U64, U64, U32, U32, U32, U32, P, SZ, ctypes.POINTER(U64)]),
        "flacgpu_levels_windows_device": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, U32, P, P, P, P, P, P, P]),
        "flacgpu_levels_host": (I32, [P, U64, U32, U32, P, P, P]),
        "flacgpu_fir_f32_host": (I32, [P, U64, P, U32, U32, U64, U64, P, ctypes.POINTER(U64)]),
        "flacgpu_decode_windows_device_fir": (I32, [P, P, U32, P, P, P, P, P, P, U32, P, P, P, P, P, U64, U32, P, P, P, P, P, P,
                                                    P]),
    }
    # an older build named by FLACGPU_LIB (same-box A/B runs, tools/ab.sh) may predate later entry
    # points: those stay unbound there; the in-tree library must export every one
    other_build = path != os.path.join(HERE, "build", "libflacgpu.so")
    for name, (res, args) in sig.items():
        if other_build and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def exported_symbols() -> list:
    return [
        "flacgpu_config_default", "flacgpu_open", "flacgpu_close", "flacgpu_strerror", "flacgpu_abi_version",
        "flacgpu_build_flags", "flacgpu_md5_get_rates", "flacgpu_md5_set_rates", "flacgpu_md5_engine_for",
        "flacgpu_reference_max_frame_bytes", "flacgpu_frame_bound_bytes", "flacgpu_encode_frames",
        "flacgpu_encode_frame_planar", "flacgpu_md5_init", "flacgpu_md5_update", "flacgpu_md5_final",
        "flacgpu_plan_create", "flacgpu_plan_destroy", "flacgpu_plan_frames", "flacgpu_plan_out_bound",
        "flacgpu_plan_stream_first_frame", "flacgpu_encode_plan_device", "flacgpu_encode_plan_device_md5_async",
        "flacgpu_plan_create_segments", "flacgpu_plan_advance", "flacgpu_encode_plan_device_ex", "flacgpu_sync_check",
        "flacgpu_streaminfo_replay_device",
        "flacgpu_md5_set_engine", "flacgpu_md5_get_engine", "flacgpu_md5_state_init",
        "flacgpu_md5_many", "flacgpu_md5_plan_host", "flacgpu_plan_md5_engine",
        "flacgpu_set_timing",
        "flacgpu_kernel_time", "flacgpu_reset_timing", "flacgpu_set_records", "flacgpu_set_overlap", "flacgpu_get_records",
        "flacgpu_get_config", "flacgpu_wav_parse", "flacgpu_streaminfo_init", "flacgpu_streaminfo_update_frame_size",
        "flacgpu_streaminfo_bytes", "flacgpu_header_bytes", "flacgpu_vorbis_comment_bytes", "flacgpu_encode_file", "flacgpu_encode_files",
        "flacgpu_wav_to_flac", "flacgpu_open_multi", "flacgpu_close_multi", "flacgpu_multi_encode_frames",
        "flacgpu_comm_unique_id", "flacgpu_comm_init", "flacgpu_comm_destroy", "flacgpu_comm_rank",
        "flacgpu_comm_size", "flacgpu_gather_frames_device", "flacgpu_encode_frames_sharded",
        "flacgpu_decode_frames_device", "flacgpu_verify_plan_device", "flacgpu_decode_frames", "flacgpu_flac_index",
        "flacgpu_decode_file", "flacgpu_flac_index_device",
        "flacgpu_flac_index_streams_device", "flacgpu_decode_streams_device", "flacgpu_decode_files",
        "flacgpu_flac_positions_streams_device", "flacgpu_decode_windows_device", "flacgpu_decode_files_windows",
        "flacgpu_decode_windows_device_as", "flacgpu_open_decoder", "flacgpu_decode_windows_device_mix",
        "flacgpu_resample_filter", "flacgpu_resample_f32_host", "flacgpu_decode_windows_device_resample",
        "flacgpu_features_table", "flacgpu_features_f32_host", "flacgpu_decode_windows_device_features",
        "flacgpu_pcm_from_elements_device", "flacgpu_pcm_from_elements_host",
        "flacgpu_mix_weights_valid", "flacgpu_mix_weights_f32_host", "flacgpu_decode_windows_device_to",
        "flacgpu_levels_windows_device", "flacgpu_levels_host",
        "flacgpu_fir_f32_host", "flacgpu_decode_windows_device_fir",
    ]


BUILD_DIAG = 1  # FLACGPU_BUILD_DIAG
BUILD_STAMPS = 2  # FLACGPU_BUILD_STAMPS


def build_flags() -> int:
    """flacgpu_build_flags(): BUILD_DIAG for a diagnostic build (`make diag`), else 0."""
    L = load_library()
    return int(L.flacgpu_build_flags()) if hasattr(L, "flacgpu_build_flags") else BUILD_DIAG


def diag_build() -> bool:
    return bool(build_flags() & BUILD_DIAG)


STREAM_LEGACY = 1  # FLACGPU_STREAM_LEGACY: the library maps it to the HIP null stream


def _stream(h: Optional[int]) -> Optional[int]:
    """A torch/HIP stream handle as the C ABI's `void *hip_stream`: None -> NULL (the context's
    own non-blocking stream); 0 (the legacy null stream, torch's default) -> FLACGPU_STREAM_LEGACY,
    so the work stays ordered against default-stream producers and consumers."""
    if h is None:
        return None
    return STREAM_LEGACY if h == 0 else h


def _check(rc: int, where: str) -> None:
    if rc != OK:
        raise FlacGpuError(rc, where)


class Plan:
    """flacgpu_plan: a batch of streams (or stream segments) laid out in one device PCM buffer."""

    def __init__(self, enc: "Encoder", offsets: Sequence[int], samples: Sequence[int],
                 first_frames: Optional[Sequence[int]] = None, final: Optional[Sequence[bool]] = None):
        self.enc = enc
        n = len(offsets)
        self._offs = (ctypes.c_uint64 * max(n, 1))(*offsets)
        self._samp = (ctypes.c_uint64 * max(n, 1))(*samples)
        ff = (ctypes.c_uint64 * max(n, 1))(*first_frames) if first_frames is not None else None
        fin = (ctypes.c_uint8 * max(n, 1))(*[1 if f else 0 for f in final]) if final is not None else None
        h = ctypes.c_void_p()
        _check(enc.lib.flacgpu_plan_create_segments(enc.ctx, n, self._offs, self._samp, enc.bytes_per_sample, ff, fin,
                                                    ctypes.byref(h)), "plan_create_segments")
        self.handle = h
        self.n_streams = n
        self.n_frames = enc.lib.flacgpu_plan_frames(h)
        self.out_bound = enc.lib.flacgpu_plan_out_bound(h)
        self.first_frame = [enc.lib.flacgpu_plan_stream_first_frame(h, s) for s in range(n)]

    def advance(self, frames: int, stream: Optional[int] = None) -> None:
        """flacgpu_plan_advance: the next window of the same streams (frame numbers + frames)."""
        _check(self.enc.lib.flacgpu_plan_advance(self.handle, frames, _stream(stream)), "plan_advance")

    def md5_engine(self) -> int:
        """flacgpu_plan_md5_engine: MD5_HOST below the stream-count crossover, else MD5_DEVICE."""
        return self.enc.lib.flacgpu_plan_md5_engine(self.handle)

    def md5_host(self, h_pcm: int, states=None, digests: Optional[int] = None) -> None:
        """flacgpu_md5_plan_host: every segment's MD5 on the host pool from the host copy h_pcm
        (address; same offsets as the device buffer), states/digests in host memory."""
        _check(self.enc.lib.flacgpu_md5_plan_host(self.handle, h_pcm, states, digests), "md5_plan_host")

    def close(self) -> None:
        if self.handle:
            self.enc.lib.flacgpu_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# per-frame decode status (FLACGPU_DEC_*): 1..7 are minus the CPU verifier decoder's codes
DEC_OK, DEC_SYNC, DEC_HEADER, DEC_CRC8, DEC_SUBFRAME, DEC_CRC16, DEC_TRUNCATED, DEC_RANGE, DEC_MISMATCH = range(9)
K_DEC_PARSE, K_DEC_RECON = 5, 6  # FLACGPU_K_DEC_PARSE / FLACGPU_K_DEC_RECON (kernel_time ids)
K_INDEX = 7  # FLACGPU_K_INDEX: the device frame index, all its stages as one timed launch
INDEX_OK, INDEX_INVALID, INDEX_TOO_SMALL = range(3)  # flacgpu_index_result.status


class IndexResult(ctypes.Structure):
    """flacgpu_index_result (device memory, 16 bytes)."""
    _fields_ = [("n_frames", ctypes.c_uint64), ("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DecodeResult(ctypes.Structure):
    """flacgpu_decode_result: one frame's status and header fields (32 bytes)."""
    _fields_ = [("status", ctypes.c_uint32), ("block_size", ctypes.c_uint32), ("number", ctypes.c_uint64),
                ("sample_rate", ctypes.c_uint32), ("first_bad", ctypes.c_uint32), ("channel_assign", ctypes.c_uint8),
                ("bits", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 6)]


class StreamResult(ctypes.Structure):
    """flacgpu_stream_result: one stream of flacgpu_decode_streams_device (device memory, 32 bytes)."""
    _fields_ = [("n_frames", ctypes.c_uint64), ("n_samples", ctypes.c_uint64), ("index_status", ctypes.c_uint32),
                ("bad_frames", ctypes.c_uint32), ("first_bad_frame", ctypes.c_uint32),
                ("first_bad_status", ctypes.c_uint32)]


WINDOW_OK, WINDOW_BAD_INDEX, WINDOW_BAD_FRAME, WINDOW_TOO_SMALL = range(4)  # flacgpu_window_result.status


class WindowResult(ctypes.Structure):
    """flacgpu_window_result: one window of flacgpu_decode_windows_device (device memory, 32 bytes)."""
    _fields_ = [("n_samples", ctypes.c_uint64), ("first_frame", ctypes.c_uint64), ("n_frames", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("first_bad_frame", ctypes.c_uint32), ("first_bad_status", ctypes.c_uint32)]


SAMPLE_I32, SAMPLE_F32, SAMPLE_F16, SAMPLE_BF16 = range(4)  # FLACGPU_SAMPLE_*: the element formats of a delivery
ELEMENT_BYTES = {SAMPLE_I32: 4, SAMPLE_F32: 4, SAMPLE_F16: 2, SAMPLE_BF16: 2}  # their element sizes
DELIVER_PLANAR, DELIVER_PAD = 1, 2  # FLACGPU_DELIVER_*


def _u64s(v: Sequence[int]):
    return (ctypes.c_uint64 * max(len(v), 1))(*v)


def _u32s(v: Optional[Sequence[int]]):
    return (ctypes.c_uint32 * max(len(v), 1))(*v) if v is not None else None


def flac_index(buf: bytes, raw_frames: bool = False):
    """flacgpu_flac_index (host only): (StreamInfo or None, first frame offset, [frame sizes]) of a
    FLAC file in memory; raw_frames: `buf` is a bare run of frames (no "fLaC", no metadata)."""
    L = load_library()
    si = None if raw_frames else StreamInfo()
    first, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
    cap = len(buf) // 8 + 1  # a frame is at least 9 bytes
    sizes = (ctypes.c_uint32 * cap)()
    _check(L.flacgpu_flac_index(bytes(buf), len(buf), ctypes.byref(si) if si is not None else None, ctypes.byref(first),
                                sizes, cap, ctypes.byref(n)), "flac_index")
    return si, first.value, list(sizes)[: n.value]


def resample_ratio(src_rate: int, dst_rate: int):
    """(L, M, taps) of the filter that delivers src_rate at dst_rate, or None where the ratio is
    not one flacgpu_resample_filter serves (equal rates included)."""
    if not (0 < int(src_rate) <= 0xFFFFFFFF and 0 < int(dst_rate) <= 0xFFFFFFFF):
        return None
    L = load_library()
    up, down, taps, n = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0)
    rc = L.flacgpu_resample_filter(int(src_rate), int(dst_rate), ctypes.byref(up), ctypes.byref(down), ctypes.byref(taps), None,
                                   0, ctypes.byref(n))
    return (up.value, down.value, taps.value) if rc == -4 else None  # FLACGPU_ERR_OUTPUT_TOO_SMALL: valid, and its size


def resample_filter(src_rate: int, dst_rate: int):
    """flacgpu_resample_filter (host only): (L, M, taps, table) of the polyphase filter that delivers
    a stream of src_rate at dst_rate; table[p][k] a float32 numpy array of shape [L, taps].  An
    invalid ratio (equal rates included) raises FlacGpuError."""
    import numpy as np

    r = resample_ratio(src_rate, dst_rate)
    if r is None:
        raise FlacGpuError(-2, f"resample_filter: {src_rate} -> {dst_rate} is not a ratio the filter serves")
    up, down, taps = r
    table, n = np.zeros(up * taps, dtype=np.float32), ctypes.c_size_t(0)
    _check(load_library().flacgpu_resample_filter(src_rate, dst_rate, None, None, None, table.ctypes.data, table.size,
                                                  ctypes.byref(n)), "resample_filter")
    return up, down, taps, table.reshape(up, taps)


def resample_f32_host(x, src_rate: int, dst_rate: int, start: int = 0, count: Optional[int] = None):
    """flacgpu_resample_f32_host (host only): output samples [start, start + count) (count None: to
    the end) of the float32 samples x of one channel at src_rate, delivered at dst_rate; a float32
    numpy array of the samples delivered.  The statement of the rule the device follows bit for
    bit, for callers and tests: not a decode path."""
    import numpy as np

    L = load_library()
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("resample_f32_host: x is one channel of samples")
    r = resample_ratio(src_rate, dst_rate)
    if r is None:
        raise FlacGpuError(-2, f"resample_f32_host: {src_rate} -> {dst_rate} is not a ratio the filter serves")
    total = (len(x) * r[0] + r[1] - 1) // r[1]
    if start < 0 or (count is not None and count < 0):
        raise ValueError("resample_f32_host: start and count are not negative")
    room = max(total - start, 0) if count is None else min(count, max(total - start, 0))
    y = np.zeros(max(room, 1), dtype=np.float32)
    got = ctypes.c_uint64(0)
    _check(L.flacgpu_resample_f32_host(x.ctypes.data if len(x) else None, len(x), src_rate, dst_rate, start,
                                       room if count is None else count, y.ctypes.data, ctypes.byref(got)),
           "resample_f32_host")
    return y[: got.value]


class Features(ctypes.Structure):
    """flacgpu_features: n_fft (even, 16..2048), hop (1..n_fft), n_rows (0: the bins, else the rows of
    a filter bank, at most 256)."""
    _fields_ = [("n_fft", ctypes.c_uint32), ("hop", ctypes.c_uint32), ("n_rows", ctypes.c_uint32)]


FEATURES_MAX_SPAN = 1 << 31  # (frames - 1) * hop + n_fft stays below it


def features_params(n_fft: int, hop: int, filters=None):
    """(Features, filters as a contiguous float32 [rows, bins] numpy array or None, rows) after the
    host checks of the feature calls; ValueError names what is wrong."""
    import numpy as np

    n_fft, hop = int(n_fft), int(hop)
    if not (16 <= n_fft <= 2048 and n_fft % 2 == 0):
        raise ValueError(f"features: n_fft {n_fft} is not an even number in 16..2048")
    if not 1 <= hop <= n_fft:
        raise ValueError(f"features: hop {hop} is not in 1..n_fft")
    bins = n_fft // 2 + 1
    if filters is None:
        return Features(n_fft, hop, 0), None, bins
    f = np.ascontiguousarray(filters, dtype=np.float32)
    if f.ndim != 2 or f.shape[1] != bins or not 1 <= f.shape[0] <= 256:
        raise ValueError(f"features: filters is not [1..256 rows, {bins} bins]")
    if not np.isfinite(f).all():
        raise ValueError("features: filters has an entry that is not finite")
    return Features(n_fft, hop, f.shape[0]), f, f.shape[0]


def features_table(n_fft: int):
    """flacgpu_features_table (host only): the STFT table of n_fft, float32 [2, bins, n_fft]: the
    windowed cosines, then the negated windowed sines."""
    import numpy as np

    ft, _, bins = features_params(n_fft, 1)
    table, n = np.zeros(2 * bins * ft.n_fft, dtype=np.float32), ctypes.c_size_t(0)
    _check(load_library().flacgpu_features_table(ft.n_fft, table.ctypes.data, table.size, ctypes.byref(n)), "features_table")
    return table.reshape(2, bins, ft.n_fft)


def features_f32_host(x, n_fft: int, hop: int, start: int, frames: int, filters=None):
    """flacgpu_features_f32_host (host only): (y, n) -- y the float32 [rows, frames] power rows of
    `frames` frames from sample `start` of the float32 samples x of one channel, n the frames whose
    centre lies inside x.  The statement of the rule the device follows bit for bit: not a decode path."""
    import numpy as np

    ft, f, rows = features_params(n_fft, hop, filters)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 1:
        raise ValueError("features_f32_host: x is one channel of samples")
    if start < 0 or frames < 0 or (frames and (frames - 1) * ft.hop + ft.n_fft >= FEATURES_MAX_SPAN):
        raise ValueError("features_f32_host: start or frames is negative, or the span reaches 2^31")
    y, got = np.zeros((rows, max(frames, 1)), dtype=np.float32)[:, :frames].copy(), ctypes.c_uint64(0)
    _check(load_library().flacgpu_features_f32_host(x.ctypes.data if len(x) else None, len(x), ctypes.byref(ft),
                                                    f.ctypes.data if f is not None else None, start, frames,
                                                    y.ctypes.data if frames else None, ctypes.byref(got)),
           "features_f32_host")
    return y, got.value


class WindowDelivery(ctypes.Structure):
    """flacgpu_window_delivery: how flacgpu_decode_windows_device_to delivers."""
    _fields_ = [("size", ctypes.c_uint32), ("sample_format", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("out_channels", ctypes.c_uint32), ("channel_masks", ctypes.c_void_p), ("channel_weights", ctypes.c_void_p),
                ("src_rate", ctypes.c_uint32), ("dst_rate", ctypes.c_uint32), ("features", ctypes.c_void_p),
                ("filters", ctypes.c_void_p)]


def _weights(weights, who: str):
    """A weight matrix as a contiguous float32 [K, C] numpy array."""
    import numpy as np

    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.ndim != 2 or w.size == 0:
        raise ValueError(f"{who}: the weights are K rows of C numbers")
    return w


def mix_weights_valid(weights, sample_format: int = SAMPLE_F32) -> bool:
    """flacgpu_mix_weights_valid (host only): whether the [K, C] matrix is one the weighted channel
    mix takes for sample_format: K and C in 1..8, a float format, every weight 0 or 2^-32 <= |w| <= 2^32."""
    w = _weights(weights, "mix_weights_valid")
    return bool(load_library().flacgpu_mix_weights_valid(w.shape[1], w.shape[0], w.ctypes.data, int(sample_format)))


def mix_weights_f32_host(samples, bits: int, weights):
    """flacgpu_mix_weights_f32_host (host only): the weighted mix of the integer samples [n, C] of
    `bits` bits by the [K, C] matrix as a float32 numpy array [n, K].  The statement of the rule the
    device follows bit for bit, for callers and tests: not a decode path."""
    import numpy as np

    w = _weights(weights, "mix_weights_f32_host")
    x = np.asarray(samples)
    if x.ndim != 2 or x.shape[1] != w.shape[1] or x.dtype.kind not in "iu":
        raise ValueError("mix_weights_f32_host: samples is an integer array [n, C], C the columns of the weights")
    lo, hi = -(1 << (int(bits) - 1)), (1 << (int(bits) - 1)) - 1
    if x.size and (int(x.min()) < lo or int(x.max()) > hi):
        raise ValueError(f"mix_weights_f32_host: a sample is outside {bits} bits")
    x = np.ascontiguousarray(x, dtype=np.int32)
    y = np.zeros((max(len(x), 1), w.shape[0]), dtype=np.float32)[:len(x)]
    _check(load_library().flacgpu_mix_weights_f32_host(x.ctypes.data if len(x) else None, len(x), w.shape[1], int(bits),
                                                       w.shape[0], w.ctypes.data, y.ctypes.data if len(x) else None),
           "mix_weights_f32_host")
    return y


class Fir(ctypes.Structure):
    """flacgpu_fir: one filter of flacgpu_decode_windows_device_fir (host memory, 24 bytes): row r is the
    `taps` floats from float offset + r * taps of the call's device taps."""
    _fields_ = [("offset", ctypes.c_uint64), ("taps", ctypes.c_uint32), ("delay", ctypes.c_uint32),
                ("rows", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


FIR_MAX_TAPS = 4096  # of a filter of flacgpu_decode_windows_device_fir
FIR_MAX_SPAN = 1 << 31  # count + taps - 1 stays below it


def fir_f32_host(x, taps, delay: int, start: int, count: int):
    """flacgpu_fir_f32_host (host only): (y, n) -- y the float32 [count] elements of the window
    [start, start + count) of the float32 samples x of one channel through the filter `taps` (1 to
    4096 finite numbers) with `delay` (0 .. len(taps) - 1), n the samples of the window inside x; y is
    +0.0 from n on.  The statement of the rule the device follows bit for bit: not a decode path."""
    import numpy as np

    x = np.ascontiguousarray(x, dtype=np.float32)
    h = np.ascontiguousarray(taps, dtype=np.float32)
    if x.ndim != 1 or h.ndim != 1:
        raise ValueError("fir_f32_host: x is one channel of samples, taps one row of numbers")
    if not 1 <= len(h) <= FIR_MAX_TAPS or not np.isfinite(h).all() or not 0 <= int(delay) < len(h):
        raise ValueError("fir_f32_host: 1 to 4096 finite taps and a delay below their count")
    if start < 0 or count < 0 or count + len(h) - 1 >= FIR_MAX_SPAN:
        raise ValueError("fir_f32_host: start or count is negative, or the span reaches 2^31")
    y, got = np.zeros(max(count, 1), dtype=np.float32)[:count], ctypes.c_uint64(0)
    _check(load_library().flacgpu_fir_f32_host(x.ctypes.data if len(x) else None, len(x), h.ctypes.data, len(h), int(delay),
                                               start, count, y.ctypes.data if count else None, ctypes.byref(got)),
           "fir_f32_host")
    return y, got.value


LEVELS_MAX_HOP = (1 << 31) - 1  # of flacgpu_levels_windows_device and flacgpu_levels_host


def levels_host(x, hop: int):
    """flacgpu_levels_host (host only): (peak, sum, energy) of the integer samples x [n, C] cut into
    blocks of `hop` samples -- numpy arrays [ceil(n / hop), C] of uint32, int64 and float64: max |x|,
    the exact sum, and the exact sum of squares rounded once to the nearest double.  The statement of
    the rule the device follows bit for bit, for callers and tests: not a decode path."""
    import numpy as np

    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] < 1 or x.dtype.kind not in "iu":
        raise ValueError("levels_host: x is an integer array [n, C]")
    hop = int(hop)
    if not 1 <= hop <= LEVELS_MAX_HOP:
        raise ValueError("levels_host: the hop is 1 to 2^31 - 1")
    if x.size and (int(x.min()) < -(1 << 31) or int(x.max()) >= 1 << 31):
        raise ValueError("levels_host: a sample is outside 32 bits")
    x = np.ascontiguousarray(x, dtype=np.int32)
    n, C = x.shape
    blocks = (n + hop - 1) // hop
    peak = np.zeros((max(blocks, 1), C), dtype=np.uint32)[:blocks]
    total = np.zeros((max(blocks, 1), C), dtype=np.int64)[:blocks]
    energy = np.zeros((max(blocks, 1), C), dtype=np.float64)[:blocks]
    _check(load_library().flacgpu_levels_host(x.ctypes.data if n else None, n, C, hop, peak.ctypes.data if n else None,
                                              total.ctypes.data if n else None, energy.ctypes.data if n else None),
           "levels_host")
    return peak, total, energy


def pcm_from_elements_host(x, bits: int, sample_format: int, planar: bool = True, samples: Optional[int] = None,
                           plane_stride: Optional[int] = None):
    """flacgpu_pcm_from_elements_host (host only): (PCM bytes rounded up to 4 with zero pads, clipped)
    of one stream whose elements are the numpy array x: [C, T] with planar (plane_stride elements
    between planes: default the row stride of x), else [T, C]; float16 and bfloat16 as uint16 bit
    patterns, float32 as float32 or uint32, int32 as int32.  The statement of the rule the device
    follows bit for bit: not a conversion path."""
    import numpy as np

    x = np.asarray(x)
    if x.ndim != 2 or x.dtype.itemsize != ELEMENT_BYTES.get(sample_format, 0):
        raise ValueError("pcm_from_elements_host: x is [C, T] or [T, C] elements of the format's size")
    C, T = (x.shape[0], x.shape[1]) if planar else (x.shape[1], x.shape[0])
    if samples is not None:
        T = samples
    if planar and plane_stride is None:
        x = np.ascontiguousarray(x)
        plane_stride = x.shape[1]
    elif not planar:
        x = np.ascontiguousarray(x)
    cap = (T * C * (bits // 8) + 3) // 4 * 4
    out = np.zeros(max(cap, 4) // 4, dtype=np.uint32)
    clipped = ctypes.c_uint64(0)
    _check(load_library().flacgpu_pcm_from_elements_host(x.ctypes.data, T, plane_stride or 0, C, bits, sample_format,
                                                         DELIVER_PLANAR if planar else 0, out.ctypes.data, cap,
                                                         ctypes.byref(clipped)), "pcm_from_elements_host")
    return out.tobytes()[:cap], clipped.value


class _DecodeOps:
    """The decode / verify entry points of a context (Encoder and Decoder share them)."""

    def decode_frames_device(self, d_frames: int, d_frame_offsets: int, d_frame_bytes: int, n_frames: int,
                             d_results: int, d_bad_count: int, d_pcm_offsets: Optional[int] = None,
                             d_pcm_out: Optional[int] = None, pcm_cap: int = 0, d_pcm_expect: Optional[int] = None,
                             stream: Optional[int] = None) -> None:
        """flacgpu_decode_frames_device: device addresses in, nothing synchronised."""
        _check(self.lib.flacgpu_decode_frames_device(self.ctx, d_frames, d_frame_offsets, d_frame_bytes, n_frames,
                                                     d_pcm_offsets or None, d_pcm_out or None, pcm_cap,
                                                     d_pcm_expect or None, d_results, d_bad_count, _stream(stream)),
               "decode_frames_device")

    def flac_index_device(self, d_data: int, length: int, d_frame_offsets: int, d_frame_bytes: int, cap: int,
                          d_result: int, stream_bits: int = 16, stream_rate: int = 0,
                          stream: Optional[int] = None) -> None:
        """flacgpu_flac_index_device: the frame table of a device-resident bare run of frames; device
        addresses in, *d_result (an IndexResult) in device memory, nothing synchronised."""
        _check(self.lib.flacgpu_flac_index_device(self.ctx, d_data, length, stream_bits, stream_rate, d_frame_offsets,
                                                  d_frame_bytes, cap, d_result, _stream(stream)), "flac_index_device")

    def flac_index_streams_device(self, d_data: int, offsets: Sequence[int], lengths: Sequence[int],
                                  table_first: Sequence[int], table_caps: Sequence[int], d_frame_offsets: int,
                                  d_frame_bytes: int, d_results: int, stream_bits: Optional[Sequence[int]] = None,
                                  stream_rates: Optional[Sequence[int]] = None, stream: Optional[int] = None) -> None:
        """flacgpu_flac_index_streams_device: the frame tables of len(offsets) bare runs of frames of one
        device buffer in one call; d_results: IndexResult per stream in device memory."""
        _check(self.lib.flacgpu_flac_index_streams_device(
            self.ctx, d_data, len(offsets), _u64s(offsets), _u64s(lengths), _u32s(stream_bits), _u32s(stream_rates),
            _u64s(table_first), _u64s(table_caps), d_frame_offsets, d_frame_bytes, d_results, _stream(stream)),
            "flac_index_streams_device")

    def decode_streams_device(self, d_data: int, offsets: Sequence[int], lengths: Sequence[int], d_pcm_out: int,
                              pcm_offsets: Sequence[int], pcm_caps: Sequence[int], d_results: int,
                              d_md5: Optional[int] = None, stream_bits: Optional[Sequence[int]] = None,
                              stream_rates: Optional[Sequence[int]] = None, stream: Optional[int] = None) -> None:
        """flacgpu_decode_streams_device: index and decode len(offsets) device-resident streams into
        their PCM regions; d_results: StreamResult per stream, d_md5: 16 bytes per stream (device)."""
        _check(self.lib.flacgpu_decode_streams_device(
            self.ctx, d_data, len(offsets), _u64s(offsets), _u64s(lengths), _u32s(stream_bits), _u32s(stream_rates),
            d_pcm_out, _u64s(pcm_offsets), _u64s(pcm_caps), d_results, d_md5 or None, _stream(stream)),
            "decode_streams_device")

    def flac_positions_streams_device(self, d_data: int, table_first: Sequence[int], table_caps: Sequence[int],
                                      d_frame_offsets: int, d_frame_bytes: int, d_index_results: int,
                                      d_frame_first_sample: int, d_stream_samples: int,
                                      stream_bits: Optional[Sequence[int]] = None,
                                      stream_rates: Optional[Sequence[int]] = None, stream: Optional[int] = None) -> None:
        """flacgpu_flac_positions_streams_device: the sample positions of len(table_first) indexed streams
        into d_frame_first_sample (laid out like the frame tables) and their totals into d_stream_samples."""
        _check(self.lib.flacgpu_flac_positions_streams_device(
            self.ctx, d_data, len(table_first), _u64s(table_first), _u64s(table_caps), d_frame_offsets, d_frame_bytes,
            d_index_results, _u32s(stream_bits), _u32s(stream_rates), d_frame_first_sample, d_stream_samples,
            _stream(stream)), "flac_positions_streams_device")

    def _window_args(self, d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                     d_stream_samples, windows):
        """The arguments the three window calls share: the context through the windows' counts."""
        return (self.ctx, d_data, len(table_first), _u64s(table_first), d_frame_offsets, d_frame_bytes, d_index_results,
                d_frame_first_sample, d_stream_samples, len(windows), _u32s([w[0] for w in windows]),
                _u64s([w[1] for w in windows]), _u64s([w[2] for w in windows]))

    def decode_windows_device(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int, d_frame_bytes: int,
                              d_index_results: int, d_frame_first_sample: int, d_stream_samples: int,
                              windows: Sequence, d_pcm_out: int, pcm_offsets: Sequence[int], pcm_caps: Sequence[int],
                              d_results: int, stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device: windows = [(stream, start, count)] over resident tables and
        positions; window w's bytes to d_pcm_out + pcm_offsets[w], d_results: WindowResult per window."""
        _check(self.lib.flacgpu_decode_windows_device(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            d_pcm_out, _u64s(pcm_offsets), _u64s(pcm_caps), d_results, _stream(stream)), "decode_windows_device")

    def decode_windows_device_as(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int, d_frame_bytes: int,
                                 d_index_results: int, d_frame_first_sample: int, d_stream_samples: int,
                                 windows: Sequence, sample_format: int, flags: int, d_out: int,
                                 out_offsets: Sequence[int], out_caps: Sequence[int], d_results: int,
                                 stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device_as: the windows of decode_windows_device as elements of
        sample_format (SAMPLE_*), laid out by flags (DELIVER_*); window w's elements from element
        out_offsets[w] of d_out on, out_caps in elements too."""
        _check(self.lib.flacgpu_decode_windows_device_as(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            sample_format, flags, d_out, _u64s(out_offsets), _u64s(out_caps), d_results, _stream(stream)),
            "decode_windows_device_as")

    def levels_windows_device(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int, d_frame_bytes: int,
                              d_index_results: int, d_frame_first_sample: int, d_stream_samples: int,
                              windows: Sequence, hop: int, d_peak: int, d_sum: int, d_energy: int,
                              out_offsets: Sequence[int], out_caps: Sequence[int], d_results: int,
                              stream: Optional[int] = None) -> None:
        """flacgpu_levels_windows_device: the windows of decode_windows_device measured, not delivered:
        every window cut into blocks of `hop` samples, and of block j, channel c the peak (uint32), the
        sum (int64) and the energy (float64) at record out_offsets[w] + j * channels + c of d_peak,
        d_sum and d_energy; out_caps in records too."""
        if not 0 <= int(hop) < 1 << 32:
            raise FlacGpuError(-2, "levels_windows_device: hop is not in 0..2^32-1")
        _check(self.lib.flacgpu_levels_windows_device(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            int(hop), d_peak, d_sum, d_energy, _u64s(out_offsets), _u64s(out_caps), d_results, _stream(stream)),
            "levels_windows_device")

    def decode_windows_device_mix(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int, d_frame_bytes: int,
                                  d_index_results: int, d_frame_first_sample: int, d_stream_samples: int,
                                  windows: Sequence, sample_format: int, flags: int, channel_masks: Sequence[int],
                                  d_out: int, out_offsets: Sequence[int], out_caps: Sequence[int], d_results: int,
                                  stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device_mix: decode_windows_device_as with len(channel_masks) output
        channels, output channel k made of the source channels whose bits channel_masks[k] has (their
        exact mean, the one, or silence); offsets and caps in elements of that channel count."""
        masks = [int(m) for m in channel_masks]
        if any(not 0 <= m <= 255 for m in masks):
            raise FlacGpuError(-2, "decode_windows_device_mix: a channel mask is not in 0..255")
        _check(self.lib.flacgpu_decode_windows_device_mix(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            sample_format, flags, len(masks), (ctypes.c_uint8 * max(len(masks), 1))(*masks), d_out, _u64s(out_offsets),
            _u64s(out_caps), d_results, _stream(stream)), "decode_windows_device_mix")

    def decode_windows_device_resample(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int,
                                       d_frame_bytes: int, d_index_results: int, d_frame_first_sample: int,
                                       d_stream_samples: int, windows: Sequence, sample_format: int, flags: int,
                                       channel_masks: Optional[Sequence[int]], src_rate: int, dst_rate: int, d_out: int,
                                       out_offsets: Sequence[int], out_caps: Sequence[int], d_results: int,
                                       stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device_resample: decode_windows_device_mix at another sample rate.
        The streams have src_rate; windows = [(stream, start, count)], offsets and caps are in output
        samples and elements at dst_rate.  channel_masks None: the context's channels as they are."""
        masks = None if channel_masks is None else [int(m) for m in channel_masks]
        if masks is not None and any(not 0 <= m <= 255 for m in masks):
            raise FlacGpuError(-2, "decode_windows_device_resample: a channel mask is not in 0..255")
        for name, r in (("src_rate", src_rate), ("dst_rate", dst_rate)):
            if not 0 <= int(r) <= 0xFFFFFFFF:
                raise FlacGpuError(-2, f"decode_windows_device_resample: {name} is not in 0..2^32-1")
        _check(self.lib.flacgpu_decode_windows_device_resample(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            sample_format, flags, len(masks) if masks is not None else 0,
            (ctypes.c_uint8 * max(len(masks), 1))(*masks) if masks is not None else None, int(src_rate), int(dst_rate), d_out,
            _u64s(out_offsets), _u64s(out_caps), d_results, _stream(stream)), "decode_windows_device_resample")

    def decode_windows_device_features(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int,
                                       d_frame_bytes: int, d_index_results: int, d_frame_first_sample: int,
                                       d_stream_samples: int, windows: Sequence, sample_format: int,
                                       channel_masks: Optional[Sequence[int]], src_rate: int, dst_rate: int, n_fft: int,
                                       hop: int, filters, d_out: int, out_offsets: Sequence[int], out_caps: Sequence[int],
                                       d_results: int, stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device_features: windows = [(stream, start, frames)], start in samples
        at the delivered rate; row r, frame t of channel k of window w at element
        out_offsets[w] + (k * rows + r) * frames + t of d_out.  filters: None (the n_fft / 2 + 1 bins) or
        float32 [rows, bins]; src_rate = dst_rate = 0: no rate change; channel_masks None: the
        context's channels as they are.  What the host can check raises ValueError before the call."""
        ft, f, _ = features_params(n_fft, hop, filters)
        masks = None if channel_masks is None else [int(m) for m in channel_masks]
        if masks is not None and (not 1 <= len(masks) <= 8 or any(not 0 <= m <= 255 for m in masks)):
            raise ValueError("decode_windows_device_features: 1 to 8 channel masks, each in 0..255")
        if sample_format not in (SAMPLE_F32, SAMPLE_F16, SAMPLE_BF16):
            raise ValueError("decode_windows_device_features: the format is SAMPLE_F32, SAMPLE_F16 or SAMPLE_BF16")
        if (src_rate or dst_rate) and resample_ratio(src_rate, dst_rate) is None:
            raise ValueError(f"decode_windows_device_features: {src_rate} -> {dst_rate} is not a ratio the filter serves")
        for _, start, frames in windows:
            if start < 0 or frames < 0 or (frames and (frames - 1) * ft.hop + ft.n_fft >= FEATURES_MAX_SPAN):
                raise ValueError("decode_windows_device_features: a window's start or frames is negative, or its span "
                                 "reaches 2^31")
        _check(self.lib.flacgpu_decode_windows_device_features(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            sample_format, len(masks) if masks is not None else 0,
            (ctypes.c_uint8 * max(len(masks), 1))(*masks) if masks is not None else None, int(src_rate), int(dst_rate),
            ctypes.byref(ft), f.ctypes.data if f is not None else None, d_out, _u64s(out_offsets), _u64s(out_caps), d_results,
            _stream(stream)), "decode_windows_device_features")

    def decode_windows_device_to(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int, d_frame_bytes: int,
                                 d_index_results: int, d_frame_first_sample: int, d_stream_samples: int,
                                 windows: Sequence, sample_format: int, flags: int, d_out: int,
                                 out_offsets: Sequence[int], out_caps: Sequence[int], d_results: int,
                                 channel_masks: Optional[Sequence[int]] = None, channel_weights=None, src_rate: int = 0,
                                 dst_rate: int = 0, n_fft: Optional[int] = None, hop: Optional[int] = None, filters=None,
                                 stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device_to: every window delivery through one call.  channel_masks (K
        masks) or channel_weights (K rows of C numbers: output channel k is the fused multiply-add
        chain of row k over the source channels), not both, or neither for the context's channels;
        src_rate and dst_rate as decode_windows_device_resample, 0 and 0 for no rate change; n_fft and
        hop (and filters) as decode_windows_device_features, windows then being [(stream, start,
        frames)] and flags 0.  Without channel_weights it is the existing call of those arguments."""
        masks = None if channel_masks is None else [int(m) for m in channel_masks]
        if masks is not None and (not 1 <= len(masks) <= 8 or any(not 0 <= m <= 255 for m in masks)):
            raise FlacGpuError(-2, "decode_windows_device_to: 1 to 8 channel masks, each in 0..255")
        w = None if channel_weights is None else _weights(channel_weights, "decode_windows_device_to")
        if w is not None and w.shape[1] != self.channels:  # the library reads K * C floats: it cannot see the rows' length
            raise FlacGpuError(-2, f"decode_windows_device_to: rows of {w.shape[1]} weights on a context of {self.channels} channels")
        for name, r in (("src_rate", src_rate), ("dst_rate", dst_rate)):
            if not 0 <= int(r) <= 0xFFFFFFFF:
                raise FlacGpuError(-2, f"decode_windows_device_to: {name} is not in 0..2^32-1")
        ft = f = None
        if n_fft is not None:
            ft, f, _ = features_params(n_fft, hop, filters)
        c_masks = (ctypes.c_uint8 * len(masks))(*masks) if masks is not None else None
        how = WindowDelivery(ctypes.sizeof(WindowDelivery), int(sample_format), int(flags),
                             len(masks) if masks is not None else (w.shape[0] if w is not None else 0),
                             ctypes.cast(c_masks, ctypes.c_void_p) if c_masks is not None else None,
                             w.ctypes.data if w is not None else None, int(src_rate), int(dst_rate),
                             ctypes.cast(ctypes.pointer(ft), ctypes.c_void_p) if ft is not None else None,
                             f.ctypes.data if f is not None else None)
        _check(self.lib.flacgpu_decode_windows_device_to(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            ctypes.byref(how), d_out, _u64s(out_offsets), _u64s(out_caps), d_results, _stream(stream)),
            "decode_windows_device_to")

    def decode_windows_device_fir(self, d_data: int, table_first: Sequence[int], d_frame_offsets: int, d_frame_bytes: int,
                                  d_index_results: int, d_frame_first_sample: int, d_stream_samples: int,
                                  windows: Sequence, sample_format: int, flags: int, d_taps: int, taps_len: int,
                                  filters: Sequence, window_filter: Sequence[int], d_out: int, out_offsets: Sequence[int],
                                  out_caps: Sequence[int], d_results: int, channel_masks: Optional[Sequence[int]] = None,
                                  channel_weights=None, src_rate: int = 0, dst_rate: int = 0,
                                  stream: Optional[int] = None) -> None:
        """flacgpu_decode_windows_device_fir: the windows of decode_windows_device_to (masks, weights
        and rates as there) convolved with a FIR filter each.  d_taps: taps_len float32 in device
        memory; filters = [(offset, taps, delay, rows)], rows 1 or the output channels, row r at float
        offset + r * taps of d_taps; window w goes through filters[window_filter[w]]: element t is the
        fused multiply-add chain over its taps k of x[start + t + delay - k]."""
        masks = None if channel_masks is None else [int(m) for m in channel_masks]
        if masks is not None and (not 1 <= len(masks) <= 8 or any(not 0 <= m <= 255 for m in masks)):
            raise FlacGpuError(-2, "decode_windows_device_fir: 1 to 8 channel masks, each in 0..255")
        w = None if channel_weights is None else _weights(channel_weights, "decode_windows_device_fir")
        if w is not None and w.shape[1] != self.channels:  # the library reads K * C floats: it cannot see the rows' length
            raise FlacGpuError(-2, f"decode_windows_device_fir: rows of {w.shape[1]} weights on a context of {self.channels} channels")
        for name, r in (("src_rate", src_rate), ("dst_rate", dst_rate)):
            if not 0 <= int(r) <= 0xFFFFFFFF:
                raise FlacGpuError(-2, f"decode_windows_device_fir: {name} is not in 0..2^32-1")
        if len(window_filter) != len(windows):
            raise FlacGpuError(-2, "decode_windows_device_fir: one filter index a window")
        for f in filters:
            if len(f) != 4 or any(not 0 <= int(v) <= 0xFFFFFFFF for v in f[1:]) or not 0 <= int(f[0]) < 1 << 64:
                raise FlacGpuError(-2, "decode_windows_device_fir: a filter is (offset, taps, delay, rows)")
        if any(not 0 <= int(i) <= 0xFFFFFFFF for i in window_filter):
            raise FlacGpuError(-2, "decode_windows_device_fir: a filter index is not in 0..2^32-1")
        c_filters = (Fir * max(len(filters), 1))(*[Fir(int(f[0]), int(f[1]), int(f[2]), int(f[3]), 0) for f in filters])
        c_masks = (ctypes.c_uint8 * len(masks))(*masks) if masks is not None else None
        how = WindowDelivery(ctypes.sizeof(WindowDelivery), int(sample_format), int(flags),
                             len(masks) if masks is not None else (w.shape[0] if w is not None else 0),
                             ctypes.cast(c_masks, ctypes.c_void_p) if c_masks is not None else None,
                             w.ctypes.data if w is not None else None, int(src_rate), int(dst_rate), None, None)
        _check(self.lib.flacgpu_decode_windows_device_fir(
            *self._window_args(d_data, table_first, d_frame_offsets, d_frame_bytes, d_index_results, d_frame_first_sample,
                               d_stream_samples, windows),
            ctypes.byref(how), d_taps, int(taps_len), len(filters), c_filters, _u32s([int(i) for i in window_filter]), d_out,
            _u64s(out_offsets), _u64s(out_caps), d_results, _stream(stream)), "decode_windows_device_fir")

    def decode_files_windows(self, flacs: Sequence[bytes], windows: Sequence, guard: int = 0,
                             pcm_caps: Optional[Sequence[int]] = None):
        """flacgpu_decode_files_windows: windows = [(file, start, count)] of whole FLAC files ->
        [(status, PCM bytes, guard bytes)] per window.  guard: that many extra bytes after every
        capacity, returned as the third member; pcm_caps: each window's capacity (default: count samples)."""
        n, nw = len(flacs), len(windows)
        per = self.channels * self.bytes_per_sample
        if pcm_caps is None:
            pcm_caps = [w[2] * per for w in windows]
        srcs = [ctypes.create_string_buffer(bytes(f), max(len(f), 1)) for f in flacs]
        outs = [ctypes.create_string_buffer(b"\xA5" * (c + guard + 1), c + guard + 1) for c in pcm_caps]
        P = ctypes.c_void_p
        a_src = (P * max(n, 1))(*[ctypes.addressof(b) for b in srcs])
        a_len = (ctypes.c_size_t * max(n, 1))(*[len(f) for f in flacs])
        a_out = (P * max(nw, 1))(*[ctypes.addressof(b) for b in outs])
        a_cap = (ctypes.c_size_t * max(nw, 1))(*pcm_caps)
        ns = (ctypes.c_uint64 * max(nw, 1))()
        st = (ctypes.c_int * max(nw, 1))()
        _check(self.lib.flacgpu_decode_files_windows(
            self.ctx, n, a_src, a_len, nw, _u32s([w[0] for w in windows]), _u64s([w[1] for w in windows]),
            _u64s([w[2] for w in windows]), a_out, a_cap, ns, st), "decode_files_windows")
        return [(int(st[w]), outs[w].raw[: min(ns[w] * per, pcm_caps[w])], outs[w].raw[pcm_caps[w]: pcm_caps[w] + guard])
                for w in range(nw)]

    def decode_files(self, flacs: Sequence[bytes], pcm_caps: Optional[Sequence[int]] = None, guard: int = 0):
        """flacgpu_decode_files: whole FLAC files in one call -> [(status, PCM bytes, md5_ok)] per
        file.  pcm_caps: each file's capacity (default: its frame count times the block size);
        guard: that many extra bytes after every capacity, returned as a fourth tuple member."""
        n = len(flacs)
        per = self.channels * self.bytes_per_sample
        if pcm_caps is None:
            pcm_caps = []
            for f in flacs:
                try:
                    pcm_caps.append(len(flac_index(f)[2]) * self.block_size * per)
                except FlacGpuError:
                    pcm_caps.append(0)
        srcs = [ctypes.create_string_buffer(bytes(f), max(len(f), 1)) for f in flacs]
        outs = [ctypes.create_string_buffer(b"\xA5" * (c + guard + 1), c + guard + 1) for c in pcm_caps]
        P = ctypes.c_void_p
        a_src = (P * max(n, 1))(*[ctypes.addressof(b) for b in srcs])
        a_out = (P * max(n, 1))(*[ctypes.addressof(b) for b in outs])
        a_len = (ctypes.c_size_t * max(n, 1))(*[len(f) for f in flacs])
        a_cap = (ctypes.c_size_t * max(n, 1))(*pcm_caps)
        ns = (ctypes.c_uint64 * max(n, 1))()
        ok = (ctypes.c_int * max(n, 1))()
        st = (ctypes.c_int * max(n, 1))()
        _check(self.lib.flacgpu_decode_files(self.ctx, n, a_src, a_len, a_out, a_cap, ns, ok, st), "decode_files")
        res = []
        for i in range(n):
            pcm = outs[i].raw[: min(ns[i] * per, pcm_caps[i])]
            item = (int(st[i]), pcm, bool(ok[i]))
            res.append(item + (outs[i].raw[pcm_caps[i]: pcm_caps[i] + guard],) if guard else item)
        return res

    def decode_frames(self, frames: bytes, sizes: Sequence[int]):
        """flacgpu_decode_frames: concatenated frames of one stream -> (PCM bytes, [DecodeResult])."""
        n = len(sizes)
        per = self.channels * self.bytes_per_sample
        cap = max(n * self.block_size * per, 1)
        out = ctypes.create_string_buffer(cap)
        fb = (ctypes.c_uint32 * max(n, 1))(*sizes)
        res = (DecodeResult * max(n, 1))()
        ns = ctypes.c_uint64(0)
        src = ctypes.create_string_buffer(bytes(frames), len(frames)) if frames else None
        _check(self.lib.flacgpu_decode_frames(self.ctx, src, fb, n, out, cap, ctypes.byref(ns), res), "decode_frames")
        return out.raw[: ns.value * per], list(res)[:n]

    def decode_file(self, flac: bytes):
        """flacgpu_decode_file: a whole FLAC file -> (PCM bytes, md5_ok)."""
        si, _, sizes = flac_index(flac)
        per = self.channels * self.bytes_per_sample
        cap = max(len(sizes) * self.block_size * per, 1)
        out = ctypes.create_string_buffer(cap)
        ns, ok = ctypes.c_uint64(0), ctypes.c_int(0)
        _check(self.lib.flacgpu_decode_file(self.ctx, bytes(flac), len(flac), out, cap, ctypes.byref(ns),
                                            ctypes.byref(ok)), "decode_file")
        return out.raw[: ns.value * per], bool(ok.value)

    def verify_plan_device(self, plan: "Plan", d_pcm: int, d_out: int, d_frame_offsets: int, d_frame_bytes: int,
                           d_results: int, d_bad_count: int, stream: Optional[int] = None) -> None:
        """flacgpu_verify_plan_device: decode the plan's encoded frames and compare them with d_pcm."""
        _check(self.lib.flacgpu_verify_plan_device(self.ctx, plan.handle, d_pcm, d_out, d_frame_offsets, d_frame_bytes,
                                                   d_results, d_bad_count, _stream(stream)), "verify_plan_device")


class Encoder(_DecodeOps):
    """GPU block encoder context == Encoder.init / deinit (encoder.zig:44-164)."""

    def __init__(self, channels: int, bits: int, sample_rate: int, device: int = 0, max_frames: int = 32768,
                 block_size: int = 4096, stereo_decorrelation: bool = True, max_rice_part_order: int = 8,
                 max_rice_param: int = 30, lpc_order: int = 0):
        self.lib = load_library()
        self.cfg = Config(sample_rate, block_size, channels, bits, 1 if stereo_decorrelation else 0,
                          max_rice_part_order, max_rice_param, lpc_order)
        self.channels, self.bits, self.sample_rate, self.block_size = channels, bits, sample_rate, block_size
        self.bytes_per_sample = bits // 8
        self.max_frames = max_frames
        h = ctypes.c_void_p()
        _check(self.lib.flacgpu_open(device, ctypes.byref(self.cfg), max_frames, ctypes.byref(h)), "open")
        self.ctx = h

    def close(self) -> None:
        if getattr(self, "ctx", None):
            self.lib.flacgpu_close(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- bounds
    def frame_bound(self) -> int:
        return self.lib.flacgpu_frame_bound_bytes(ctypes.byref(self.cfg))

    def reference_max_frame_bytes(self) -> int:
        return self.lib.flacgpu_reference_max_frame_bytes(ctypes.byref(self.cfg))

    # ---- encode
    def encode_frames(self, pcm: bytes, first_frame: int = 0):
        """Encode interleaved LE PCM -> (frame bytes, [per-frame sizes])."""
        per = self.channels * self.bytes_per_sample
        assert len(pcm) % per == 0
        n = len(pcm) // per
        nf = (n + self.block_size - 1) // self.block_size
        cap = nf * self.frame_bound() + 64
        out = ctypes.create_string_buffer(cap)
        sizes = (ctypes.c_uint32 * max(nf, 1))()
        out_len = ctypes.c_size_t(0)
        src = ctypes.create_string_buffer(bytes(pcm), len(pcm)) if pcm else None
        _check(self.lib.flacgpu_encode_frames(self.ctx, src, self.bytes_per_sample, n, first_frame, out, cap,
                                              ctypes.byref(out_len), sizes), "encode_frames")
        return out.raw[: out_len.value], list(sizes)[:nf]

    def encode_file(self, pcm: bytes) -> bytes:
        """Whole .flac file (73-byte header + frames) for interleaved LE PCM (wav2flac.zig:10-97)."""
        per = self.channels * self.bytes_per_sample
        n = len(pcm) // per
        nf = (n + self.block_size - 1) // self.block_size
        cap = 200 + nf * self.frame_bound()
        out = ctypes.create_string_buffer(cap)
        out_len = ctypes.c_size_t(0)
        src = ctypes.create_string_buffer(bytes(pcm), len(pcm)) if pcm else None
        _check(self.lib.flacgpu_encode_file(self.ctx, src, self.bytes_per_sample, n, out, cap, ctypes.byref(out_len)),
               "encode_file")
        return out.raw[: out_len.value]

    def encode_files(self, pcms: Sequence[bytes]) -> list:
        """flacgpu_encode_files: encode_file of every buffer, in one call (one pipelined schedule,
        the MD5s batched on the host pool)."""
        per = self.channels * self.bytes_per_sample
        n = len(pcms)
        ns = [len(p) // per for p in pcms]
        caps = [200 + ((k + self.block_size - 1) // self.block_size) * self.frame_bound() for k in ns]
        outs = [ctypes.create_string_buffer(c) for c in caps]
        srcs = [ctypes.create_string_buffer(bytes(p), len(p)) if p else None for p in pcms]
        src_p = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p).value if b is not None else None
                                                 for b in srcs])
        out_p = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p).value for b in outs])
        ns_a = (ctypes.c_uint64 * max(n, 1))(*ns)
        cap_a = (ctypes.c_size_t * max(n, 1))(*caps)
        len_a = (ctypes.c_size_t * max(n, 1))()
        _check(self.lib.flacgpu_encode_files(self.ctx, n, src_p, self.bytes_per_sample, ns_a, out_p, cap_a, len_a),
               "encode_files")
        return [outs[i].raw[: len_a[i]] for i in range(n)]

    def write_frame(self, planes, frame_number: int) -> bytes:
        """Encoder.writeFrame: planar int32 samples (C x n) -> one frame."""
        import numpy as np

        planes = np.ascontiguousarray(np.asarray(planes, dtype=np.int32))
        C, n = planes.shape
        assert C == self.channels
        ptrs = (ctypes.c_void_p * 8)()
        for c in range(C):
            ptrs[c] = planes[c].ctypes.data
        cap = self.frame_bound() + 64
        out = ctypes.create_string_buffer(cap)
        fb = ctypes.c_uint32(0)
        _check(self.lib.flacgpu_encode_frame_planar(self.ctx, ptrs, n, frame_number, out, cap, ctypes.byref(fb)),
               "encode_frame_planar")
        return out.raw[: fb.value]

    # ---- MD5 (md5.zig): the context's engine (host core by default, one GPU lane opt-in)
    def set_md5_engine(self, engine: int) -> None:
        _check(self.lib.flacgpu_md5_set_engine(self.ctx, engine), "md5_set_engine")

    def md5_engine(self) -> int:
        e = self.lib.flacgpu_md5_get_engine(self.ctx)
        if e < 0:
            raise FlacGpuError(e, "md5_get_engine")
        return e

    def md5(self, data: bytes) -> bytes:
        _check(self.lib.flacgpu_md5_init(self.ctx), "md5_init")
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        _check(self.lib.flacgpu_md5_update(self.ctx, buf, len(data)), "md5_update")
        d = ctypes.create_string_buffer(16)
        _check(self.lib.flacgpu_md5_final(self.ctx, d), "md5_final")
        return d.raw

    def md5_update(self, data: bytes) -> None:
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        _check(self.lib.flacgpu_md5_update(self.ctx, buf, len(data)), "md5_update")

    def md5_final(self) -> bytes:
        d = ctypes.create_string_buffer(16)
        _check(self.lib.flacgpu_md5_final(self.ctx, d), "md5_final")
        return d.raw

    # ---- device-resident batches
    def plan(self, offsets: Sequence[int], samples: Sequence[int], first_frames: Optional[Sequence[int]] = None,
             final: Optional[Sequence[bool]] = None) -> Plan:
        return Plan(self, offsets, samples, first_frames, final)

    def encode_plan_device_ex(self, plan: Plan, d_pcm: int, d_out: int, out_cap: int, d_frame_bytes: int,
                              d_frame_offsets: int, d_total: int, d_md5_state: Optional[int] = None,
                              d_md5: Optional[int] = None, stream: Optional[int] = None,
                              md5_stream: Optional[int] = None) -> None:
        """flacgpu_encode_plan_device_ex: MD5 state carried in d_md5_state (32 B per stream).
        md5_stream None: the MD5 is joined back into `stream`; any handle (0 = the legacy null
        stream) queues it there unjoined, as in encode_plan_device."""
        _check(self.lib.flacgpu_encode_plan_device_ex(
            self.ctx, plan.handle, d_pcm, d_out, out_cap, d_frame_bytes, d_frame_offsets, d_total,
            d_md5_state or None, d_md5 or None, _stream(stream), _stream(md5_stream)), "encode_plan_device_ex")

    def pcm_from_elements_device(self, d_src: Sequence[int], samples: Sequence[int], plane_stride: Optional[Sequence[int]],
                                 sample_format: int, flags: int, d_pcm: int, pcm_offsets: Sequence[int], pcm_cap: int,
                                 d_clipped: int, stream: Optional[int] = None) -> None:
        """flacgpu_pcm_from_elements_device: len(d_src) streams of elements (device addresses) to the
        interleaved PCM of this encoder's channels and depth at d_pcm + pcm_offsets[s]; d_clipped: a
        uint64 per stream in device memory.  Nothing synchronised."""
        n = len(d_src)
        _check(self.lib.flacgpu_pcm_from_elements_device(
            self.ctx, n, (ctypes.c_void_p * max(n, 1))(*d_src), _u64s(samples),
            _u64s(plane_stride) if plane_stride is not None else None, sample_format, flags, d_pcm, _u64s(pcm_offsets),
            pcm_cap, d_clipped, _stream(stream)), "pcm_from_elements_device")

    def sync_check(self, stream: Optional[int] = None) -> None:
        """Synchronise `stream` and raise if a kernel flagged a device-side error."""
        _check(self.lib.flacgpu_sync_check(self.ctx, _stream(stream)), "sync_check")

    def streaminfo_replay_device(self, d_frame_bytes: int, n_frames: int, d_minmax: int,
                                 stream: Optional[int] = None) -> None:
        """StreamInfo.updateFrameSize (metadata.zig:35-40) over device frame sizes; d_minmax = u32
        {min, max} in/out on the device ({0xFFFFFF, 0} for a new stream)."""
        _check(self.lib.flacgpu_streaminfo_replay_device(self.ctx, d_frame_bytes, n_frames, d_minmax,
                                                         _stream(stream)), "streaminfo_replay_device")

    def encode_frames_device(self, d_pcm: int, n_samples: int, first_frame: int = 0, stream: Optional[int] = None):
        """Frames of n_samples interleaved samples at device address d_pcm, numbered from first_frame, kept in
        device memory: returns (torch uint8 tensor of the bitstream, torch int32 tensor of frame sizes)."""
        import torch

        dev = torch.device("cuda", torch.cuda.current_device())
        plan = self.plan([0], [n_samples], first_frames=[first_frame])
        try:
            d_out = torch.empty(max(int(plan.out_bound), 1), dtype=torch.uint8, device=dev)
            d_fb = torch.empty(max(int(plan.n_frames), 1), dtype=torch.int32, device=dev)
            d_off = torch.empty(max(int(plan.n_frames), 1), dtype=torch.int64, device=dev)
            d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
            st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
            self.encode_plan_device_ex(plan, d_pcm, d_out.data_ptr(), int(plan.out_bound), d_fb.data_ptr(),
                                       d_off.data_ptr(), d_tot.data_ptr(), stream=st)
            self.sync_check(st)
            total = int(d_tot[0].item())
            return d_out[:total], d_fb[: int(plan.n_frames)]
        finally:
            plan.close()

    def encode_plan_device(self, plan: Plan, d_pcm: int, d_out: int, out_cap: int, d_frame_bytes: int,
                           d_frame_offsets: int, d_total: int, d_md5: Optional[int] = None,
                           stream: Optional[int] = None, md5_stream: Optional[int] = None) -> None:
        """md5_stream: queue the MD5 there without joining it back into `stream` (the caller
        synchronises it); None joins it (flacgpu_encode_plan_device).  As in encode_plan_device_ex,
        only None means "joined": a handle of 0 is the legacy null stream (_stream), like any
        other stream handle."""
        if md5_stream is not None:
            _check(self.lib.flacgpu_encode_plan_device_md5_async(
                self.ctx, plan.handle, d_pcm, d_out, out_cap, d_frame_bytes, d_frame_offsets, d_total,
                d_md5 or None, _stream(stream), _stream(md5_stream)), "encode_plan_device_md5_async")
            return
        _check(self.lib.flacgpu_encode_plan_device(self.ctx, plan.handle, d_pcm, d_out, out_cap, d_frame_bytes,
                                                   d_frame_offsets, d_total, d_md5 or None, _stream(stream)),
               "encode_plan_device")

    # ---- instrumentation
    def set_timing(self, on: bool) -> None:
        _check(self.lib.flacgpu_set_timing(self.ctx, 1 if on else 0), "set_timing")

    def reset_timing(self) -> None:
        _check(self.lib.flacgpu_reset_timing(self.ctx), "reset_timing")

    def kernel_time(self, k: int):
        n = ctypes.c_uint64(0)
        ms = ctypes.c_double(0)
        _check(self.lib.flacgpu_kernel_time(self.ctx, k, ctypes.byref(n), ctypes.byref(ms)), "kernel_time")
        return n.value, ms.value

    def set_overlap(self, ranges: int, ana_per_cu: int = 2, pack_per_cu: int = 2, min_frames: int = 4096) -> None:
        """Encode schedule (flacgpu_set_overlap): ranges > 1 overlaps the analysis of range i+1 with the
        scan + pack of range i on a second HIP stream; output bytes are unchanged."""
        _check(self.lib.flacgpu_set_overlap(self.ctx, ranges, ana_per_cu, pack_per_cu, min_frames), "set_overlap")

    def set_records(self, on: bool) -> None:
        _check(self.lib.flacgpu_set_records(self.ctx, 1 if on else 0), "set_records")

    def records(self) -> list:
        n = ctypes.c_uint64(0)
        _check(self.lib.flacgpu_get_records(self.ctx, None, 0, ctypes.byref(n)), "get_records")
        arr = (FrameRecord * max(n.value, 1))()
        _check(self.lib.flacgpu_get_records(self.ctx, arr, n.value, ctypes.byref(n)), "get_records")
        return list(arr)[: n.value]


DECODER_MAX_BLOCK = 16384  # FLACGPU_DECODER_MAX_BLOCK
DECODER_MAX_BLOCK_32 = 8192  # FLACGPU_DECODER_MAX_BLOCK_32: at 32 bits per sample


def decoder_max_block(bits: int) -> int:
    return DECODER_MAX_BLOCK_32 if bits == 32 else DECODER_MAX_BLOCK


class Decoder(Encoder):
    """A context used to decode: frames of `channels` x `bits` with blocks of at most block_size
    samples.  Up to 4096 it is the encoder's context (flacgpu_open); above, a decode-only one
    (flacgpu_open_decoder: up to decoder_max_block(bits) samples), on which every encode method raises
    FlacGpuError(-1).  There is no CPU fallback: without a device the constructor raises FlacGpuError(-5)."""

    def __init__(self, channels: int, bits: int, sample_rate: int, device: int = 0, max_frames: int = 4096,
                 block_size: int = 4096):
        if block_size <= 4096:
            super().__init__(channels, bits, sample_rate, device=device, max_frames=max_frames, block_size=block_size)
            return
        self.lib = load_library()
        self.cfg = Config(sample_rate, min(block_size, 0xFFFF), channels, bits, 0, 0, 0, 0)
        self.channels, self.bits, self.sample_rate, self.block_size = channels, bits, sample_rate, block_size
        self.bytes_per_sample = bits // 8
        self.max_frames = max_frames
        h = ctypes.c_void_p()
        _check(self.lib.flacgpu_open_decoder(device, sample_rate, channels, bits, block_size, max_frames, ctypes.byref(h)),
               "open_decoder")
        self.ctx = h


class MultiEncoder:
    """One input's frames sharded over several GPUs of this process (flacgpu_open_multi):
    contiguous frame ranges encoded concurrently, concatenated in frame order."""

    def __init__(self, devices: Sequence[int], channels: int, bits: int, sample_rate: int, max_frames: int = 32768,
                 block_size: int = 4096):
        self.lib = load_library()
        self.cfg = Config(sample_rate, block_size, channels, bits, 1, 8, 30, 0)
        self.channels, self.bytes_per_sample, self.block_size = channels, bits // 8, block_size
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        _check(self.lib.flacgpu_open_multi(len(devices), devs, ctypes.byref(self.cfg), max_frames, ctypes.byref(h)),
               "open_multi")
        self.m = h

    def close(self) -> None:
        if getattr(self, "m", None):
            self.lib.flacgpu_close_multi(self.m)
            self.m = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def encode_frames(self, pcm: bytes, first_frame: int = 0):
        per = self.channels * self.bytes_per_sample
        n = len(pcm) // per
        nf = (n + self.block_size - 1) // self.block_size
        cap = nf * self.lib.flacgpu_frame_bound_bytes(ctypes.byref(self.cfg)) + 64
        out = ctypes.create_string_buffer(cap)
        sizes = (ctypes.c_uint32 * max(nf, 1))()
        out_len = ctypes.c_size_t(0)
        src = ctypes.create_string_buffer(bytes(pcm), len(pcm)) if pcm else None
        _check(self.lib.flacgpu_multi_encode_frames(self.m, src, self.bytes_per_sample, n, first_frame, out, cap,
                                                    ctypes.byref(out_len), sizes), "multi_encode_frames")
        return out.raw[: out_len.value], list(sizes)[:nf]
