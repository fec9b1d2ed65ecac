"""Inputs shared by the decoder's CPU tests (test_decode_host.py) and GPU tests
(test_gpu_decode.py): the golden streams split into frames, hand-built frames (flac_bits), the
corruptions, and the CPU verifier decoder's verdict on one frame."""
from __future__ import annotations

import ctypes
import json
import os
import random

import flac_bits as fb
import oracle_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))["cases"]
FRAME_CASES = [c for c in MANIFEST if c["kind"] == "frames"]
FILE_CASE = next(c for c in MANIFEST if c["kind"] == "file")

STATUS = {"OK": 0, "SYNC": 1, "HEADER": 2, "CRC8": 3, "SUBFRAME": 4, "CRC16": 5, "TRUNCATED": 6, "RANGE": 7, "MISMATCH": 8}


def golden_frames(c):
    """(list of frame bytes, stream bytes) of a `frames` golden."""
    raw = open(os.path.join(GOLD, c["name"] + ".flac"), "rb").read()
    out, pos = [], 0
    for n in c["frame_bytes"]:
        out.append(raw[pos:pos + n])
        pos += n
    assert pos == len(raw)
    return out, raw


def oracle_status(frame: bytes, channels: int, bits: int, rate: int, number: int) -> int:
    """Minus the code fdec_frames_to_pcm returns for this frame alone (0: it decodes)."""
    L = oracle_ref.lib()
    out = ctypes.create_string_buffer(65536 * channels * (bits // 8))
    sizes = (ctypes.c_uint32 * 4)()
    r = L.fdec_frames_to_pcm(frame, ctypes.c_size_t(len(frame)), channels, bits, rate, bits // 8, out,
                             ctypes.c_uint64(65535), ctypes.c_uint64(number), sizes, ctypes.c_uint64(4))
    return -r if r < 0 else 0


def oracle_pcm(frame: bytes, channels: int, bits: int, rate: int, number: int) -> bytes:
    pcm, _ = oracle_ref.decode_frames(frame, channels, bits, rate, 65535, first_number=number)
    return pcm


def flip(frame: bytes, bit: int) -> bytes:
    b = bytearray(frame)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def edge_flips(frame: bytes):
    """Every single-bit flip of the first 64 and the last 32 bits."""
    n = len(frame) * 8
    return sorted(set(list(range(min(64, n))) + list(range(max(0, n - 32), n))))


def random_flips(c, frames, count=200):
    """count seeded (frame index, bit) pairs over a golden's frames."""
    rng = random.Random("flips:" + c["name"])
    return [(f, rng.randrange(len(frames[f]) * 8)) for f in (rng.randrange(len(frames)) for _ in range(count))]


def cuts(frame: bytes):
    return [frame[:-1], frame[:-2], frame[:len(frame) // 2]]


# ---- hand-built frames: (name, channels, bits, number, frame bytes, marks) -------------------------
def _wave(n, amp, seed):
    import math
    rng = random.Random(seed)
    return [int(amp * math.sin(0.05 * i + seed) + rng.randrange(-3, 4)) for i in range(n)]


def interleave(planes, bits: int) -> bytes:
    """Channels of integer samples -> interleaved little-endian PCM of bits / 8 bytes a sample."""
    return b"".join((v & ((1 << bits) - 1)).to_bytes(bits // 8, "little") for row in zip(*planes) for v in row)


def hand_built():
    """Each with "pcm": the samples the frame was written from, known without any decoder."""
    out = []

    def add(name, ch, bits, number, bs, chc, writer, planes):
        marks = {}
        fr = fb.frame(number, bs, chc, bits, lambda w: writer(w, marks), marks)
        assert len(planes) == ch and all(len(p) == bs for p in planes)
        out.append({"name": name, "channels": ch, "bits": bits, "number": number, "block": bs, "frame": fr, "marks": marks,
                    "pcm": interleave(planes, bits)})

    # LPC order 32, precision 15
    x = _wave(192, 9000, 1)
    rng = random.Random(2)
    coefs = [rng.randrange(-900, 900) for _ in range(32)]
    coefs[0] = 16000
    add("lpc32_prec15", 1, 16, 5, 192, 0, lambda w, m: fb.sub_lpc(w, x, 16, coefs, 15, 14, 0, 1, [9, 10]), [x])
    # an escape partition of width 0 (all-zero residuals) beside a Rice one
    x2 = [7] * 64 + _wave(64, 500, 3)
    x2[64] = 7
    add("escape_width0", 1, 16, 6, 128, 0,
        lambda w, m: fb.sub_fixed(w, x2, 16, 1, 0, 1, [("esc", 0), 8]), [x2])
    # method 1 (5-bit parameters) with k = 20
    rng3 = random.Random(4)
    x3 = [rng3.randrange(-(1 << 22), 1 << 22) for _ in range(64)]
    add("method1_k20", 1, 24, 7, 64, 0, lambda w, m: fb.sub_fixed(w, x3, 24, 0, 1, 0, [20]), [x3])
    # FIXED order 4 in a 16-sample block, partition order 0
    x4 = _wave(16, 300, 5)
    add("fixed4_block16", 1, 16, 8, 16, 0, lambda w, m: fb.sub_fixed(w, x4, 16, 4, 0, 0, [4], m), [x4])
    # CONSTANT with wasted bits
    add("constant_waste", 1, 16, 9, 100, 0, lambda w, m: fb.sub_constant(w, -1024, 16, waste=3), [[-1024] * 100])
    # block 4096, partition order 8 (16-sample partitions, the first with 12 residuals), FIXED order 4
    x6 = _wave(4096, 12000, 6)
    add("fixed4_porder8", 1, 16, 10, 4096, 0,
        lambda w, m: fb.sub_fixed(w, x6, 16, 4, 0, 8, [5 + (p % 3) for p in range(256)]), [x6])
    # mid/side with odd side samples
    left = _wave(64, 1000, 7)
    right = [v + 2 * (i % 5) + 1 for i, v in enumerate(left)]  # left - right odd
    mid = [(a + b) >> 1 for a, b in zip(left, right)]
    side = [a - b for a, b in zip(left, right)]

    def ms(w, m):
        fb.sub_fixed(w, mid, 16, 2, 0, 0, [6])
        fb.sub_fixed(w, side, 17, 1, 0, 0, [3])

    add("midside_odd", 2, 16, 11, 64, 10, ms, [left, right])
    return out


def curated(frame: bytes, marks: dict):
    """The curated corruptions of a hand-built frame whose marks hold "low_bit" and pad_bits > 0:
    (name, corrupted frame, expected status name)."""
    hdr = marks["hdr_bytes"]
    n = len(frame)
    assert marks["pad_bits"] > 0 and "low_bit" in marks
    return [
        ("sync_byte", flip(frame, 3), "SYNC"),
        ("reserved_bit", flip(frame, 31), "HEADER"),
        ("crc8_byte", flip(frame, 8 * (hdr - 1) + 7), "CRC8"),
        ("number_bit", flip(frame, 8 * 4 + 7), "CRC8"),
        ("rice_low_bit", flip(frame, marks["low_bit"]), "CRC16"),
        ("crc16_byte", flip(frame, 8 * (n - 1) + 2), "CRC16"),
        ("padding_bit", flip(frame, marks["pad_pos"]), "SUBFRAME"),
    ]


def curated_base():
    """A hand-built frame with a Rice code of k > 0 and padding bits before its CRC-16."""
    c = next(h for h in hand_built() if h["name"] == "fixed4_block16")
    assert c["marks"]["pad_bits"] > 0
    return c
