"""Inputs shared by the frame index's CPU test (test_index_host.py) and GPU test
(test_gpu_index.py): bare runs of frames, each with the stream bit depth / sample rate its headers
are read with.  The crafted ones assert their defining property here, in Python, before anybody
uses them: a drift in flac_bits then fails loudly instead of silently testing nothing."""
from __future__ import annotations

import functools
import os
import random

import numpy as np

import decode_cases as dc
import flac_bits as fb
import oracle_ref

VERBATIM = 0x02  # the one-byte subframe header: padding 0, type 000001, no wasted bits


def _header(number: int, bs: int) -> bytes:
    """The header fb.frame writes for a mono 16-bit frame (block size as an 8-bit field)."""
    fr = fb.frame(number, bs, 0, 16, lambda w: fb.sub_verbatim(w, [0] * bs, 16))
    n = 4 + len(fb.utf8_number(number)) + 1 + 1
    h = fr[:n]
    assert h[:2] == b"\xff\xf8" and fb.crc8(h[:-1]) == h[-1]
    return h


def _verbatim_frame(number: int, payload: bytes) -> bytes:
    """A mono 16-bit VERBATIM frame whose samples spell `payload` (even length, <= 512 bytes)."""
    assert len(payload) % 2 == 0 and 2 <= len(payload) <= 512
    x = [int.from_bytes(payload[i:i + 2], "big", signed=True) for i in range(0, len(payload), 2)]
    fr = fb.frame(number, len(x), 0, 16, lambda w: fb.sub_verbatim(w, x, 16))
    hdr = len(_header(number, len(x)))
    assert fr[hdr] == VERBATIM and fr[hdr + 1:hdr + 1 + len(payload)] == payload and len(fr) == hdr + 1 + len(payload) + 2
    assert fb.crc16(fr) == 0
    return fr


def _noise(n: int, seed) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def _small(number: int, seed) -> bytes:
    return _verbatim_frame(number, _noise(24, seed))


def lone_fake_header():
    fake = _header(77, 32)
    payload = _noise(30, "lone-a") + fake + _noise(40 - len(fake) % 2, "lone-b")
    payload += b"\0" * (len(payload) % 2)
    fr = _verbatim_frame(3, payload)
    at = fr.index(fake)
    assert fb.crc8(fr[at:at + len(fake) - 1]) == fr[at + len(fake) - 1]
    assert fb.crc16(fr[:at]) != 0  # no frame end there
    return _small(2, "lone-p") + fr + _small(4, "lone-s")


def nested_fake_frames():
    f1, f2 = _small(40, "nest-1"), _small(41, "nest-2")
    assert fb.crc16(f1) == 0 and fb.crc16(f2) == 0
    payload = _noise(10, "nest-a") + f1 + f2 + _noise(12, "nest-b")
    payload += b"\0" * (len(payload) % 2)
    fr = _verbatim_frame(9, payload)
    at = fr.index(f1)
    assert fr[at + len(f1):at + len(f1) + len(f2)] == f2
    assert fb.crc16(fr[:at]) != 0  # the inner frames match each other, not the stream start
    return _small(8, "nest-p") + fr + _small(10, "nest-s")


def false_end():
    number, fake = 21, _header(22, 16)
    prefix = _noise(20, "false-a")
    total = 20 + 2 + len(fake) + 31
    total += total % 2
    head = _header(number, total // 2) + bytes([VERBATIM]) + prefix  # the frame so far
    crc = fb.crc16(head).to_bytes(2, "big")
    payload = prefix + crc + fake + _noise(total - 22 - len(fake), "false-b")
    fr = _verbatim_frame(number, payload)
    cut = len(head) + 2
    assert fr[:len(head)] == head and fb.crc16(fr[:cut]) == 0 and fr[cut:cut + len(fake)] == fake
    return _small(20, "false-p") + fr + _small(23, "false-s"), len(_small(20, "false-p")) + cut


def _crc_tables():
    t16 = [fb.crc16(bytes([b])) for b in range(256)]
    t8 = [fb.crc8(bytes([b])) for b in range(256)]
    return t16, t8


@functools.lru_cache(maxsize=None)
def near_candidate():
    """A frame whose CRC-16 over the header, the subframe header byte and one sample byte is 0 (the
    frame number and that byte are found by search), followed at once by a clean header: a
    candidate hdr + 2 bytes after a frame start, closer than the hdr + 3 a frame's end must keep.
    (hdr + 1 cannot be had: a header with its CRC-8 has even parity, since z + 1 divides the CRC-8
    polynomial, the VERBATIM byte 0x02 makes it odd, and z + 1 divides the CRC-16 polynomial too.)"""
    fake = _header(5, 16)
    rest = fake + _noise(31 - len(fake) % 2, "near-b")
    assert len(rest) % 2 == 1
    bs = (1 + len(rest)) // 2
    t16, t8 = _crc_tables()
    found = None
    for number in range(1 << 16, 1 << 18):
        h = b"\xff\xf8\x69\x08" + fb.utf8_number(number) + bytes([bs - 1])
        c8 = 0
        for b in h:
            c8 = t8[c8 ^ b]
        c = 0
        for b in h + bytes([c8, VERBATIM]):
            c = ((c << 8) & 0xFFFF) ^ t16[(c >> 8) ^ b]
        if c & 0xFF == 0:  # then the byte c >> 8 brings the register to 0
            found = (number, c >> 8)
            break
    assert found is not None
    fr = _verbatim_frame(found[0], bytes([found[1]]) + rest)
    hdr = len(_header(found[0], bs))
    assert fb.crc16(fr[:hdr + 2]) == 0 and fr[hdr + 2:hdr + 2 + len(fake)] == fake
    return _small(1, "near-p") + fr + _small(2, "near-s"), hdr


@functools.lru_cache(maxsize=None)
def tiny_frames():
    """3001 frames of 11 to 13 bytes (mono 8-bit, block 16, CONSTANT); the frame numbers cross
    127 -> 128 and 2047 -> 2048, where the header grows by a byte."""
    out = []
    for i in range(3001):
        number = 100 + i
        out.append(fb.frame(number, 16, 0, 8, lambda w: fb.sub_constant(w, (number * 37) % 256 - 128, 8)))
    assert {len(f) for f in out} == {11, 12, 13} and fb.crc16(out[0]) == 0  # 1-, 2- and 3-byte frame numbers
    return out


@functools.lru_cache(maxsize=None)
def huge_frames():
    """8 channels x 32-bit noise, block 4096: VERBATIM frames of about 131 KB, three and a one-sample tail."""
    rng = np.random.default_rng(11)
    n = 3 * 4096 + 1
    pcm = rng.integers(-2 ** 31, 2 ** 31, size=n * 8, dtype=np.int64).astype(np.int32).tobytes()
    fr, sizes, _ = oracle_ref.encode_stream(pcm, 8, 32, 96000)
    assert len(sizes) == 4 and min(sizes[:3]) > 131000
    return fr, sizes


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, data, stream_bits, stream_rate)]: everything both tests run."""
    out = []
    for c in dc.FRAME_CASES:
        _, raw = dc.golden_frames(c)
        out.append((c["name"], raw, c["bits"], c["rate"]))
    c = dc.FILE_CASE
    buf = open(os.path.join(dc.GOLD, c["name"] + ".flac"), "rb").read()
    out.append((c["name"] + "@73", buf[73:], c["bits"], c["rate"]))
    hand = b"".join(h["frame"] for h in dc.hand_built() if h["channels"] == 1 and h["bits"] == 16)
    out.append(("hand_built", hand, 16, 44100))
    tiny = b"".join(tiny_frames())
    out.append(("tiny_frames", tiny, 8, 44100))
    out.append(("huge_frames", huge_frames()[0], 32, 96000))
    out.append(("lone_fake_header", lone_fake_header(), 16, 44100))
    out.append(("nested_fake_frames", nested_fake_frames(), 16, 44100))
    out.append(("false_end", false_end()[0], 16, 44100))
    out.append(("near_candidate", near_candidate()[0], 16, 44100))
    # refusals (whatever the host says, the device must say): a stream cut short, junk after the last
    # frame, no sync code at the start, and lengths below any frame's
    base = out[0][1]
    g = dc.FRAME_CASES[0]
    for k in (1, 2, 5):
        out.append((f"cut_{k}", base[:-k], g["bits"], g["rate"]))
    out.append(("trailing_junk", base + b"\x00\x11\x22", g["bits"], g["rate"]))
    out.append(("no_sync", b"\x7f" + base[1:], g["bits"], g["rate"]))
    for n in (0, 1, 5):
        out.append((f"len_{n}", base[:n], g["bits"], g["rate"]))
    return out


def host_index(data: bytes):
    """flacgpu_flac_index on a bare run of frames: the list of sizes, or None where it refuses."""
    import flacgpu

    try:
        return flacgpu.flac_index(data, raw_frames=True)[2]
    except flacgpu.FlacGpuError as e:
        assert e.code == -2
        return None
