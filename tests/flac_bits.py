"""A small FLAC frame writer for hand-built test frames, written from RFC 9639 (section 9: frame
header 9.1, subframes 9.2, coded residual 9.2.7, footer 9.3).  Test side only: it shares nothing
with the encoder, the CPU restatement or the decoder under test, and it can write layouts no
encoder here produces (LPC order 32, method-1 parameters, width-0 escapes)."""
from __future__ import annotations

BITS_CODE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


class BitWriter:
    def __init__(self):
        self.bits = []  # list of 0/1; frames are small

    def u(self, v: int, n: int):
        assert 0 <= v < (1 << n) if n else v == 0, (v, n)
        self.bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def s(self, v: int, n: int):
        assert -(1 << (n - 1)) <= v < (1 << (n - 1)), (v, n)
        self.u(v & ((1 << n) - 1), n)

    def unary(self, q: int):
        self.bits.extend([0] * q + [1])

    @property
    def pos(self) -> int:
        return len(self.bits)

    def align(self) -> int:
        pad = (-len(self.bits)) % 8
        self.bits.extend([0] * pad)
        return pad

    def bytes(self) -> bytes:
        assert len(self.bits) % 8 == 0
        return bytes(int("".join(map(str, self.bits[i:i + 8])), 2) for i in range(0, len(self.bits), 8))


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def utf8_number(v: int) -> bytes:
    """9.1.5: the UTF-8-like coded number, up to 36 bits in 7 bytes."""
    if v < 0x80:
        return bytes([v])
    for n, lead in ((2, 0xC0), (3, 0xE0), (4, 0xF0), (5, 0xF8), (6, 0xFC), (7, 0xFE)):
        if v < (1 << (5 * n + 1)) or n == 7:
            payload = 6 * (n - 1)
            first = lead | (v >> payload) if n < 7 else 0xFE
            return bytes([first] + [0x80 | ((v >> (6 * (n - 2 - i))) & 0x3F) for i in range(n - 1)])
    raise ValueError(v)


def zigzag(r: int) -> int:
    return (r << 1) if r >= 0 else ((-r - 1) << 1) | 1


def residual(w: BitWriter, res, bs: int, order: int, method: int, porder: int, params, marks=None):
    """9.2.7: res = the residuals of samples order..bs-1; params[p] = k, or ("esc", width).  marks
    (a dict) receives "low_bit": the position of the low binary bit of the first code with k > 0."""
    pbits, esc = (5, 31) if method else (4, 15)
    w.u(method, 2)
    w.u(porder, 4)
    psize = bs >> porder
    assert bs % (1 << porder) == 0 and psize >= order and len(params) == 1 << porder and len(res) == bs - order
    i = 0
    for p, par in enumerate(params):
        cnt = psize - (order if p == 0 else 0)
        if isinstance(par, tuple):
            w.u(esc, pbits)
            w.u(par[1], 5)
            for r in res[i:i + cnt]:
                if par[1]:
                    w.s(r, par[1])
                else:
                    assert r == 0
        else:
            assert par < esc
            w.u(par, pbits)
            for r in res[i:i + cnt]:
                u = zigzag(r)
                w.unary(u >> par)
                if par:
                    w.u(u & ((1 << par) - 1), par)
                    if marks is not None and "low_bit" not in marks:
                        marks["low_bit"] = w.pos - 1
        i += cnt


def sub_header(w: BitWriter, type_code: int, waste: int):
    w.u(0, 1)
    w.u(type_code, 6)
    if waste:
        w.u(1, 1)
        w.unary(waste - 1)
    else:
        w.u(0, 1)


def sub_constant(w, value: int, bps: int, waste: int = 0):
    sub_header(w, 0, waste)
    w.s(value >> waste, bps - waste)


def sub_verbatim(w, x, bps: int, waste: int = 0):
    sub_header(w, 1, waste)
    for v in x:
        w.s(v >> waste, bps - waste)


def fixed_residual(x, order: int):
    c = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}[order]
    return [x[i] - sum(cj * x[i - 1 - j] for j, cj in enumerate(c)) for i in range(order, len(x))]


def sub_fixed(w, x, bps: int, order: int, method: int, porder: int, params, marks=None, waste: int = 0):
    """9.2.5; waste: x holds multiples of 2^waste, coded as x >> waste at bps - waste bits."""
    sub_header(w, 8 + order, waste)
    x = [v >> waste for v in x]
    for v in x[:order]:
        w.s(v, bps - waste)
    residual(w, fixed_residual(x, order), len(x), order, method, porder, params, marks)


def lpc_residual(x, coefs, shift: int):
    o = len(coefs)
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(o, len(x))]


def sub_lpc(w, x, bps: int, coefs, prec: int, shift: int, method: int, porder: int, params, waste: int = 0):
    """9.2.6; waste as in sub_fixed."""
    order = len(coefs)
    sub_header(w, 32 + order - 1, waste)
    x = [v >> waste for v in x]
    for v in x[:order]:
        w.s(v, bps - waste)
    w.u(prec - 1, 4)
    w.s(shift, 5)
    for c in coefs:
        w.s(c, prec)
    residual(w, lpc_residual(x, coefs, shift), len(x), order, method, porder, params)


def block_size_code(bs: int) -> int:
    """9.1.1: the table code of a block size that has one (1: 192, 2..5: 576 * 2^n, 8..15:
    256 * 2^n), else 6 / 7 (the size follows the coded number as an 8- / 16-bit field)."""
    if bs == 192:
        return 1
    for n in range(4):
        if bs == 576 << n:
            return 2 + n
    for n in range(8):
        if bs == 256 << n:
            return 8 + n
    return 6 if bs <= 256 else 7


# 9.1.2: the sample rates of codes 1..11 (0: from STREAMINFO; 12: kHz in 8 bits, 13: Hz in 16 bits,
# 14: tens of Hz in 16 bits, each after the block-size field)
RATE_OF_CODE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
                11: 96000}


def frame(number: int, bs: int, channel_assign: int, bits: int, write_subframes, marks=None, *, table_bs: bool = False,
          rate_code: int = 9, rate_field: int = 0, bits_code=None, variable: bool = False) -> bytes:
    """9.1 + 9.3: header, write_subframes(w), zero padding, CRC-16.  By default 44.1 kHz, fixed
    block size, the block size as an 8- or 16-bit field.  table_bs: the block size's table code
    where it has one; rate_code 0..14, rate_field the value of the field codes 12..14 carry;
    bits_code: the bit-depth code (0: from STREAMINFO) instead of the one of `bits`; variable: the
    blocking-strategy bit set, `number` then being the frame's first sample number (36 bits).
    marks: "pad_bits", "pad_pos", "hdr_bytes"."""
    bsc = block_size_code(bs) if table_bs else (6 if bs <= 256 else 7)
    assert 0 <= rate_code <= 14 and 0 <= number < (1 << 36)
    w = BitWriter()
    w.u(0x7FFC, 15)
    w.u(1 if variable else 0, 1)
    w.u(bsc, 4)
    w.u(rate_code, 4)
    w.u(channel_assign, 4)
    w.u(BITS_CODE[bits] if bits_code is None else bits_code, 3)
    w.u(0, 1)
    for b in utf8_number(number):
        w.u(b, 8)
    if bsc in (6, 7):
        w.u(bs - 1, 8 if bsc == 6 else 16)
    if rate_code >= 12:
        w.u(rate_field, 8 if rate_code == 12 else 16)
    w.u(crc8(w.bytes()), 8)
    hdr = w.pos // 8
    write_subframes(w)
    pad_pos = w.pos
    pad = w.align()
    body = w.bytes()
    if marks is not None:
        marks.update(pad_bits=pad, pad_pos=pad_pos, hdr_bytes=hdr)
    return body + crc16(body).to_bytes(2, "big")
