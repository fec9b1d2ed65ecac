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


def sub_fixed(w, x, bps: int, order: int, method: int, porder: int, params, marks=None):
    sub_header(w, 8 + order, 0)
    for v in x[:order]:
        w.s(v, bps)
    residual(w, fixed_residual(x, order), len(x), order, method, porder, params, marks)


def lpc_residual(x, coefs, shift: int):
    o = len(coefs)
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(o, len(x))]


def sub_lpc(w, x, bps: int, coefs, prec: int, shift: int, method: int, porder: int, params):
    order = len(coefs)
    sub_header(w, 32 + order - 1, 0)
    for v in x[:order]:
        w.s(v, bps)
    w.u(prec - 1, 4)
    w.s(shift, 5)
    for c in coefs:
        w.s(c, prec)
    residual(w, lpc_residual(x, coefs, shift), len(x), order, method, porder, params)


def frame(number: int, bs: int, channel_assign: int, bits: int, write_subframes, marks=None) -> bytes:
    """9.1 + 9.3: header (44.1 kHz, fixed block size, block size as an 8- or 16-bit field),
    write_subframes(w), zero padding, CRC-16.  marks: "pad_bits", "pad_pos", "hdr_bytes"."""
    w = BitWriter()
    w.u(0x7FFC, 15)
    w.u(0, 1)
    w.u(6 if bs <= 256 else 7, 4)
    w.u(9, 4)
    w.u(channel_assign, 4)
    w.u(BITS_CODE[bits], 3)
    w.u(0, 1)
    for b in utf8_number(number):
        w.u(b, 8)
    w.u(bs - 1, 8 if bs <= 256 else 16)
    w.u(crc8(w.bytes()), 8)
    hdr = w.pos // 8
    write_subframes(w)
    pad_pos = w.pos
    pad = w.align()
    body = w.bytes()
    if marks is not None:
        marks.update(pad_bits=pad, pad_pos=pad_pos, hdr_bytes=hdr)
    return body + crc16(body).to_bytes(2, "big")
