"""Shared by test_cpu_jpeg_cases.py, test_gpu_jpeg_sweep.py and tools/jpeg_host_check.sh: a baseline JPEG
writer that starts from chosen quantised coefficients, and the named case table of the JPEG decode sweep
(csrc/jpeg.hip; DESIGN.md "JPEG decode sweep").  Pure numpy: no GPU, no Pillow.

Pillow's encoder only writes what a forward DCT of real pixels gives, with the Annex-K Huffman tables, 8-bit
tables, component ids 1, 2, 3 and one table per segment.  write_jpeg() takes the coefficients themselves, so a
case can put any run/size pattern, any amplitude the entropy coding can carry (DC differences of 11 bits, AC
values of 10), any Huffman table and any marker layout in front of the decoder.

The expectation of an accepted case is oracle/jpeg_oracle.py's decode of its bytes (libjpeg's C arithmetic,
jidctint.c / jdsample.c / jdcolor.c).  test_cpu_jpeg_cases.py pins that oracle, on every accepted case, to Pillow
with libjpeg-turbo's SIMD switched off (JSIMD_FORCENONE=1: the plain C path), and pins the tag of every case:
  tag "in"   the oracle also equals Pillow's default (SIMD) decode: coefficients a real encoder could produce
  tag "out"  Pillow's default decode differs: its SIMD IDCT works on 16-bit lanes and saturates where the C code
             keeps 32-bit intermediates and wraps the result through range_limit[x & 1023]
Tolerance: none; every comparison is array_equal.

MUTATIONS are arithmetic mistakes injected into a copy of the oracle's source (mutated_oracle); the CPU test
asserts that each one changes the expected output of at least one case, i.e. that the GPU comparison would catch
the same mistake in a kernel.

`python tests/jpeg_cases.py --dump DIR` writes every accepted case and damaged header as DIR/<name>.jpg for tools/jpeg_host_check.sh."""
from __future__ import annotations

import functools
import sys
import types
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
    21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
    61, 54, 47, 55, 62, 63], dtype=np.int64)

# ---------------------------------------------------------------------------------------------------------
# ITU T.81 Annex K.3 Huffman tables, as (counts of codes of length 1..16, symbols in code order)
_AC_LUMA = """
01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0
24 33 62 72 82 09 0a 16 17 18 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49
4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 83 84 85 86 87 88 89
8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5
c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8
f9 fa"""
_AC_CHROMA = """
00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0
15 62 72 d1 0a 16 24 34 e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48
49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79 7a 82 83 84 85 86 87
88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3
c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8
f9 fa"""
STD_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
STD_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
STD_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), tuple(int(x, 16) for x in _AC_LUMA.split()))
STD_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(int(x, 16) for x in _AC_CHROMA.split()))
STD_HUFF = {(0, 0): STD_DC_LUMA, (1, 0): STD_AC_LUMA, (0, 1): STD_DC_CHROMA, (1, 1): STD_AC_CHROMA}

# Annex K.1 / K.2 quantisation tables (natural order) for the cases that want a real encoder's steps
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)


def huff_codes(table) -> Dict[int, Tuple[int, int]]:
    """(counts, symbols) -> symbol -> (code, length), the canonical assignment of T.81 Annex C."""
    counts, syms = table
    assert len(counts) == 16 and sum(counts) == len(syms) and len(set(syms)) == len(syms)
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[syms[k]] = (code, length)
            code += 1
            k += 1
        assert code < (1 << length), "the all-ones code of a length is not assignable (libjpeg refuses the table)"
        code <<= 1
    return out


def long_code_table(used: Sequence[int], dummies: Sequence[int]):
    """A Huffman table in which every symbol of `used` sits on a code of 10 to 16 bits: nine `dummies` (symbols
    the case never emits) take one code of each length 1..9, so the 9-bit look-ahead of BitReader::sym resolves
    nothing the scan contains.  The used symbols go one to each length from 10 + skip to 15 and the rest to 16,
    with the smallest skip whose code space holds them."""
    used, dummies = list(used), list(dummies)
    assert len(dummies) >= 9 and not set(used) & set(dummies)
    for skip in range(7):
        counts = [1] * 9 + [0] * 7
        rest = len(used)
        for length in range(10 + skip, 16):
            if rest > 1:
                counts[length - 1] = 1
                rest -= 1
        counts[15] = rest
        table = (tuple(counts), tuple(dummies[:9] + used))
        try:
            huff_codes(table)
        except AssertionError:
            continue
        return table
    raise ValueError("too many symbols for a long-code table")


def _size(v: int) -> int:
    return int(abs(int(v))).bit_length()


def block_symbols(blk_zz: np.ndarray) -> List[Tuple[int, int, int]]:
    """AC part of one block in zigzag order -> [(run/size symbol, value bits, bit count)] per F.1.2.2."""
    out, run = [], 0
    nz = np.nonzero(blk_zz[1:])[0]
    last = int(nz[-1]) + 1 if len(nz) else 0
    for z in range(1, last + 1):
        v = int(blk_zz[z])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((0xF0, 0, 0))
            run -= 16
        s = _size(v)
        assert s <= 10, "baseline AC values have at most 10 bits"
        out.append(((run << 4) | s, v if v > 0 else v + (1 << s) - 1, s))
        run = 0
    if last < 63:
        out.append((0x00, 0, 0))
    return out


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0
        self.stuffed = 0
        self.lengths = {}          # Huffman code length -> how many such codes were written

    def put(self, v: int, n: int):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def code(self, cl):
        self.lengths[cl[1]] = self.lengths.get(cl[1], 0) + 1
        self.put(*cl)

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


@dataclass(frozen=True)
class Comp:
    id: int
    h: int
    v: int
    tq: int = 0
    td: int = 0
    ta: int = 0


def grid(width: int, height: int, comps: Sequence[Comp]) -> List[Tuple[int, int]]:
    """(blocks_y, blocks_x) of every component, padded to whole MCUs (one component: its own 8x8 raster)."""
    if len(comps) == 1:
        return [(-(-height // 8), -(-width // 8))]
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    return [(my * c.v, mx * c.h) for c in comps]


def encode_scan(comps: Sequence[Comp], coefs: Sequence[np.ndarray], huff, restart: int = 0):
    """Interleaved entropy-coded segment (RSTn markers included, byte-stuffed) and the writer's statistics."""
    codes = {k: huff_codes(v) for k, v in huff.items()}
    single = len(comps) == 1
    hv = [(1, 1) if single else (c.h, c.v) for c in comps]
    mx, my = coefs[0].shape[1] // hv[0][0], coefs[0].shape[0] // hv[0][1]
    w, pred, rst = _BitWriter(), [0] * len(comps), []
    for mcu in range(mx * my):
        if restart and mcu and mcu % restart == 0:
            w.align()
            m = 0xD0 + (mcu // restart - 1) % 8
            w.out += bytes([0xFF, m])
            rst.append(m)
            pred = [0] * len(comps)
        my0, mx0 = divmod(mcu, mx)
        for k, c in enumerate(comps):
            dc, ac = codes[(0, c.td)], codes[(1, c.ta)]
            for v in range(hv[k][1]):
                for h in range(hv[k][0]):
                    zz = coefs[k][my0 * hv[k][1] + v, mx0 * hv[k][0] + h][ZIGZAG]
                    d = int(zz[0]) - pred[k]
                    pred[k] = int(zz[0])
                    s = _size(d)
                    assert s <= 11 and abs(pred[k]) <= 2047, "baseline DC differences have at most 11 bits"
                    w.code(dc[s])
                    if s:
                        w.put(d if d > 0 else d + (1 << s) - 1, s)
                    for sym, bits, nb in block_symbols(zz):
                        w.code(ac[sym])
                        if nb:
                            w.put(bits, nb)
    w.align()
    return bytes(w.out), dict(stuffed=w.stuffed, lengths=dict(w.lengths), rst=rst)


def seg(marker: int, payload: bytes, fill: int = 0) -> bytes:
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dqt_payload(tid: int, table, bits16: bool = False) -> bytes:
    t = np.asarray(table, np.int64)[ZIGZAG]
    assert t.min() >= 1 and t.max() <= (65535 if bits16 else 255)
    return bytes([(16 if bits16 else 0) | tid]) + (t.astype(">u2").tobytes() if bits16 else t.astype("u1").tobytes())


def dht_payload(tc: int, th: int, table) -> bytes:
    return bytes([(tc << 4) | th]) + bytes(table[0]) + bytes(table[1])


def segments(data: bytes) -> List[Tuple[int, bytes, int]]:
    """(marker, payload, fill bytes in front of it) of every segment up to and including SOS."""
    out, i = [], 2
    while i < len(data):
        assert data[i] == 0xFF
        j = i + 1
        while data[j] == 0xFF:
            j += 1
        n = int.from_bytes(data[j + 1:j + 3], "big")
        out.append((data[j], data[j + 3:j + 1 + n], j - i - 1))
        if data[j] == 0xDA:
            break
        i = j + 1 + n
    return out


JFIF = seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def write_jpeg(width: int, height: int, comps: Sequence[Comp], coefs: Sequence[np.ndarray], qtables, huff=None,
               restart: int = 0, sof: int = 0xC0, precision: int = 8, merge_dqt: bool = False, merge_dht: bool = False,
               head: bytes = JFIF, before_sos: bytes = b"", fill: int = 0, omit: Sequence[str] = (),
               scan_comps: Optional[Sequence[int]] = None, check_grid: bool = True):
    """A single-scan interleaved sequential JPEG from quantised coefficients.

    comps       per component: id, sampling factors h x v, quantisation / DC / AC table selectors
    coefs       per component: int array [blocks_y, blocks_x, 64] in natural order, the grid of grid()
    qtables     {id: (table of 64 in natural order, 16-bit?)}
    huff        {(class, id): (counts, symbols)}; the Annex-K tables on ids 0 / 1 when None
    restart     restart interval in MCUs (DRI), 0 for none;  sof: 0xC0 (SOF0) or 0xC1 (SOF1)
    merge_dqt / merge_dht   all tables in one DQT / DHT segment (as ffmpeg writes), else a segment each
    head / before_sos       raw segments placed after SOI / before SOS;  fill: 0xFF fill bytes before every marker
    omit        any of "soi", "dqt", "dht", "sos" (the scan and EOI go with it), "eoi"
    scan_comps  the component indices the SOS names (all by default)
    Returns (bytes, stats of the entropy coder)."""
    huff = STD_HUFF if huff is None else huff
    if check_grid:
        assert [tuple(c.shape) for c in coefs] == [g + (64,) for g in grid(width, height, comps)]
    out = bytearray(b"" if "soi" in omit else b"\xff\xd8")
    out += head
    if "dqt" not in omit:
        parts = [dqt_payload(t, *qtables[t]) for t in sorted(qtables)]
        for p in ([b"".join(parts)] if merge_dqt else parts):
            out += seg(0xDB, p, fill)
    sofp = bytes([precision]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([len(comps)])
    for c in comps:
        sofp += bytes([c.id, (c.h << 4) | c.v, c.tq])
    out += seg(sof, sofp, fill)
    if "dht" not in omit:
        parts = [dht_payload(tc, th, huff[(tc, th)]) for (tc, th) in sorted(huff)]
        for p in ([b"".join(parts)] if merge_dht else parts):
            out += seg(0xC4, p, fill)
    if restart:
        out += seg(0xDD, restart.to_bytes(2, "big"), fill)
    out += before_sos
    stats = {}
    if "sos" not in omit:
        idx = list(range(len(comps))) if scan_comps is None else list(scan_comps)
        sosp = bytes([len(idx)])
        for k in idx:
            sosp += bytes([comps[k].id, (comps[k].td << 4) | comps[k].ta])
        out += seg(0xDA, sosp + b"\x00\x3f\x00", fill)
        scan, stats = encode_scan([comps[k] for k in idx], [coefs[k] for k in idx], huff, restart)
        out += scan
    if "eoi" not in omit:
        out += b"\xff" * fill + b"\xff\xd9"
    return bytes(out), stats


# ---------------------------------------------------------------------------------------------------------
# the case table
@dataclass
class Case:
    name: str
    data: bytes
    tag: Optional[str] = None          # "in" / "out" for accepted cases
    refuse: Optional[str] = None       # "ARG" / "UNSUPPORTED" for refused ones
    stats: dict = field(default_factory=dict)
    batch: Optional[str] = None        # cases of one batch key share size and sampling and go out in one call
    narrow: bool = False               # refused only for its narrow chroma: Pillow decodes it
    meta: dict = field(default_factory=dict)   # what the builder asked of the writer (size, sampling, ids, DRI ..)


S444 = ((1, 1), (1, 1), (1, 1))
S422 = ((2, 1), (1, 1), (1, 1))
S420 = ((2, 2), (1, 1), (1, 1))
S_CR22 = ((2, 2), (1, 1), (2, 2))      # Y 2x2, Cb 1x1, Cr 2x2
S_CR21 = ((2, 1), (1, 1), (2, 1))      # Y 2x1, Cb 1x1, Cr 2x1


def components(sampling, ids=(1, 2, 3), tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1)) -> List[Comp]:
    return [Comp(ids[k], hv[0], hv[1], tq[k], td[k], ta[k]) for k, hv in enumerate(sampling)]


GREY = [Comp(1, 1, 1, 0, 0, 0)]


def natural(g, shape, dc=40, ac=12.0):
    """Coefficients shaped like an encoder's: a DC walk inside +-dc, AC magnitudes falling off along the zigzag."""
    by, bx = shape
    c = np.zeros((by, bx, 64), np.int64)
    amp = ac / (1.0 + np.arange(64)) ** 1.1
    zz = np.rint(g.normal(0, 1, (by, bx, 64)) * amp).astype(np.int64)
    zz[:, :, 0] = g.integers(-dc, dc + 1, (by, bx))
    c[:, :, ZIGZAG] = zz
    return c


def _flat(width, height, comps, dc=0):
    cs = [np.zeros(g + (64,), np.int64) for g in grid(width, height, comps)]
    for c in cs:
        c[:, :, 0] = dc
    return cs


def _q(v=1, bits16=False):
    return (np.full(64, v, np.int64), bits16)


QSTD = {0: (Q_LUMA, False), 1: (Q_CHROMA, False)}
Q1 = {0: _q(1), 1: _q(1)}


def _build() -> List[Case]:
    cases: List[Case] = []

    def add(name, tag, width, height, comps, coefs, qtables, refuse=None, batch=None, narrow=False, **kw):
        data, stats = write_jpeg(width, height, comps, coefs, qtables, **kw)
        meta = dict(width=width, height=height, hv=[(c.h, c.v) for c in comps], ids=[c.id for c in comps],
                    tables=[(c.tq, c.td, c.ta) for c in comps], restart=kw.get("restart", 0), sof=kw.get("sof", 0xC0))
        cases.append(Case(name, data, tag, refuse, stats, batch, narrow, meta))
        return cases[-1]

    def rng(name):
        return np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 63))

    # ---- amplitude, in range
    # one coefficient per block, every one of the 64 positions, in each component (positions rotated per plane)
    comps = components(S444)
    cs = _flat(64, 64, comps)
    for k, c in enumerate(cs):
        for p in range(64):
            pos = (p * (2 * k + 1) + 5 * k) % 64
            c[p // 8, p % 8, pos] = (-1) ** (p + k) * (90 + 3 * p) if pos else 60 - 2 * p
    add("amp_single_coefficient_each_position", "in", 64, 64, comps, cs, {0: _q(2), 1: _q(3)})
    for nm, (w, h), samp in [("amp_dense_444_40x24", (40, 24), S444), ("amp_dense_420_48x40", (48, 40), S420)]:
        comps, g = components(samp), rng(nm)
        cs = [natural(g, s) for s in grid(w, h, comps)]
        add(nm, "in", w, h, comps, cs, QSTD)
    # every quantiser 1 and coefficients at the size a quality-100 encode of noise reaches
    comps, g = components(S444), rng("amp_dense_q1")
    add("amp_dense_q1_full_scale_32x16", "in", 32, 16, comps, [natural(g, s, 900, 260.0) for s in grid(32, 16, comps)], Q1)

    # ---- amplitude, out of range
    # DC differences of +-2047 (11 bits): the prediction walks 0, 2047, 0, -2047, 0 .. and a restart in the middle
    # puts it back to 0 from +-2047; quantiser 8 takes the sample to +-2047 + 128: the range table wraps
    comps = components(S444)
    cs = _flat(48, 16, comps)
    walk = np.array([2047, 0, -2047, 0, 2047, -2047, 0, 2047, 2047, 0, -2047, -2047])   # restarts before 5 and 10
    for k, c in enumerate(cs):
        c[:, :, 0] = ((-1) ** k * walk).reshape(2, 6)
    add("amp_dc_chain_2047_restart", "out", 48, 16, comps, cs, {0: _q(3), 1: _q(3)}, restart=5)
    # AC +-1023 (10 bits) under quantisers up to 255
    comps, g = components(S420), rng("amp_ac_1023_q255")
    cs = _flat(32, 16, comps)
    for c in cs:
        for b in c.reshape(-1, 64):
            pos = g.choice(np.arange(1, 64), 5, replace=False)
            b[pos] = g.choice([-1023, 1023], 5)
            b[0] = g.integers(-300, 300)
    qa = np.concatenate([[16], g.integers(1, 256, 63)])
    qa[[1, 8, 63]] = 255
    add("amp_ac_1023_q255", "out", 32, 16, comps, cs, {0: (qa, False), 1: (qa[::-1].copy(), False)})
    # the same with 16-bit tables: entries above 255 (300 .. 4000)
    q16 = np.concatenate([[8], g.integers(300, 4001, 63)])
    add("amp_ac_1023_q16bit", "out", 32, 16, comps, cs, {0: (q16, True), 1: (q16[::-1].copy(), True)})
    # 16-bit entries of 32768 and more: libjpeg-turbo holds the multiplier as a signed short, so 40000 acts as
    # -25536 and 65535 as -1 (the decoder used to multiply by the unsigned entry; this case found it)
    qneg = np.concatenate([[8], g.choice([32768, 40000, 65535], 63)])
    csn = _flat(32, 16, comps)
    for c in csn:
        for b in c.reshape(-1, 64):
            b[g.choice(np.arange(1, 64), 4, replace=False)] = g.integers(-3, 4, 4)
            b[0] = g.integers(-100, 100)
    add("amp_q16bit_entry_above_32767", "out", 32, 16, comps, csn, {0: (qneg, True), 1: (qneg[::-1].copy(), True)})
    # every position at its largest value: DC +-2047, all 63 ACs +-1023, quantiser 255 everywhere
    comps = components(S444)
    cs = _flat(24, 8, comps)
    for k, c in enumerate(cs):
        for j, b in enumerate(c.reshape(-1, 64)):
            sgn = np.where((np.arange(64) * (j + 2 * k + 1)) % 3 == 0, -1, 1) if j else 1
            b[:] = 1023 * sgn
            b[0] = (-1) ** k * [2047, 0, -2047][j % 3]
    add("amp_all_positions_maximal", "out", 24, 8, comps, cs, {0: _q(255), 1: _q(255)})
    # provably wrapping: one DC-only block per value, sample = dc + 128 for quantiser 8: 700 + 128 = 828 -> the
    # table gives 0 (828 & 1023 in 512..895), a clamp 255; -900 + 128 -> 252 (wrapped), a clamp 0
    comps = GREY
    cs = _flat(32, 8, comps)
    cs[0][0, :, 0] = [700, -900, 100, -100]
    add("amp_range_wrap_grey", "out", 32, 8, comps, cs, {0: _q(8)})

    # ---- run/size
    comps, g = components(S444), rng("runsize")
    cs = _flat(32, 8, comps, 10)
    for c in cs:
        c[0, 0, ZIGZAG[63]] = 37                               # run 62 = ZRL x3 + (14, s) landing on 63
        c[0, 1, ZIGZAG[1:]] = g.choice([-3, -2, -1, 1, 2, 5], 63)   # 63 nonzero ACs: no EOB
        # block 2: EOB straight after DC (left as it is)
        c[0, 3, ZIGZAG[47]] = -9                               # (15, s) from position 47 lands on 63 by r alone
        c[0, 3, ZIGZAG[63]] = 4
    add("runsize_zrl3_full_eob_r15", "in", 32, 8, comps, cs, Q1)

    # ---- entropy coding
    # long codes: every DC size and AC run/size the scan uses sits on a 10- to 16-bit code
    comps, g = components(S420, td=(0, 1, 1), ta=(0, 1, 1)), rng("huff_long")
    cs = [natural(g, s, 20, 12.0) for s in grid(32, 24, comps)]
    cs[0][0, 0, ZIGZAG[63]] = 3
    huff_long = _long_tables(comps, cs)
    add("huff_long_codes", "in", 32, 24, comps, cs, QSTD, huff=huff_long)
    # table ids 2 and 3 under SOF1 (extended sequential, Huffman): the Annex-K tables on the upper ids
    comps = components(S422, tq=(2, 3, 3), td=(2, 3, 3), ta=(3, 2, 2))
    cs = [natural(g, s) for s in grid(24, 16, comps)]
    huff23 = {(0, 2): STD_DC_LUMA, (1, 3): STD_AC_LUMA, (0, 3): STD_DC_CHROMA, (1, 2): STD_AC_CHROMA}
    add("huff_ids_2_3_sof1", "in", 24, 16, comps, cs, {2: (Q_LUMA, False), 3: (Q_CHROMA, False)}, huff=huff23, sof=0xC1)
    # many stuffed bytes: values whose bits are all ones (255 = 8 ones, -1 = "0", 127, 63) behind all-ones-heavy codes
    comps = components(S444)
    cs = _flat(32, 16, comps, 0)
    for k, c in enumerate(cs):
        c[:, :, ZIGZAG[1:3]] = 255
        c[:, :, ZIGZAG[3:30]] = np.array([63, 31, 15] * 9)
        c[:, :, 0] = (np.arange(8).reshape(2, 4) % 2) * 255
    add("huff_stuffed_ff00", "in", 32, 16, comps, cs, {0: _q(1), 1: _q(1)})

    # ---- structure
    comps, g = components(S420), rng("structure")
    base = [natural(g, s) for s in grid(32, 24, comps)]
    add("struct_merged_dht_dqt", "in", 32, 24, comps, base, QSTD, merge_dqt=True, merge_dht=True, batch="b420")
    q16s = {0: (Q_LUMA * 3, True), 1: (Q_CHROMA, False)}
    add("struct_dqt_16bit", "in", 32, 24, comps, [natural(g, s, 20, 12.0) for s in grid(32, 24, comps)], q16s, batch="b420")
    add("struct_ids_0_1_2", "in", 32, 24, components(S420, ids=(0, 1, 2)), [natural(g, s) for s in grid(32, 24, comps)],
        {0: (Q_LUMA // 2 + 1, False), 1: (Q_CHROMA // 3 + 1, False)}, batch="b420")
    add("struct_ids_7_9_200_no_jfif", "in", 32, 24, components(S420, ids=(7, 9, 200)),
        [natural(g, s) for s in grid(32, 24, comps)], QSTD, head=b"", batch="b420")
    add("struct_fill_bytes", "in", 32, 24, comps, base, QSTD, fill=3)
    nested = b"\xff\xd8\xff\xdb\x00\x43\x00 thumbnail \xff\xda\x00\x0c\x03\x01\x00 \xff\xd9"
    add("struct_com_app1_with_soi_eoi", "in", 32, 24, comps, base, QSTD,
        head=JFIF + seg(0xFE, b"comment " + nested) + seg(0xE1, b"Meta\x00" + nested), before_sos=seg(0xFE, nested))
    add("struct_dri_1", "in", 32, 24, comps, [natural(g, s) for s in grid(32, 24, comps)], QSTD, restart=1, batch="b420")
    c11 = components(S444)
    add("struct_dri_11_intervals", "in", 48, 32, c11, [natural(g, s) for s in grid(48, 32, c11)], QSTD, restart=2)
    add("struct_dri_beyond_mcu_count", "in", 32, 24, comps, base, QSTD, restart=1000)
    cs = [natural(g, s, 20, 12.0) for s in grid(32, 24, comps)]
    add("struct_long_codes_dri_3", "in", 32, 24, comps, cs, QSTD, huff=_long_tables(comps, cs), restart=3, batch="b420")

    # ---- sampling
    for nm, (w, h), samp in [("samp_444_19x13", (19, 13), S444), ("samp_422_35x21", (35, 21), S422),
                             ("samp_420_37x27", (37, 27), S420), ("samp_cb11_cr22_29x19", (29, 19), S_CR22),
                             ("samp_cb11_cr21_27x11", (27, 11), S_CR21), ("samp_420_w5_h9", (5, 9), S420),
                             ("samp_420_w6_h2", (6, 2), S420), ("samp_422_w5_h17", (5, 17), S422),
                             ("samp_422_w6_h1", (6, 1), S422), ("samp_420_w21_h1", (21, 1), S420),
                             ("samp_420_w40_h17", (40, 17), S420), ("samp_444_w1_h9", (1, 9), S444),
                             ("samp_444_w9_h2", (9, 2), S444)]:
        comps, g = components(samp), rng(nm)
        add(nm, "in", w, h, comps, [natural(g, s) for s in grid(w, h, comps)], QSTD)
    for nm, (w, h) in [("samp_grey_24x16_a", (24, 16)), ("samp_grey_24x16_b", (24, 16)), ("samp_grey_24x16_dri", (24, 16)),
                       ("samp_grey_13x17", (13, 17))]:
        g = rng(nm)
        add(nm, "in", w, h, GREY, [natural(g, s) for s in grid(w, h, GREY)],
            {0: (Q_LUMA if nm.endswith("a") else Q_LUMA // 2 + 1, False)}, restart=2 if nm.endswith("dri") else 0,
            batch="bgrey" if "24x16" in nm else None)
    # 64x64 4:2:0: the largest image of the table (the staging-buffer sequence decodes 16 of them)
    comps, g = components(S420), rng("samp_420_64x64")
    for k, nm in enumerate(["samp_420_64x64", "samp_420_64x64_b", "samp_420_64x64_c", "samp_420_64x64_d"]):
        add(nm, "in", 64, 64, comps, [natural(g, s) for s in grid(64, 64, comps)],
            {0: (Q_LUMA // (k + 1) + 1, False), 1: (Q_CHROMA // (k + 1) + 1, False)}, restart=3 * k, batch="b64")
    add("samp_grey_8x8", "in", 8, 8, GREY, [natural(g, s) for s in grid(8, 8, GREY)], {0: (Q_LUMA, False)})

    # ---- refusals
    def refuse(name, code, width, height, comps, narrow=False, **kw):
        g = rng(name)
        cs = kw.pop("coefs", None) or [natural(g, s, 20, 12.0) for s in grid(width, height, comps)]
        add(name, None, width, height, comps, cs, kw.pop("qtables", QSTD), refuse=code, narrow=narrow, **kw)

    refuse("refuse_440", "UNSUPPORTED", 16, 16, components(((1, 2), (1, 1), (1, 1))))
    refuse("refuse_luma_not_largest", "UNSUPPORTED", 16, 16, components(((1, 1), (2, 2), (2, 2))))
    refuse("refuse_sampling_factor_4", "UNSUPPORTED", 32, 8, components(((4, 1), (1, 1), (1, 1))))
    c4 = [Comp(1, 1, 1, 0, 0, 0), Comp(2, 1, 1, 1, 1, 1), Comp(3, 1, 1, 1, 1, 1), Comp(4, 1, 1, 0, 0, 0)]
    refuse("refuse_4_components", "UNSUPPORTED", 16, 8, c4)
    # non-interleaved: three scans of one component each (only the first is written in full; the refusal is at its SOS)
    c3 = components(S444)
    g = rng("refuse_multi_scan")
    cs = [natural(g, s, 20, 12.0) for s in grid(16, 8, c3)]
    first, _ = write_jpeg(16, 8, c3, cs, QSTD, scan_comps=[0], omit=("eoi",))
    rest = b""
    for k in (1, 2):
        scan, _ = encode_scan([c3[k]], [cs[k]], STD_HUFF)
        rest += seg(0xDA, bytes([1, c3[k].id, (c3[k].td << 4) | c3[k].ta]) + b"\x00\x3f\x00") + scan
    cases.append(Case("refuse_non_interleaved_scans", first + rest + b"\xff\xd9", None, "UNSUPPORTED"))
    refuse("refuse_12_bit", "UNSUPPORTED", 16, 8, components(S444), sof=0xC1, precision=12)
    refuse("refuse_missing_dht", "UNSUPPORTED", 16, 8, components(S444), omit=("dht",))
    refuse("refuse_missing_dqt", "UNSUPPORTED", 16, 8, components(S444), omit=("dqt",))
    refuse("refuse_narrow_420_w4_h16", "UNSUPPORTED", 4, 16, components(S420), narrow=True)
    refuse("refuse_narrow_422_w3_h16", "UNSUPPORTED", 3, 16, components(S422), narrow=True)
    refuse("refuse_rgb_ids_no_jfif", "UNSUPPORTED", 16, 8, components(S444, ids=(ord("R"), ord("G"), ord("B"))), head=b"")
    refuse("refuse_no_soi", "ARG", 16, 8, components(S444), omit=("soi",))
    refuse("refuse_no_scan", "ARG", 16, 8, components(S444), omit=("sos",))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def _long_tables(comps, coefs):
    """Long-code tables for exactly the symbols this scan emits, luma on ids 0, chroma on ids 1."""
    used = {(0, 0): set(), (1, 0): set(), (0, 1): set(), (1, 1): set()}
    hmax, vmax = max(c.h for c in comps), max(c.v for c in comps)
    mx, my = coefs[0].shape[1] // hmax, coefs[0].shape[0] // vmax
    for k, c in enumerate(comps):
        pred = 0
        for mcu in range(mx * my):                       # no restart: a restart only adds the sizes of the values
            my0, mx0 = divmod(mcu, mx)
            for v in range(c.v):
                for h in range(c.h):
                    zz = coefs[k][my0 * c.v + v, mx0 * c.h + h][ZIGZAG]
                    used[(0, c.td)] |= {_size(int(zz[0]) - pred), _size(int(zz[0]))}
                    pred = int(zz[0])
                    used[(1, c.ta)] |= {s for s, _, _ in block_symbols(zz)}
    out = {}
    for (tc, th), u in used.items():
        pool = [s for s in (range(16) if tc == 0 else [0x0B, 0x0C, 0x0D, 0x0E, 0x0F, 0x1B, 0x1C, 0x1D, 0x1E, 0x1F])
                if s not in u]
        out[(tc, th)] = long_code_table(sorted(u), pool)
    return out


@functools.lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    return tuple(_build())


def accepted() -> List[Case]:
    return [c for c in cases() if c.refuse is None]


def refused() -> List[Case]:
    return [c for c in cases() if c.refuse is not None]


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def batch(key: str) -> List[Case]:
    return [c for c in cases() if c.batch == key]


_EXPECTED: Dict[str, np.ndarray] = {}


def expected(c: Case) -> np.ndarray:
    """The oracle's decode of an accepted case, computed once per process and handed out read-only."""
    if c.name not in _EXPECTED:
        from oracle import jpeg_oracle as J
        a = J.decode(c.data)
        a.setflags(write=False)
        _EXPECTED[c.name] = a
    return _EXPECTED[c.name]


# ---------------------------------------------------------------------------------------------------------
# arithmetic mistakes, as edits of the oracle's source: name -> [(text, replacement)], each text occurring once
MUTATIONS = {
    "h2v2 odd-column bias 7 -> 8": [("odd = (3 * cs + nxt + 7) >> 4", "odd = (3 * cs + nxt + 8) >> 4")],
    "h2v1 odd-column bias 2 -> 1": [("odd = (3 * p + right + 2) >> 2", "odd = (3 * p + right + 1) >> 2")],
    # an interior column reads its real neighbour: column -1 / dw is another sample, not the replicated edge
    "h2v1 first column as interior": [("left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)", "left = np.roll(p, 1, axis=1)"),
                                      ("        even[:, 0] = p[:, 0]\n", "")],
    "h2v1 last column as interior": [("right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)", "right = np.roll(p, -1, axis=1)"),
                                     ("        odd[:, -1] = p[:, -1]\n", "")],
    "h2v2 first column as interior": [("last = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)", "last = np.roll(cs, 1, axis=1)"),
                                      ("            even[:, 0] = (4 * cs[:, 0] + 8) >> 4\n", "")],
    "h2v2 last column as interior": [("nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)", "nxt = np.roll(cs, -1, axis=1)"),
                                     ("            odd[:, -1] = (4 * cs[:, -1] + 7) >> 4\n", "")],
    "h2v2 bottom context row not replicated": [("dn = np.concatenate([p[1:], p[-1:]], axis=0)",
                                                "dn = np.concatenate([p[1:], 0 * p[-1:]], axis=0)")],
    "range wrap -> clamp": [("    y = v & 1023\n", "    return np.clip(v + 128, 0, 255).astype(np.uint8)\n    y = v & 1023\n")],
    "pass-1 descale without rounding": [("ws = np.stack([_descale(o, CB - P1) for o in cols], axis=1)",
                                         "ws = np.stack([o >> (CB - P1) for o in cols], axis=1)")],
    "IDCT constant FIX_0_541196100 + 1": [("= 2446, 3196, 4433,", "= 2446, 3196, 4434,")],
    "green offset with ONE_HALF twice": [("x_cb + (1 << 15) + (-_fix(0.71414))", "x_cb + (1 << 16) + (-_fix(0.71414))")],
}


def mutated_oracle(name: Optional[str]) -> types.ModuleType:
    """A private copy of oracle/jpeg_oracle.py with one MUTATIONS entry applied (None: an unchanged copy)."""
    from oracle import jpeg_oracle as J
    src = Path(J.__file__).read_text()
    for old, new in (MUTATIONS[name] if name else []):
        assert src.count(old) == 1, f"{name}: {old!r} occurs {src.count(old)} times in the oracle"
        src = src.replace(old, new)
    mod = types.ModuleType("jpeg_oracle_mutated")
    exec(compile(src, f"<jpeg_oracle {name}>", "exec"), mod.__dict__)
    return mod


# Damaged headers the parser used to read past or carry on from, each the smallest byte string that gets there:
# (name, bytes, refusal, message).  test_cpu_jpeg_cases.py holds the refusals, tools/jpeg_host_check.sh the reads.
_SOF1 = seg(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0]))
_SOF3 = seg(0xC0, bytes([8, 0, 8, 0, 8, 3, 1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0]))
_TINY_DHT = seg(0xC4, dht_payload(0, 0, ((1,) + (0,) * 15, (0,))) + dht_payload(1, 0, ((1,) + (0,) * 15, (0,))))
DAMAGED = [
    # SOS of length 2: not even the component count; the count used to be read one byte past the buffer
    ("sos_without_count", b"\xff\xd8" + _SOF1 + b"\xff\xda\x00\x02", "ARG", "corrupt JPEG: SOS length"),
    # SOS that ends after its component count: the selectors used to be read two bytes past the buffer
    ("sos_without_selectors", b"\xff\xd8" + _SOF1 + b"\xff\xda\x00\x03\x01", "ARG", "corrupt JPEG: SOS length"),
    ("sos_three_components_one_selector", b"\xff\xd8" + _SOF3 + b"\xff\xda\x00\x05\x03\x01\x00", "ARG",
     "corrupt JPEG: SOS length"),
    # SOS naming component 1 twice: component 2's table selectors stayed unset and the scan was decoded with them
    ("sos_component_named_twice", b"\xff\xd8" + _SOF3 + _TINY_DHT + seg(0xDA, bytes([3, 1, 0, 1, 0, 3, 0, 0, 63, 0])),
     "UNSUPPORTED", "SOS component id"),
]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        out = Path(sys.argv[2])
        out.mkdir(parents=True, exist_ok=True)
        for c in accepted():
            (out / f"{c.name}.jpg").write_bytes(c.data)
        for name, data, _, _ in DAMAGED:
            (out / f"damaged_{name}.jpg").write_bytes(data)
        print(f"{len(accepted())} cases, {len(DAMAGED)} damaged headers -> {out}")
    else:
        sys.exit("usage: jpeg_cases.py --dump DIR")
