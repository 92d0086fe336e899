"""A baseline JPEG writer for tests, and a table of hand-built streams.

The JPEG step (sift-features_amd/csrc/jpeg.hip) and its restatement
(tests/golden/jpeg_decode.py) are written the same way, and PIL's encoder on
smooth frames leaves most of their paths to luck.  This module writes the
stream from the other end: given QUANTISED coefficient blocks, quantisation
tables, Huffman tables (counts and symbols), sampling factors, component ids,
table selectors and a restart interval, `write()` returns the bytes.  It does
DC prediction, run/size coding with ZRL and EOB, byte stuffing, RSTn insertion
with predictor reset and 1-bit padding of the last byte (ITU-T T.81 F.1.2,
B.1.1.5, E.1.4), and shares no code with either decoder.  What a decoder
returns can therefore be held against what the encoder put in.

CASES holds one named stream per property; `why` says which line of jpeg.hip
the case is for.  Each is the smallest frame that shows it.

  long_*      Huffman codes of every length 1..16 (Huff::fast stops at 9 bits,
              fast_ac at code + size = 11)
  symbols_*   every AC (run, size), both signs and both ends of each category;
              DC categories 0..11
  runs        ZRL chains, index 63 without EOB, index 62 with it, 63 ACs
  stuffing    0xFF data bytes at every offset of Bits::fill's 8-byte window
  restart_*   RSTn cycling, predictor reset, intervals that do / do not divide
  layout_*    16-bit DQT, table ids 1..3, DRI position, component ids, SOF1,
              a 65535-byte COM, fill bytes, split / joined / redefined tables
  size_*      partial MCUs whose chroma padding differs from the picture
  samp_*      all 64 combinations of (h, v) in {1, 2}^2 for three components
  idct_*      single coefficients, the DC-only shortcut, the col0 shortcut,
              dense blocks (amplitudes chosen so that a 32-bit decoder's
              intermediates stay below 2^31; the bound is asserted in
              tests/test_jpeg_streams_cpu.py)
  colour      every clamp of R, G and B from both sides
  batch_*     one size, different tables and restart intervals

A helper module, not a conftest.  Test infrastructure only.
"""
import collections
import functools

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63])
EOB, ZRL = 0x00, 0xF0

Comp = collections.namedtuple("Comp", "id h v tq td ta blocks")  # blocks[row][col][64]: quantised, natural order
Stats = collections.namedtuple("Stats", "scan_start scan_end stuffed rst symbols lengths")


class Spec:
    """One stream: the frame, its tables and the layout switches."""

    def __init__(self, w, h, comps, qt, ht, restart=0, **layout):
        self.w, self.h, self.comps, self.restart = w, h, list(comps), restart
        self.qt = qt  # id -> (64 entries in natural order, precision flag 0 / 1)
        self.ht = ht  # (class 0 DC / 1 AC, id) -> (16 counts, symbols)
        self.sof = layout.pop("sof", 0xC0)
        self.fill = layout.pop("fill", ())             # marker names written after FF FF FF
        self.extra = layout.pop("extra", ())           # (marker, payload) segments after SOI
        self.split = layout.pop("split", False)        # one table per DQT / DHT segment
        self.redefine = layout.pop("redefine", False)  # every table first defined wrongly
        self.dri_first = layout.pop("dri_first", False)
        self.tokens = layout.pop("tokens", {})         # (component, row, col) -> raw AC tokens (malformed scans)
        assert not layout, layout

    def geometry(self):
        hmax, vmax = max(c.h for c in self.comps), max(c.v for c in self.comps)
        mcux, mcuy = -(-self.w // (8 * hmax)), -(-self.h // (8 * vmax))
        return hmax, vmax, mcux, mcuy

    def dequantised(self):
        """Per component [row][col][64]: coefficient x table entry (T.81 F.2.1.4)."""
        return [np.asarray(c.blocks, np.int64) * np.asarray(self.qt[c.tq][0], np.int64) for c in self.comps]


# ---------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------
def huff_codes(table):
    """symbol -> (code, length) of the canonical code (T.81 C.2)."""
    counts, symbols = table
    assert len(counts) == 16 and len(symbols) == sum(counts) and len(set(symbols)) == len(symbols)
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            assert code < (1 << ln) - (ln == 16), "code space oversubscribed"
            out[symbols[k]] = (code, ln)
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, 0

    def put(self, value, ln):
        assert 0 <= value < (1 << ln)
        self.acc, self.n = (self.acc << ln) | value, self.n + ln
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:  # B.1.1.5: a data 0xFF is followed by a zero byte
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):  # F.1.2.3: pad the last byte with 1-bits
        if self.n:
            pad = 8 - self.n
            self.put((1 << pad) - 1, pad)

    def marker(self, m):
        self.flush()
        self.out += bytes([0xFF, m])


def _category(v):
    return int(abs(int(v))).bit_length()


def _magnitude(v, s):
    return int(v) if v >= 0 else int(v) + (1 << s) - 1


def ac_tokens(zz):
    """(symbol, extra bits, size) of the 63 AC coefficients in zigzag order."""
    out, run = [], 0
    nz = np.nonzero(zz[1:])[0]
    last = int(nz[-1]) + 1 if len(nz) else 0
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            out.append((ZRL, 0, 0))
            run -= 16
        s = _category(zz[k])
        assert 1 <= s <= 10, "baseline AC magnitudes are below 2^10"
        out.append(((run << 4) | s, _magnitude(zz[k], s), s))
        run = 0
    if last < 63:
        out.append((EOB, 0, 0))
    return out


def _segment(marker, payload, fill=False):
    assert len(payload) + 2 <= 0xFFFF
    return (b"\xff\xff\xff" if fill else b"") + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + \
        bytes(payload)


def _dqt(tq, table, precision):
    zz = [int(x) for x in np.asarray(table)[ZIGZAG]]
    assert all(1 <= x < (65536 if precision else 256) for x in zz)
    body = b"".join(x.to_bytes(2, "big") for x in zz) if precision else bytes(zz)
    return bytes([(precision << 4) | tq]) + body


def _dht(tc, th, table):
    counts, symbols = table
    return bytes([(tc << 4) | th]) + bytes(counts) + bytes(symbols)


def _wrong_q(table):
    return [int(x) % 255 + 1 for x in np.asarray(table) + 7]


def _wrong_h(table):
    counts, symbols = table
    return counts, tuple(symbols[1:]) + tuple(symbols[:1])


def write(spec):
    """(bytes, Stats) of one Spec."""
    out = bytearray(b"\xff\xd8")
    for marker, payload in spec.extra:
        out += _segment(marker, payload)
    dri = spec.restart != 0

    def put_dri():
        if dri:
            out.extend(_segment(0xDD, spec.restart.to_bytes(2, "big"), "DRI" in spec.fill))

    def put_tables(marker, parts, name):
        if spec.split:
            for i, p in enumerate(parts):
                out.extend(_segment(marker, p, name in spec.fill and i == 0))
        else:
            out.extend(_segment(marker, b"".join(parts), name in spec.fill))

    if spec.dri_first:
        put_dri()
    if spec.redefine:
        put_tables(0xDB, [_dqt(tq, _wrong_q(t), p) for tq, (t, p) in sorted(spec.qt.items())], "none")
    put_tables(0xDB, [_dqt(tq, t, p) for tq, (t, p) in sorted(spec.qt.items())], "DQT")
    sof = bytes([8]) + spec.h.to_bytes(2, "big") + spec.w.to_bytes(2, "big") + bytes([len(spec.comps)])
    for c in spec.comps:
        sof += bytes([c.id, (c.h << 4) | c.v, c.tq])
    out += _segment(spec.sof, sof, "SOF" in spec.fill)
    if not spec.dri_first:
        put_dri()
    if spec.redefine:
        put_tables(0xC4, [_dht(tc, th, _wrong_h(t)) for (tc, th), t in sorted(spec.ht.items())], "none")
    put_tables(0xC4, [_dht(tc, th, t) for (tc, th), t in sorted(spec.ht.items())], "DHT")
    sos = bytes([len(spec.comps)])
    for c in spec.comps:
        sos += bytes([c.id, (c.td << 4) | c.ta])
    out += _segment(0xDA, sos + bytes([0, 63, 0]), "SOS" in spec.fill)
    start = len(out)

    codes = {key: huff_codes(t) for key, t in spec.ht.items()}
    symbols, lengths = collections.Counter(), collections.Counter()
    bw = _BitWriter()

    def emit(tc, th, sym, extra, size):
        code, ln = codes[(tc, th)][sym]
        bw.put(code, ln)
        if size:
            bw.put(extra, size)
        symbols[(tc, th, sym)] += 1
        lengths[(tc, ln, size)] += 1

    hmax, vmax, mcux, mcuy = spec.geometry()
    for c in spec.comps:
        assert np.asarray(c.blocks).shape == (mcuy * c.v, mcux * c.h, 64), (np.asarray(c.blocks).shape, mcuy, mcux)
    pred, n, rst = [0] * len(spec.comps), 0, 0
    for my in range(mcuy):
        for mx in range(mcux):
            if spec.restart and n and n % spec.restart == 0:  # E.1.4: RSTm, m counting modulo 8
                bw.marker(0xD0 + (rst & 7))
                rst += 1
                pred = [0] * len(spec.comps)
            n += 1
            for ci, c in enumerate(spec.comps):
                for by in range(c.v):
                    for bx in range(c.h):
                        row, col = my * c.v + by, mx * c.h + bx
                        zz = np.asarray(c.blocks[row][col])[ZIGZAG]
                        diff, pred[ci] = int(zz[0]) - pred[ci], int(zz[0])
                        s = _category(diff)
                        emit(0, c.td, s, _magnitude(diff, s), s)
                        for sym, extra, size in spec.tokens.get((ci, row, col), None) or ac_tokens(zz):
                            emit(1, c.ta, sym, extra, size)
    bw.flush()
    out += bw.out
    end = len(out)
    out += b"\xff\xff\xff\xff\xd9" if "EOI" in spec.fill else b"\xff\xd9"
    return bytes(out), Stats(start, end, bw.stuffed, rst, symbols, lengths)


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
ALL_AC = tuple([EOB, ZRL] + [(r << 4) | s for s in range(1, 11) for r in range(16)])  # 162 symbols
ALL_DC = tuple(range(12))


def _counts(**at):
    c = [0] * 16
    for k, v in at.items():
        c[int(k[1:]) - 1] = v
    return tuple(c)


# every symbol at 8 bits (DC: 4 bits): all of them inside the 9-bit lookahead
FLAT_DC = (_counts(n4=12), ALL_DC)
FLAT_AC = (_counts(n8=162), ALL_AC)
# lengths 2..16 with the count vector of T.81 table K.5, symbols in this module's own order
# (by size, then run), and the same reversed: the large sizes get the short codes
K5_COUNTS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
SPREAD_AC = (K5_COUNTS, ALL_AC)
SPREAD_AC_REV = (K5_COUNTS, tuple(reversed(ALL_AC)))
SPREAD_DC = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), ALL_DC)
SPREAD_DC_REV = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(reversed(ALL_DC)))
# one code of every length 1..16; the symbol at position i has a code of i + 1 bits
ONE_EACH = (1,) * 16
LONG_DC_A = (ONE_EACH, (2, 3, 1, 4, 0, 5, 12, 13, 6, 7, 8, 9, 14, 15, 10, 11))
LONG_DC_B = (ONE_EACH, (15, 14, 13, 12, 0, 1, 2, 11, 3, 4, 5, 6, 10, 9, 8, 7))
#             length:   1     2     3     4     5     6    7     8     9     10    11    12    13    14    15    16
LONG_AC_A = (ONE_EACH, (0x01, EOB, 0x02, 0x11, 0x03, ZRL, 0x04, 0x12, 0x13, 0x31, 0x22, 0x0A, 0x41, 0x06, 0x51, 0x07))
LONG_AC_B = (ONE_EACH, (EOB, 0x11, 0x01, 0x21, 0x05, 0x07, 0x03, 0x04, 0x02, 0x12, 0x31, 0x41, ZRL, 0x0A,
                        0x06, 0x22))
# the stuffing case's table: byte-aligned tokens (see _stuffing)
STUFF_DC = (_counts(n8=12), ALL_DC)
_S4 = (0x04, 0x02, 0x11, 0x0A, 0x21, 0x31, 0x41, 0x51, 0x61, 0x71, 0x81, 0x91, 0xA1, 0xB1)          # 0000 .. 1101
_S8 = (EOB, ZRL, 0x08, 0x12, 0x22, 0x32, 0x42, 0x52, 0x62, 0x72, 0x82, 0x92, 0xA2, 0xB2, 0xC2, 0xD2,  # 0xE0 .. 0xEF
       0x14, 0x13, 0x23, 0x33, 0x43, 0x53, 0x63, 0x73, 0x83, 0x93, 0xA3, 0xB3, 0xC3, 0xD3, 0xE3)      # 0xF0 .. 0xFE
STUFF_AC = (_counts(n4=14, n8=31), _S4 + _S8)

Q_ONE = [1] * 64


def q_ramp(lo, step, cap=255):
    """A table growing along the zigzag, as encoders' tables do."""
    t = np.zeros(64, np.int64)
    t[ZIGZAG] = np.minimum(lo + step * np.arange(64), cap)
    return [int(x) for x in t]


Q_FINE, Q_MID, Q_COARSE = q_ramp(1, 1), q_ramp(3, 2), q_ramp(16, 5)


# ---------------------------------------------------------------------------
# block builders
# ---------------------------------------------------------------------------
def zz_block(dc, ac=()):
    """Natural-order block from a DC value and {zigzag index: value}."""
    zz = np.zeros(64, np.int64)
    zz[0] = dc
    for k, v in dict(ac).items():
        assert 1 <= k <= 63
        zz[k] = v
    out = np.zeros(64, np.int64)
    out[ZIGZAG] = zz
    return out


def grid(blocks, cols):
    """[row][col][64] from a list of natural-order blocks (zero blocks pad the last row)."""
    blocks = list(blocks)
    rows = -(-len(blocks) // cols)
    out = np.zeros((rows, cols, 64), np.int64)
    for i, b in enumerate(blocks):
        out[i // cols, i % cols] = b
    return out


def random_blocks(rng, rows, cols, dc=40, ac=30, keep=0.5, tail=12):
    """Blocks with strong low frequencies and a sparse tail, DC varying from block to block."""
    zz = np.zeros((rows, cols, 64), np.int64)
    zz[..., 0] = rng.integers(-dc, dc + 1, (rows, cols))
    env = np.maximum(1, (ac / (1 + 0.35 * np.arange(1, 64))).astype(np.int64))
    vals = rng.integers(-env, env + 1, (rows, cols, 63))
    zz[..., 1:] = np.where(rng.random((rows, cols, 63)) < keep, vals, 0)
    zz[..., tail:] *= rng.random((rows, cols, 64 - tail)) < 0.25
    out = np.zeros_like(zz)
    out[..., ZIGZAG] = zz
    return out


def gray_spec(w, h, blocks, q=Q_MID, dc=FLAT_DC, ac=FLAT_AC, precision=0, **kw):
    return Spec(w, h, [Comp(1, 1, 1, 0, 0, 0, blocks)], {0: (q, precision)}, {(0, 0): dc, (1, 0): ac}, **kw)


SAMPLING = {"444": ((1, 1), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "420": ((2, 2), (1, 1), (1, 1))}


def colour_spec(w, h, sampling, seed, qy=Q_MID, qc=Q_COARSE, tables=None, ids=(1, 2, 3), tq=(0, 1, 1), sel=None,
                flat=(), chroma_ac=60, **kw):
    """Three components of random blocks; `flat` lists components that are one value throughout."""
    rng = np.random.default_rng(seed)
    hv = SAMPLING[sampling] if isinstance(sampling, str) else sampling
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    tables = tables or {(0, 0): FLAT_DC, (1, 0): FLAT_AC, (0, 1): SPREAD_DC, (1, 1): SPREAD_AC}
    sel = sel or ((0, 0), (1, 1), (1, 1))
    comps = []
    for k, (ch, cv) in enumerate(hv):
        if k in flat:
            blocks = np.zeros((mcuy * cv, mcux * ch, 64), np.int64)
            blocks[..., 0] = (-9, 7, 4)[k]
        else:
            blocks = random_blocks(rng, mcuy * cv, mcux * ch, dc=(40, 12, 12)[k], ac=(30, chroma_ac, chroma_ac)[k])
        comps.append(Comp(ids[k], ch, cv, tq[k], sel[k][0], sel[k][1], blocks))
    qt = {0: (qy, 0), 1: (qc, 0)} if not isinstance(qy, dict) else qy
    return Spec(w, h, comps, qt, tables, **kw)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name why make")
CASES = collections.OrderedDict()


def case(name, why):
    def add(fn):
        assert name not in CASES
        CASES[name] = Case(name, why, fn)
        return fn
    return add


@functools.lru_cache(maxsize=None)
def spec(name):
    return CASES[name].make()


@functools.lru_cache(maxsize=None)
def stream(name):
    """(bytes, Stats) of a named case."""
    return write(spec(name))


# -- long codes -------------------------------------------------------------
def _long_blocks(ac_table, n_blocks, seed):
    """Blocks that use every symbol of a 16-symbol AC table, and DC categories 0..11."""
    rng = np.random.default_rng(seed)
    syms = [s for s in ac_table[1] if s not in (EOB, ZRL)]
    diffs = [0] + [sg * int(rng.integers(1 << (s - 1), 1 << s)) for s in range(1, 12) for sg in (1, -1)]
    blocks, dcv, i = [], 0, 0
    while len(blocks) < n_blocks:
        ac, k = {}, 1
        while True:
            sym = syms[i % len(syms)]
            r, s = sym >> 4, sym & 15
            if k + r > 63:
                break
            ac[k + r] = int(rng.integers(1 << (s - 1), 1 << s)) * (1 if rng.random() < 0.5 else -1)
            k += r + 1
            i += 1
            if rng.random() < 0.2:
                break
        if len(blocks) % 3 == 2 and k < 30:  # a ZRL in every third block
            ac[k + 20] = 1
        dcv += diffs[len(blocks) % len(diffs)]
        blocks.append(zz_block(dcv, ac))
    return blocks


@case("long_gray", "codes of 1..16 bits in DC and AC: Huff::fast ends at 9 bits, fast_ac at code + size = 11; "
                   "code + size of 10, 11, 12 and up to 23")
def _():
    return gray_spec(48, 40, grid(_long_blocks(LONG_AC_A, 30, 1), 6), q=Q_ONE, dc=LONG_DC_A, ac=LONG_AC_A)


@case("long_420", "the same with another arrangement (a 10-bit code with size 2, a 16-bit code with size 2), "
                  "different tables for luma and chroma, in 4:2:0")
def _():
    y = grid(_long_blocks(LONG_AC_B, 16, 2), 4)
    cb, cr = grid(_long_blocks(LONG_AC_A, 4, 3), 2), grid(_long_blocks(LONG_AC_B, 4, 4), 2)
    ht = {(0, 0): LONG_DC_B, (1, 0): LONG_AC_B, (0, 1): LONG_DC_A, (1, 1): LONG_AC_A}
    return Spec(32, 32, [Comp(1, 2, 2, 0, 0, 0, y), Comp(2, 1, 1, 1, 1, 1, cb), Comp(3, 1, 1, 1, 1, 0, cr)],
                {0: (Q_ONE, 0), 1: ([2] * 64, 0)}, ht)


# -- symbols ------------------------------------------------------------------
def _symbol_blocks():
    """Every (run, size), run 0..15, size 1..10, at +-2^(s-1) and +-(2^s - 1); DC differences of every
    category at the same four values, so +-2047 among them."""
    toks = [(r, v) for s in range(1, 11) for r in range(16)
            for v in ((1 << (s - 1)), -(1 << (s - 1)), (1 << s) - 1, -((1 << s) - 1))]
    diffs = [0] + [v for s in range(1, 12) for v in ((1 << (s - 1)), -(1 << (s - 1)), (1 << s) - 1, -((1 << s) - 1))]
    blocks, ac, k, dcv = [], {}, 1, 0
    for r, v in toks:
        if k + r > 63:
            dcv += diffs[len(blocks) % len(diffs)]
            blocks.append(zz_block(dcv, ac))
            ac, k = {}, 1
        ac[k + r] = v
        k += r + 1
    blocks.append(zz_block(dcv, ac))
    while len(blocks) < len(diffs) or len(blocks) % 12:
        dcv += diffs[len(blocks) % len(diffs)]
        blocks.append(zz_block(dcv))
    return blocks


@case("symbols_flat", "every AC (run, size) and DC category at both signs and both ends, codes of 8 / 4 bits: "
                      "extend() at its boundaries, fast_ac for sizes 1..3 only")
def _():
    b = _symbol_blocks()
    return gray_spec(96, 8 * (len(b) // 12), grid(b, 12), q=Q_ONE)


@case("symbols_spread", "the same symbols with codes of 2..16 bits: each (length, size) pair on its own side of "
                        "fast_ac's limit")
def _():
    b = _symbol_blocks()
    return gray_spec(96, 8 * (len(b) // 12), grid(b, 12), q=Q_ONE, dc=SPREAD_DC, ac=SPREAD_AC)


@case("symbols_spread_rev", "the reversed arrangement: sizes 8..10 behind the short codes")
def _():
    b = _symbol_blocks()
    return gray_spec(96, 8 * (len(b) // 12), grid(b, 12), q=Q_ONE, dc=SPREAD_DC_REV, ac=SPREAD_AC_REV)


# -- runs -----------------------------------------------------------------------
RUN_BLOCKS = [
    zz_block(5, {40: 3, 63: -2}),            # 22 zeros: ZRL + run 6, index 63, no EOB
    zz_block(-7, {20: -1, 63: 9}),           # 42 zeros: ZRL ZRL + run 10
    zz_block(11, {5: 2, 63: 1}),             # 57 zeros: ZRL ZRL ZRL + run 9
    zz_block(0, {15: 1, 31: -1, 47: 1, 63: -1}),  # run 15 four times: no ZRL, ends on 63
    zz_block(3, {14: 1, 31: 1, 63: 5}),      # 16 zeros: ZRL + run 0; 31: ZRL + run 15
    zz_block(-3, {14: 4, 63: 4}),            # 48 zeros: ZRL ZRL ZRL + run 0
    zz_block(9),                              # EOB straight after DC
    zz_block(9),                              # ... and a DC difference of 0 before it
    zz_block(-20, {62: 7}),                  # index 62, then EOB
    zz_block(1, {k: (-1) ** k * (1 + k % 7) for k in range(1, 64)}),  # 63 ACs, no EOB
    zz_block(2, {63: -1023}),                # ZRL ZRL ZRL + run 14, the largest magnitude
    zz_block(0, {1: 1}),
]


@case("runs", "ZRL chains of 1, 2 and 3 before index 63 without EOB, EOB after DC, index 62 + EOB, 63 ACs: "
              "the k > 63 check and the loop end of entropy_decode")
def _():
    return gray_spec(32, 24, grid(RUN_BLOCKS, 4), q=Q_ONE)


def _runs_table(blocks):
    """A 16-symbol AC table, one code per length, that holds what `blocks` need: EOB at 2 bits, ZRL at 13,
    the longest runs behind it."""
    need = sorted({t[0] for b in blocks for t in ac_tokens(b[ZIGZAG])} - {EOB, ZRL})
    assert 4 <= len(need) <= 14
    spare = [s for s in ALL_AC[2:] if s not in need]
    rest = spare[:14 - len(need)] + need[1:]
    return (ONE_EACH, tuple(need[:1] + [EOB] + rest[:10] + [ZRL] + rest[10:]))


@case("runs_long_codes", "the same runs with coefficients of +-1 through the bit-by-bit Huffman walk (ZRL at 13 "
                         "bits, run 15 at 16)")
def _():
    blocks = [zz_block(b[0], {k: int(np.sign(b[ZIGZAG][k])) for k in range(1, 64) if b[ZIGZAG][k]})
              for b in RUN_BLOCKS]
    return gray_spec(32, 24, grid(blocks, 4), q=Q_FINE, dc=LONG_DC_B, ac=_runs_table(blocks))


# -- stuffing -------------------------------------------------------------------
def _stuffing():
    """One row of gray blocks whose scan is a chosen byte sequence.  With STUFF_DC / STUFF_AC every token
    below is a whole number of bytes: DC difference 0 = one byte (0x00); EOB = 0xE0; (0, 4) = 0000vvvv; (0, 8)
    = 0xE2 then the value byte, 0xFF for +255; and the 4-byte group (0, 2), (0, 10) = 1023, (1, 4), that is
    cccc vv 0011 | 1111 1111 | 1111 1111 | 0000 vvvv: a pair of 0xFF.  Returns (blocks, expected stuffed bytes)."""
    rng = np.random.default_rng(12)
    blocks, ac, k, pos, ff, clean = [], {}, 1, 1, 0, 1  # pos: scan offset of the next byte (after the DC byte)

    def close(last=False):
        nonlocal ac, k, pos, clean
        blocks.append(zz_block(0, ac))
        if k <= 63:
            pos, clean = pos + 1, clean + 1  # EOB
        if not last:
            pos, clean = pos + 1, clean + 1  # the next block's DC
        ac, k = {}, 1

    def room(n):
        if k + n > 64:
            close()

    def pad():
        nonlocal k, pos, clean
        room(1)
        ac[k] = int(rng.choice([-15, -12, -9, -8, 8, 10, 13, 15]))
        k, pos, clean = k + 1, pos + 1, clean + 1

    def one_ff(value=255):
        nonlocal k, pos, clean, ff
        room(1)
        ac[k] = value
        k, pos = k + 1, pos + 1  # the code byte
        if value == 255:
            pos, ff, clean = pos + 2, ff + 1, 0
        else:
            pos, clean = pos + 1, clean + 1

    def pair():
        nonlocal k, pos, clean, ff
        room(5)
        ac[k], ac[k + 1], ac[k + 3] = 2, 1023, int(rng.choice([-15, -8, 9, 14]))
        k, pos, ff, clean = k + 4, pos + 1 + 4 + 1, ff + 2, 1

    for r in range(8):  # isolated: >= 16 clean bytes, then a 0xFF at scan offset r (mod 8)
        while clean < 17 or (pos + 1) % 8 != r:
            pad()
        one_ff()
    for r in range(8):  # the same residues counted with the stuffed zeros of the file
        for _ in range(3 + r):
            pad()
        one_ff()
    for _ in range(3):  # pairs, and a pair right after a single
        for _ in range(5):
            pad()
        pair()
    one_ff()
    pair()
    for v in (255, 254, 255, -255, 255, 255, 128, 255):  # dense: 0xFF, 0xFE, 0xFF, 0x00, ...
        one_ff(v)
    for _ in range(9):
        pad()
    while k < 63:  # the last data byte before EOI: +255 at index 63, no EOB
        pad()
    one_ff()
    close(last=True)
    return blocks, ff


@case("stuffing", "0xFF data bytes isolated at every offset of an 8-byte window, in pairs, packed, and as the "
                  "last byte before EOI: Bits::fill's 8-byte path and its byte-wise fallback")
def _():
    blocks, _ = _stuffing()
    return gray_spec(8 * len(blocks), 8, grid(blocks, len(blocks)), q=Q_ONE, dc=STUFF_DC, ac=STUFF_AC)


STUFFED_BYTES = _stuffing()[1]


# -- restarts -------------------------------------------------------------------
RESTART_INTERVALS = collections.OrderedDict([  # name -> (Ri, RSTn markers in a 12-MCU scan)
    ("1", (1, 11)), ("row", (4, 2)), ("5", (5, 2)), ("12", (12, 0)), ("13", (13, 0))])

for _name, (_ri, _) in RESTART_INTERVALS.items():
    @case("restart_420_" + _name, "Ri = %d over 4 x 3 MCUs of 4:2:0, DC non-zero and varying in every component: "
          "the predictor reset of all three, RST7 -> RST0 at Ri = 1, no marker at Ri >= 12" % _ri)
    def _(ri=_ri):
        return colour_spec(64, 48, "420", 20 + ri, restart=ri)

    @case("restart_gray_" + _name, "Ri = %d over 4 x 3 blocks of gray" % _ri)
    def _(ri=_ri):
        return gray_spec(32, 24, random_blocks(np.random.default_rng(40 + ri), 3, 4), restart=ri, dc=SPREAD_DC,
                         ac=SPREAD_AC)


# -- layout ---------------------------------------------------------------------
def _layout(**kw):
    return colour_spec(24, 16, "420", 5, **kw)


@case("layout_dqt16_small", "16-bit DQT (Pq = 1) with every entry <= 255")
def _():
    return _layout(qy={0: (Q_MID, 1), 1: (Q_COARSE, 1)})


@case("layout_dqt16_large", "16-bit DQT with entries up to 1000: the high byte reaches the dequantisation")
def _():
    big = q_ramp(200, 13, cap=1000)
    s = colour_spec(24, 16, "420", 6, qy={0: (big, 1), 1: (q_ramp(256, 9, cap=800), 1)}, chroma_ac=4)
    for c in s.comps:  # small coefficients: the products stay inside 16 bits
        np.clip(c.blocks, -3, 3, out=c.blocks)
    return s


@case("layout_table_ids", "quantisation tables 1, 2, 3 (all different) and Huffman tables 1, 2, 3; nothing has id 0")
def _():
    ht = {(0, 1): FLAT_DC, (1, 1): FLAT_AC, (0, 2): SPREAD_DC, (1, 2): SPREAD_AC, (0, 3): SPREAD_DC_REV,
          (1, 3): SPREAD_AC_REV}
    return _layout(qy={1: (Q_FINE, 0), 2: (Q_MID, 0), 3: (Q_COARSE, 0)}, tq=(1, 2, 3), tables=ht,
                   sel=((1, 1), (2, 2), (3, 3)))


@case("layout_dri_before_sof", "DRI ahead of the frame header")
def _():
    return _layout(restart=1, dri_first=True)


@case("layout_dri_after_sof", "DRI between the frame header and the Huffman tables")
def _():
    return _layout(restart=1)


@case("layout_ids_012", "component ids 0, 1, 2: the scan header's selectors are matched by id, not by position")
def _():
    return _layout(ids=(0, 1, 2))


@case("layout_ids_rgb", "component ids 82, 71, 66 ('R', 'G', 'B'): still decoded as YCbCr, as the restatement does")
def _():
    return _layout(ids=(82, 71, 66))


@case("layout_sof1", "SOF1 (extended sequential Huffman) with 8-bit samples")
def _():
    return _layout(sof=0xC1)


@case("layout_com_65535", "a COM segment of the largest length and two APPn segments before the tables")
def _():
    return _layout(extra=((0xFE, bytes(range(256)) * 255 + bytes(253)), (0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0"),
                          (0xEE, b"\xff\xd8\xff\xda inside a payload")))


@case("layout_fill", "FF FF FF before SOF, DHT, SOS and EOI: the fill-byte loop of parse")
def _():
    return _layout(fill=("SOF", "DHT", "SOS", "EOI"))


@case("layout_split", "one table per DQT / DHT segment")
def _():
    return _layout(split=True)


@case("layout_redefined", "every table defined twice, the first definition wrong: the last one wins")
def _():
    return _layout(redefine=True)


@case("layout_redefined_split", "the same with one table per segment")
def _():
    return _layout(redefine=True, split=True, restart=2)


def without_fill(s):
    """The same stream without fill bytes (the restatement's parse has no fill-byte loop)."""
    return Spec(s.w, s.h, s.comps, s.qt, s.ht, s.restart, sof=s.sof, extra=s.extra, split=s.split,
                redefine=s.redefine, dri_first=s.dri_first, tokens=s.tokens)


# -- sizes ----------------------------------------------------------------------
SIZES = {"gray": [(1, 1), (7, 9), (8, 8), (9, 8), (33, 1), (1, 33)],
         "444": [(1, 1), (7, 9), (8, 8), (9, 8), (33, 1), (1, 33)],
         "420": [(2, 2), (15, 15), (16, 16), (17, 17), (31, 18)],
         "422": [(15, 9), (17, 9), (31, 9)]}

for _mode, _sizes in SIZES.items():
    for _w, _h in _sizes:
        @case("size_%s_%dx%d" % (_mode, _w, _h), "%d x %d in %s: partial MCUs; strong AC in every plane, so the "
              "block padding that sample()'s clamps reach differs from the picture" % (_w, _h, _mode))
        def _(mode=_mode, w=_w, h=_h):
            if mode == "gray":
                rng = np.random.default_rng(100 + 7 * w + h)
                return gray_spec(w, h, random_blocks(rng, -(-h // 8), -(-w // 8), ac=60))
            return colour_spec(w, h, mode, 200 + 7 * w + h, qc=Q_MID)


# -- sampling -------------------------------------------------------------------
HV = [(1, 1), (2, 1), (1, 2), (2, 2)]


def sampling_supported(hv):
    """The restatement's cases: every component is full size, h2v1 or h2v2 against the largest factors."""
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    return all((hmax // a, vmax // b) != (1, 2) for a, b in hv)


def _h1v2(hv):
    hmax, vmax = max(a for a, _ in hv), max(b for _, b in hv)
    return tuple(k for k, (a, b) in enumerate(hv) if (hmax // a, vmax // b) == (1, 2))


SAMPLING_CASES = collections.OrderedDict()
for _a in HV:
    for _b in HV:
        for _c in HV:
            _hv = (_a, _b, _c)
            _n = "samp_" + "_".join("%dx%d" % x for x in _hv)
            SAMPLING_CASES[_n] = _hv

            @case(_n, "17 x 19 with sampling %s: %s" % (_hv, "decoded" if sampling_supported(_hv) else
                  "vertical-only upsampling of a component, which the library refuses (that component is flat, "
                  "so that any upsampler gives libjpeg's result)"))
            def _(hv=_hv, n=_n):
                return colour_spec(17, 19, hv, sum(map(ord, n)), qc=Q_MID, flat=_h1v2(hv))


# -- IDCT -----------------------------------------------------------------------
def _single(coef, q):
    blocks = []
    for sign in (1, -1):
        for pos in range(64):
            b = np.zeros(64, np.int64)
            b[pos] = sign * coef
            blocks.append(b)
    return gray_spec(128, 64, grid(blocks, 16), q=[q] * 64, dc=SPREAD_DC, ac=SPREAD_AC)


for _amp, _coef, _q in ((1, 1, 1), (64, 64, 1), (8192, 64, 128)):
    @case("idct_single_%d" % _amp, "one coefficient of +-%d (dequantised: %d x %d) at each of the 64 positions: "
          "every basis function, rounding at the smallest value, both clamps at the largest" % (_amp, _coef, _q))
    def _(coef=_coef, q=_q):
        return _single(coef, q)


DC_ONLY = list(range(-1031, -1016)) + list(range(1016, 1032))


@case("idct_dc_only", "DC-only blocks with DC x q from -1031 to -1017 and 1016 to 1031: (DC >> 3) + 128 floors "
                      "negative odd values and clamps at 0 and 255")
def _():
    blocks = [zz_block(v) for v in DC_ONLY] + [zz_block(v) for v in (-1, 1, -7, 7, -8, 8, -9, 9, 0)]
    return gray_spec(64, 40, grid(blocks, 8), q=Q_ONE, dc=SPREAD_DC, ac=SPREAD_AC)


def _row0_blocks(extra):
    rng = np.random.default_rng(77)
    blocks = []
    for i in range(16):
        b = np.zeros(64, np.int64)
        n = 1 + i % 7
        cols = rng.permutation(np.arange(1, 8))[:n]
        b[cols] = rng.integers(-60, 61, n)
        b[0] = rng.integers(-100, 101)
        if i == 15:
            b[:8] = [0, 0, 0, 0, 0, 0, 0, 1]  # DC zero, the smallest row-0 coefficient
        if extra:
            b[7 * 8 + 3] = (-1) ** i * (1 + i)
        blocks.append(b)
    return blocks


@case("idct_row0", "non-zero coefficients in row 0 only: every column takes the col0 shortcut (c[u] * 4), the "
                   "block is not DC-only")
def _():
    return gray_spec(32, 32, grid(_row0_blocks(False), 4), q=[4] * 64)


@case("idct_row0_plus", "the same blocks plus one coefficient at (7, 3): column 3 alone takes the full column pass")
def _():
    return gray_spec(32, 32, grid(_row0_blocks(True), 4), q=[4] * 64)


# amplitudes of the dense blocks (quantised), chosen so that no intermediate of the 12-bit fixed-point IDCT
# reaches 2^31 (asserted in tests/test_jpeg_streams_cpu.py): 8 x amplitude x q x 12586 at the column pass,
# about 8 x (column output) x 12586 at the row pass
DENSE_AMPLITUDE = {1: 1023, 255: 6}


def _dense(q):
    rng = np.random.default_rng(900 + q)
    a = DENSE_AMPLITUDE[q]
    blocks = rng.integers(-a, a + 1, (4, 4, 64))
    blocks[0, 0, :] = a * np.where(np.arange(64) % 2, -1, 1)
    blocks[0, 1, :] = a
    blocks[0, 2, :] = -a
    return gray_spec(32, 32, blocks, q=[q] * 64)


for _q in DENSE_AMPLITUDE:
    @case("idct_dense_q%d" % _q, "all 64 coefficients random in +-%d at q = %d, and blocks of all +a, all -a and "
          "alternating signs" % (DENSE_AMPLITUDE[_q], _q))
    def _(q=_q):
        return _dense(q)


# -- colour ---------------------------------------------------------------------
COLOUR_Y = [0, 1, 127, 128, 254, 255]
COLOUR_C = sorted([0, 1, 127, 128, 129, 254, 255] + list(range(5, 250, 10)))  # 32 values


def colour_values():
    """(64, 96) arrays of the flat Y, Cb, Cr value of every 8 x 8 block of the colour frame."""
    y, cb, cr = np.meshgrid(COLOUR_Y, COLOUR_C, COLOUR_C, indexing="ij")
    return y.reshape(64, 96), cb.reshape(64, 96), cr.reshape(64, 96)


@case("colour", "768 x 512, 4:4:4, DC-only blocks with q = 8 and DC = v - 128, so block = flat v: Y in "
                "{0, 1, 127, 128, 254, 255} x 32 values of Cb x 32 of Cr reach every clamp of R, G and B from "
                "both sides")
def _():
    comps = []
    for k, v in enumerate(colour_values()):
        blocks = np.zeros((64, 96, 64), np.int64)
        blocks[..., 0] = v - 128
        comps.append(Comp(k + 1, 1, 1, 0, k and 1, k and 1, blocks))
    ht = {(0, 0): FLAT_DC, (1, 0): FLAT_AC, (0, 1): SPREAD_DC, (1, 1): SPREAD_AC}
    return Spec(768, 512, comps, {0: ([8] * 64, 0)}, ht)


def colour_luma(y, cb, cr):
    """The closed form of jpeg.hip's file comment on flat values (int64 arrays)."""
    cb, cr = cb - 128, cr - 128
    r = np.clip(y + ((45 * cr) >> 5), 0, 255)
    g = np.clip(y - ((11 * cb + 23 * cr) >> 5), 0, 255)
    b = np.clip(y + ((113 * cb) >> 6), 0, 255)
    return np.minimum((2126 * r + 7152 * g + 722 * b) // 10000, 255)


# -- batch ----------------------------------------------------------------------
BATCH_VARIANTS = [  # (tables luma, tables chroma, qy, qc, Ri) at 40 x 24 in 4:2:0: 3 x 2 MCUs
    ((FLAT_DC, FLAT_AC), (SPREAD_DC, SPREAD_AC), Q_FINE, Q_MID, 0),
    ((SPREAD_DC, SPREAD_AC), (FLAT_DC, FLAT_AC), Q_MID, Q_COARSE, 1),
    ((SPREAD_DC_REV, SPREAD_AC_REV), (SPREAD_DC, SPREAD_AC), Q_COARSE, Q_FINE, 2),
    ((FLAT_DC, SPREAD_AC), (SPREAD_DC_REV, FLAT_AC), Q_MID, Q_MID, 4),
    ((SPREAD_DC, FLAT_AC), (FLAT_DC, SPREAD_AC_REV), Q_FINE, Q_COARSE, 3),
    ((STUFF_DC, SPREAD_AC_REV), (SPREAD_DC, SPREAD_AC), q_ramp(2, 3), Q_FINE, 6),
]
BATCH = ["batch_%d" % i for i in range(len(BATCH_VARIANTS))]

for _i, _v in enumerate(BATCH_VARIANTS):
    @case(BATCH[_i], "40 x 24 in 4:2:0, variant %d of the batch frames: own Huffman and quantisation tables, "
          "Ri = %d" % (_i, _v[4]))
    def _(i=_i, v=_v):
        ht = {(0, 0): v[0][0], (1, 0): v[0][1], (0, 1): v[1][0], (1, 1): v[1][1]}
        return colour_spec(40, 24, "420", 300 + i, qy=v[2], qc=v[3], tables=ht, restart=v[4])


def overrun_stream():
    """batch_0's size and sampling with one block whose AC tokens run past index 63 (run 15, three times
    over, then a coefficient): the library's "coefficient index out of range"."""
    s = spec(BATCH[0])
    tok = [(0xF1, 1, 1)] * 4
    bad = Spec(s.w, s.h, s.comps, s.qt, s.ht, s.restart, tokens={(0, 1, 2): tok})
    return write(bad)[0]


WELL_FORMED = list(CASES)
