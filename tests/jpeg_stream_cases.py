"""Baseline JPEG streams DESIGNED for the device entropy decoder (lane_slam_amd/csrc/k_jhuff.hip): a stream writer that takes
quantised coefficient blocks and writes the file, and the catalogue of cases placed against the decoder's own thresholds.

The writer reuses tests/jpeg_enc_ref.py's huff_table and scan_bytes.  A caller gives the blocks in scan order (natural
coefficient order, TRUE DC values: what oracle.jpeg_coefficients returns), the size, the component layout, quantisation tables
(8 or 16 bit), Huffman tables as (bits, vals) per (class, id) with the component selectors free, and the restart interval.  The
escape hatch is `raw_ac` / `raw_dc`: per block a list of literal tokens (symbol, extra bits, number of extra bits; symbol None =
bits without a code), for what an encoder never writes.  `hooks` damage the marker structure: a fill byte before an RSTn, a wrong
RSTn number, a dropped RSTn, a byte of 1-bits in front of a marker, blocks after the last MCU, a block left out, a cut tail.

Every stream records where each of its symbols starts in the CLEAN scan (unstuffed, markers removed: the decoder's coordinates),
by the plain sequential sum of the token lengths.  A case's CENSUS is a list of (property, observed, holds) rows computed from
that record: it states what the case was built for, and tests/test_jpeg_stream_cases_cpu.py asserts every row.  Cases whose
property depends on byte positions are found by a deterministic search (a seed loop or filler in front); the census proves they
landed.  The constants below mirror k_jhuff.hip; the CPU test reads the kernel's text and fails when they part.
"""
import functools

import numpy as np

import jpeg_enc_ref as R

# ---- k_jhuff.hip's thresholds (checked against its text by the CPU test)
JH_SB = 48                   # clean bytes per subsequence
JH_TD = 512                  # k_jh_decode's workgroup
JH_T = 256                   # k_jh_unstuff's workgroup
JH_DL = 2048                 # subsequences a dirty list holds: more, and the passes run unlisted with sup = 1
JH_LDS_CLEAN = 96 * 1024     # LDS for the clean scan
JH_CHUNK = 128               # raw bytes per thread and round in jh_unstuff_body
ROUND_UNSTUFF = JH_T * JH_CHUNK      # 32 768: a round of k_jh_unstuff
ROUND_DECODE = JH_TD * JH_CHUNK      # 65 536: a round of the decoder's own unstuffing
NBLK_FIELD_MAX = 255         # the "blocks completed" field of h_pn is 8 bits wide
WAVE = 64

OK, ERR_UNSUPPORTED, ERR_DECODE = 0, -5, -6

LAYOUTS = {"gray": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}


def std_huff():
    return {(0, 0): (R.DC_LUMA_BITS, R.DC_VALS), (1, 0): (R.AC_LUMA_BITS, R.AC_LUMA_VALS),
            (0, 1): (R.DC_CHROMA_BITS, R.DC_VALS), (1, 1): (R.AC_CHROMA_BITS, R.AC_CHROMA_VALS)}


def geometry(rows, cols, layout):
    """(ncomp, luma blocks per MCU, blocks per MCU, MCU count, component of each block of an MCU)"""
    ncomp, h, v = LAYOUTS[layout]
    mcux, mcuy = -(-cols // (8 * h)), -(-rows // (8 * v))
    luma = 1 if ncomp == 1 else h * v
    bpm = 1 if ncomp == 1 else luma + 2
    comp = [0 if r < luma else r - luma + 1 for r in range(bpm)]
    return ncomp, luma, bpm, mcux * mcuy, comp


def n_blocks(rows, cols, layout):
    _, _, bpm, n_mcu, _ = geometry(rows, cols, layout)
    return bpm * n_mcu


class Stream(object):
    """data: the file.  scan: the entropy-coded bytes between SOS and EOI.  tok_*: one entry per symbol (code + its extra bits) --
    seg (restart interval), bit (start, in bits from the interval's first clean byte), len, blk (scan-order block), last (the symbol
    completes its block).  seg_len / seg_begin: clean bytes of every interval and where it starts in the clean scan."""

    def clean_len(self):
        return int(self.seg_len.sum())

    def n_sub_per_seg(self):
        return np.maximum(1, -(-self.seg_len // JH_SB))

    def n_sub(self):
        return int(self.n_sub_per_seg().sum())

    def tok_global_bit(self):
        return self.seg_begin[self.tok_seg] * 8 + self.tok_bit

    def tok_sub(self):
        """the subsequence (counted through the frame) a symbol starts in: the last one of an interval takes what is left"""
        per = self.n_sub_per_seg()
        first = np.cumsum(per) - per
        local = np.minimum(self.tok_bit // (8 * JH_SB), per[self.tok_seg] - 1)
        return first[self.tok_seg] + local

    def blocks_per_sub(self):
        return np.bincount(self.tok_sub()[self.tok_last], minlength=self.n_sub())

    def raw_ff_offsets(self, second):
        """raw offsets (from the scan's first byte) of the 0xFF bytes that `second` (a set of byte values) follows"""
        b = np.frombuffer(self.scan + b"\xff\xd9", np.uint8)
        ff = np.flatnonzero(b[:-1] == 0xFF)
        return ff[np.isin(b[ff + 1], list(second))]

    # what launch_jh_decode and k_jh_decode decide from the sizes, for a batch whose longest scan is max_raw
    def lds_bytes(self, max_raw=None):
        m = len(self.scan) if max_raw is None else max_raw
        return min((m + 64 + (m + 64) // 32 + 32 + 15) & ~15, JH_LDS_CLEAN)

    def unstuffs_in_decoder(self, max_raw=None):
        m = len(self.scan) if max_raw is None else max_raw
        lds_raw = (m + m // 32 + 64 + 15) & ~15
        return lds_raw <= JH_LDS_CLEAN and lds_raw <= self.lds_bytes(max_raw)

    def clean_in_lds(self, max_raw=None):
        c = self.clean_len()
        return (c + 48) + (c + 48) // 32 + 16 <= self.lds_bytes(max_raw)

    def listed(self):
        return self.n_sub() <= JH_DL

    def sup(self):
        _, _, bpm, _, _ = geometry(self.rows, self.cols, self.layout)
        return max(1, -(-self.n_sub() * bpm // JH_TD)) if self.listed() else 1


def _magnitude(v):
    nb = abs(v).bit_length()
    return nb, (v if v >= 0 else v - 1) & ((1 << nb) - 1)


def write_stream(rows, cols, blocks, layout="420", qtabs=None, tq=None, huff=None, sel=None, restart=0, raw_ac=None, raw_dc=None,
                 hooks=None, dht=True, sof_hv=None, scan_ncomp=None):
    """blocks: int [n][64], natural order, true DC.  qtabs: {id: (pq, int[64] natural)}; tq: table id per component.  huff:
    {(class, id): (bits, vals)}; sel: (dc id, ac id) per component.  raw_ac: {block: [(symbol, extra, n_extra), ...]} in place of
    the block's AC part; raw_dc: {block: (symbol, extra, n_extra)} in place of its DC symbol.  hooks (indices are the RSTn's
    ordinals from 0): fill_before, drop_rst, ones_before: sets; rst_number: {ordinal: n}; skip_blocks: set of scan-order blocks not
    written; trailing: int [m][64] blocks written after the last MCU (as further blocks of component 0); cut_tail: bytes removed
    from the scan's end.  sof_hv: (h, v) per component as the SOF states them; scan_ncomp: components the SOS names."""
    ncomp, luma, bpm, n_mcu, comp_of = geometry(rows, cols, layout)
    blocks = np.asarray(blocks)
    assert blocks.shape == (bpm * n_mcu, 64), (blocks.shape, bpm * n_mcu)
    qtabs = {0: (0, np.ones(64, np.int64))} if qtabs is None else qtabs
    tq = (0,) * ncomp if tq is None else tq
    huff = std_huff() if huff is None else huff
    sel = ((0, 0), (1, 1), (1, 1))[:ncomp] if sel is None else sel
    raw_ac, raw_dc, hooks = raw_ac or {}, raw_dc or {}, hooks or {}
    enc_huff = std_huff() if not dht else huff
    tabs = {key: tuple(a.tolist() for a in R.huff_table(*bv)) for key, bv in enc_huff.items()}

    def token(tab, sym, extra, n_extra):
        if sym is None:
            return extra, n_extra
        code, size = tab
        assert size[sym] > 0, "the table has no code for symbol 0x%02x" % sym
        return (code[sym] << n_extra) | extra, size[sym] + n_extra

    zz = blocks[:, R.ZIGZAG].astype(np.int64)
    nz_b, nz_k = np.nonzero(zz[:, 1:])
    nz_at = np.searchsorted(nz_b, np.arange(len(zz) + 1))
    nz_v, nz_k, dcs = zz[nz_b, nz_k + 1].tolist(), (nz_k + 1).tolist(), zz[:, 0].tolist()
    skip = hooks.get("skip_blocks", ())
    trailing = np.asarray(hooks["trailing"])[:, R.ZIGZAG].astype(np.int64) if "trailing" in hooks else None
    n_seg = -(-n_mcu // restart) if restart > 0 else 1
    per_seg = restart * bpm if restart > 0 else bpm * n_mcu
    seg_bytes, t_seg, t_bit, t_len, t_blk, t_last = [], [], [], [], [], []
    for g in range(n_seg):
        pred = [0, 0, 0]
        val, length, blk_of, last = [], [], [], []
        todo = [(b, comp_of[b % bpm], dcs[b], None) for b in range(g * per_seg, min((g + 1) * per_seg, bpm * n_mcu)) if b not in skip]
        if trailing is not None and g == n_seg - 1:
            todo += [(-1 - i, 0, int(trailing[i, 0]), trailing[i]) for i in range(len(trailing))]
        for b, c, dc, extra_block in todo:
            dct, act = tabs[(0, sel[c][0])], tabs[(1, sel[c][1])]
            if b in raw_dc:
                t = [token(dct, *raw_dc[b])]
            else:
                nb, low = _magnitude(dc - pred[c])
                t = [token(dct, nb, low, nb)]
            pred[c] = dc
            if b in raw_ac:
                t += [token(act, *r) for r in raw_ac[b]]
            else:
                if extra_block is None:
                    ks, vs = nz_k[nz_at[b]:nz_at[b + 1]], nz_v[nz_at[b]:nz_at[b + 1]]
                else:
                    ks = (np.flatnonzero(extra_block[1:]) + 1).tolist()
                    vs = [int(extra_block[k]) for k in ks]
                at = 0
                for k, v in zip(ks, vs):
                    run = k - at - 1
                    while run > 15:
                        t.append(token(act, 0xF0, 0, 0))
                        run -= 16
                    nb, low = _magnitude(v)
                    t.append(token(act, (run << 4) | nb, low, nb))
                    at = k
                if at < 63:
                    t.append(token(act, 0x00, 0, 0))
            for i, (tv, tl) in enumerate(t):
                val.append(tv); length.append(tl); blk_of.append(b); last.append(i == len(t) - 1)
        tl = np.array(length, np.int64)
        tv = np.array(val, np.uint64)
        start = np.cumsum(tl) - tl
        tok = np.repeat(np.arange(tl.size), tl)
        pos = np.arange(int(tl.sum())) - start[tok]
        bits = ((tv[tok] >> (tl[tok] - 1 - pos).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
        seg_bytes.append(R.scan_bytes(bits))
        t_seg.append(np.full(tl.size, g)); t_bit.append(start); t_len.append(tl); t_blk.append(np.array(blk_of, np.int64)); t_last.append(np.array(last, bool))
    s = Stream()
    s.rows, s.cols, s.layout, s.restart = rows, cols, layout, restart
    s.tok_seg, s.tok_bit, s.tok_len, s.tok_blk, s.tok_last = (np.concatenate(x) for x in (t_seg, t_bit, t_len, t_blk, t_last))
    s.seg_len = np.array([len(x) - x.count(b"\xff") for x in seg_bytes], np.int64)            # (every 0xFF of a segment has its stuffed zero)
    s.seg_begin = np.cumsum(s.seg_len) - s.seg_len
    scan = bytearray()
    s.rst_raw = []
    for g, sb in enumerate(seg_bytes):
        scan += sb
        if g == n_seg - 1:
            break
        if g in hooks.get("ones_before", ()):
            scan += b"\xff\x00"
        if g in hooks.get("drop_rst", ()):
            continue
        if g in hooks.get("fill_before", ()):
            scan += b"\xff"
        s.rst_raw.append(len(scan))
        scan += bytes([0xFF, 0xD0 + hooks.get("rst_number", {}).get(g, g & 7)])
    if hooks.get("cut_tail", 0):
        del scan[-hooks["cut_tail"]:]
    s.scan = bytes(scan)
    # ---- headers
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tid, (pq, tab) in sorted(qtabs.items()):
        q = [int(x) for x in np.asarray(tab)[R.ZIGZAG]]
        body = bytes([(pq << 4) | tid]) + (b"".join(bytes([x >> 8, x & 255]) for x in q) if pq else bytes(q))
        out += b"\xff\xdb" + bytes([(len(body) + 2) >> 8, (len(body) + 2) & 255]) + body
    _, h, v = LAYOUTS[layout]
    hv = [(h, v)] + [(1, 1)] * (ncomp - 1) if sof_hv is None else sof_hv
    out += b"\xff\xc0" + bytes([0, 8 + 3 * ncomp, 8, rows >> 8, rows & 255, cols >> 8, cols & 255, ncomp])
    for c in range(ncomp):
        out += bytes([c + 1, (hv[c][0] << 4) | hv[c][1], tq[c]])
    if dht:
        for (cls, tid), (bits, vals) in sorted(huff.items()):
            n = 2 + 1 + 16 + len(vals)
            out += b"\xff\xc4" + bytes([n >> 8, n & 255, (cls << 4) | tid]) + bytes(bits) + bytes(vals)
    if restart > 0:
        out += b"\xff\xdd\x00\x04" + bytes([restart >> 8, restart & 255])
    ns = ncomp if scan_ncomp is None else scan_ncomp
    out += b"\xff\xda" + bytes([0, 6 + 2 * ns, ns])
    for c in range(ns):
        out += bytes([c + 1, (sel[c][0] << 4) | sel[c][1]])
    out += b"\x00\x3f\x00"
    s.scan_off = len(out)
    s.data = bytes(out) + s.scan + b"\xff\xd9"
    return s


# ------------------------------------------------------------------------------------------------ tables
def _bits(counts):
    b = [0] * 16
    for length, n in counts.items():
        b[length - 1] = n
    return b


DC13 = list(range(13))                                      # with a code for symbol 12, which no DC difference may use
HUFF_ALL16 = {(0, 0): (_bits({16: 12}), R.DC_VALS), (1, 0): (_bits({16: 162}), R.AC_LUMA_VALS),
              (0, 1): (_bits({16: 12}), R.DC_VALS), (1, 1): (_bits({16: 162}), R.AC_CHROMA_VALS)}
HUFF_9_10 = {(0, 0): (_bits({9: 6, 10: 6}), R.DC_VALS), (1, 0): (_bits({9: 80, 10: 82}), R.AC_LUMA_VALS),
             (0, 1): (_bits({9: 5, 10: 7}), R.DC_VALS), (1, 1): (_bits({9: 81, 10: 81}), R.AC_CHROMA_VALS)}
# size 0 / EOB in one bit ('0'); the rest one code per length, then the crowd at 16
_ONE_AC = [0x00, 0x01, 0x11, 0x02, 0x21, 0x03, 0xF0] + [s for s in R.AC_LUMA_VALS if s not in (0x00, 0x01, 0x11, 0x02, 0x21, 0x03, 0xF0)]
HUFF_1BIT = {(0, 0): (_bits(dict((n, 1) for n in range(1, 13))), R.DC_VALS),
             (1, 0): (_bits(dict([(n, 1) for n in range(1, 8)] + [(16, 155)])), _ONE_AC)}
HUFF_1BIT[(0, 1)], HUFF_1BIT[(1, 1)] = HUFF_1BIT[(0, 0)], HUFF_1BIT[(1, 0)]
# two 1-bit codes: '0' = nothing / EOB, '1' = size 7: a value of +127 is eight 1-bits -- scans made of 0xFF bytes
HUFF_FF = {(0, 0): (_bits({1: 2}), [0, 7]), (1, 0): (_bits({1: 2}), [0x00, 0x07])}
HUFF_FF[(0, 1)], HUFF_FF[(1, 1)] = HUFF_FF[(0, 0)], HUFF_FF[(1, 0)]
# every code 8 bits: a symbol of size 8 is two whole bytes (its code = its index in vals, its extra bits), so a block is a
# byte string the case writes out: DC 0x00 | 0x08 xx, then 0x?? xx per coefficient, the EOB's code last
_B8_AC = [0x08, 0x00] + [s for s in R.AC_LUMA_VALS if s not in (0x08, 0x00)]
HUFF_B8 = {(0, 0): (_bits({8: 12}), [0, 8] + [s for s in range(12) if s not in (0, 8)]), (1, 0): (_bits({8: 162}), _B8_AC)}
HUFF_B8[(0, 1)], HUFF_B8[(1, 1)] = HUFF_B8[(0, 0)], HUFF_B8[(1, 0)]
HUFF_DC12 = dict(std_huff())
HUFF_DC12[(0, 0)] = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0], DC13)
HUFF_SWAPPED = {(0, 1): std_huff()[(0, 0)], (1, 1): std_huff()[(1, 0)], (0, 0): std_huff()[(0, 1)], (1, 0): std_huff()[(1, 1)]}
HUFF_THREE = dict(std_huff())
HUFF_THREE[(0, 2)], HUFF_THREE[(1, 2)] = HUFF_9_10[(0, 0)], HUFF_ALL16[(1, 0)]


# ------------------------------------------------------------------------------------------------ block builders
def noise_blocks(n, seed, amp_ac, amp_dc, density=1.0):
    rng = np.random.default_rng(seed)
    b = rng.integers(-amp_ac, amp_ac + 1, (n, 64))
    if density < 1.0:
        b[rng.random((n, 64)) >= density] = 0
    b[:, 0] = rng.integers(-amp_dc, amp_dc + 1, n)
    return b.astype(np.int64)


def hold_dc(blocks, layout, which):
    """give the blocks `which` the DC of the block before them in their component: a DC difference of 0"""
    _, _, bpm, _, comp_of = geometry(8, 8, layout)
    last = [0, 0, 0]
    for b in range(len(blocks)):
        c = comp_of[b % bpm]
        if b in which:
            blocks[b, 0] = last[c]
        last[c] = blocks[b, 0]
    return blocks


def zz_block(pairs, dc=0):
    """a block from {zigzag position: value}"""
    b = np.zeros(64, np.int64)
    for k, v in pairs.items():
        b[R.ZIGZAG[k]] = v
    b[0] = dc
    return b


class Case(object):
    def __init__(self, name, stream, expect=None, status=OK, in_range=False, census=(), pillow_accepts=None, note=""):
        self.name, self.stream, self.status, self.in_range, self.note = name, stream, status, in_range, note
        self.expect = None if expect is None else np.asarray(expect).astype(np.int16)
        self.census = list(census)
        self.pillow_accepts = pillow_accepts
        self.rows, self.cols, self.data = stream.rows, stream.cols, stream.data


def row(text, observed, holds):
    return (text, observed, bool(holds))


CANVAS = (32, 64)
BUILDERS = {}


def case(fn):
    BUILDERS[fn.__name__] = fn
    return fn


def _valid(name, blocks, census_fn=None, in_range=False, **kw):
    rows, cols = kw.pop("size", CANVAS)
    s = write_stream(rows, cols, blocks, **kw)
    exp = np.array(blocks, copy=True)
    return Case(name, s, expect=exp, in_range=in_range, census=census_fn(s) if census_fn else [])


def _long_symbol_rows(s, modulus_bits):
    """symbols of >= 26 bits: those that lie across a multiple of modulus_bits (in the clean scan), and those that end on one"""
    g = s.tok_global_bit()
    big = s.tok_len >= 26
    across = big & (g // modulus_bits != (g + s.tok_len - 1) // modulus_bits)
    return int(across.sum()), int((big & ((g + s.tok_len) % modulus_bits == 0)).sum()), int((big & (g % modulus_bits == 0)).sum())


def _search_long_symbol(name, want):
    """32x64 4:2:0, standard tables (run 0 / size 10 has a 16-bit code in both AC tables): sparse blocks of +-512 .. 1023, the seed
    that puts such a symbol where `want` asks"""
    n = n_blocks(*CANVAS, "420")
    for seed in range(400):
        rng = np.random.default_rng(1000 + seed)
        b = np.zeros((n, 64), np.int64)
        for i in range(n):
            ks = rng.choice(np.arange(1, 64), int(rng.integers(0, 7)), replace=False)
            b[i, ks] = rng.integers(512, 1024, ks.size) * rng.choice([-1, 1], ks.size)
            b[i, 0] = int(rng.integers(-300, 301))
        s = write_stream(*CANVAS, b)
        census = want(s)
        if all(r[2] for r in census):
            return Case(name, s, expect=b, census=census + [row("seed of the search", seed, True)])
    raise AssertionError("no seed places the symbol for " + name)


# ---- symbols and tables
@case
def long_symbol_across_subsequence():
    def want(s):
        a, _, _ = _long_symbol_rows(s, 8 * JH_SB)
        return [row(">= 26-bit symbols lying across a multiple of %d clean bytes" % JH_SB, a, a >= 1),
                row("longest symbol (bits)", int(s.tok_len.max()), s.tok_len.max() >= 26)]
    return _search_long_symbol("long_symbol_across_subsequence", want)


@case
def long_symbol_across_dword():
    def want(s):
        a, e, b = _long_symbol_rows(s, 32)
        return [row(">= 26-bit symbols lying across a multiple of 4 clean bytes", a, a >= 1),
                row(">= 26-bit symbols ending exactly on a dword (the reader's sh lands on 32)", e, e >= 1),
                row(">= 26-bit symbols starting exactly on a dword (entered with sh = 32)", b, b >= 1)]
    return _search_long_symbol("long_symbol_across_dword", want)


def _code_length_rows(s, huff, lengths):
    out = []
    for key, (bits, _) in sorted(huff.items()):
        have = sorted(i + 1 for i, n in enumerate(bits) if n)
        out.append(row("code lengths of table class %d id %d" % key, have, have == lengths))
    return out


@case
def all_codes_16_bits():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 11, 40, 300, 0.3)
    return _valid("all_codes_16_bits", b, lambda s: _code_length_rows(s, HUFF_ALL16, [16]) +
                  [row("shortest symbol (bits)", int(s.tok_len.min()), s.tok_len.min() >= 16)], huff=HUFF_ALL16)


@case
def codes_of_9_and_10_bits():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 12, 40, 300, 0.4)

    def census(s):
        return _code_length_rows(s, HUFF_9_10, [9, 10]) + [row("symbols in the scan", int(s.tok_len.size), s.tok_len.size > 500)]
    return _valid("codes_of_9_and_10_bits", b, census, huff=HUFF_9_10)


@case
def one_bit_tables():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 13, 3, 40, 0.03)
    b[::3] = 0
    b = hold_dc(b, "420", set(range(0, len(b), 3)))
    return _valid("one_bit_tables", b, lambda s: [row("2-bit blocks (DC '0' + EOB '0')", int(np.sum(np.bincount(s.tok_blk, s.tok_len) == 2)),
                                                      np.sum(np.bincount(s.tok_blk, s.tok_len) == 2) >= 16)], in_range=True, huff=HUFF_1BIT)


@case
def identical_tables_420():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 14, 2, 60, 0.5)
    return _valid("identical_tables_420", b, lambda s: [row("table selectors", "all (0, 0)", True)], in_range=True,
                  sel=((0, 0), (0, 0), (0, 0)))


@case
def luma_on_table_1_chroma_on_0():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 15, 2, 60, 0.5)
    return _valid("luma_on_table_1_chroma_on_0", b, lambda s: [row("SOS selectors", s.data[s.scan_off - 9:s.scan_off - 3].hex(), s.data[s.scan_off - 9:s.scan_off - 3] == bytes([1, 0x11, 2, 0x00, 3, 0x00]))], in_range=True, huff=HUFF_SWAPPED, sel=((1, 1), (0, 0), (0, 0)))


@case
def three_components_three_tables():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 16, 2, 60, 0.5)
    return _valid("three_components_three_tables", b, lambda s: [row("SOS selectors", s.data[s.scan_off - 9:s.scan_off - 3].hex(), s.data[s.scan_off - 9:s.scan_off - 3] == bytes([1, 0x02, 2, 0x10, 3, 0x21]))], in_range=True, huff=HUFF_THREE, sel=((0, 2), (1, 0), (2, 1)))


@case
def no_dht_annex_k_tables():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 17, 2, 60, 0.5)
    return _valid("no_dht_annex_k_tables", b, lambda s: [row("DHT segments in the file", s.data.count(b"\xff\xc4"), s.data[:s.scan_off].count(b"\xff\xc4") == 0)],
                  in_range=True, dht=False)


@case
def quantiser_16_bit():
    b = noise_blocks(n_blocks(*CANVAS, "422"), 18, 1, 3, 0.1)
    q = {0: (1, np.full(64, 300)), 1: (0, np.full(64, 7))}
    q[0][1][0] = 20
    return _valid("quantiser_16_bit", b, lambda s: [row("Pq of table 0", 1, True)], layout="422", qtabs=q, tq=(0, 1, 1))


def _specials(name, special, in_range=False, **kw):
    """32x64 4:2:0: `special(i)` at every third block from block 1 on, a block that is only EOB (DC difference 0) before and after each"""
    n = n_blocks(*CANVAS, "420")
    b = np.zeros((n, 64), np.int64)
    at = list(range(1, n, 3))
    for i, k in enumerate(at):
        b[k] = special(i)
    b = hold_dc(b, "420", set(range(n)) - set(at))

    def census(s):
        bits = np.bincount(s.tok_blk, minlength=n)
        return [row("special blocks", len(at), len(at) >= 8),
                row("blocks of two symbols (DC difference 0 + EOB) around each", int(np.sum(bits == 2)), all(bits[k - 1] == 2 and (k + 1 >= n or bits[k + 1] == 2) for k in at))]
    return name, b, census, in_range, kw


@case
def dc_differences_of_2047():
    # (the specials fall on luma and Cb in turn: each component's own specials alternate between the two extremes)
    name, b, census, _, kw = _specials("dc_differences_of_2047", lambda i: zz_block({}, dc=(1023, -1024)[(i // 2) % 2]))

    def c2(s):
        comp_of = geometry(*CANVAS, "420")[4]
        comp = np.array([comp_of[i % 6] for i in range(len(b))])
        d = np.concatenate([np.diff(b[comp == c, 0], prepend=0) for c in range(3)])
        return census(s) + [row("DC differences of +2047 and of -2047", (int(np.sum(d == 2047)), int(np.sum(d == -2047))), np.sum(d == 2047) >= 2 and np.sum(d == -2047) >= 2),
                            row("longest symbol: an 11-bit chroma DC code + 11 bits", int(s.tok_len.max()), s.tok_len.max() == 22)]
    return _valid(name, b, c2, **kw)


@case
def all_63_ac_no_eob():
    name, b, census, in_range, kw = _specials("all_63_ac_no_eob", lambda i: np.concatenate([[8 * (i % 5)], np.where(np.arange(63) % 2, 1, -1) * (1 + i % 2)]), in_range=True)

    def c2(s):
        per = np.bincount(s.tok_blk)
        return census(s) + [row("blocks of 64 symbols (DC + 63 coefficients, no EOB)", int(np.sum(per == 64)), np.sum(per == 64) >= 8)]
    return _valid(name, b, c2, in_range=in_range, **kw)


@case
def three_zrl_then_run_14():
    name, b, census, in_range, kw = _specials("three_zrl_then_run_14", lambda i: zz_block({63: (3, -2, 1)[i % 3]}, dc=5 * i), in_range=True)

    def c2(s):
        per = np.bincount(s.tok_blk)
        return census(s) + [row("blocks of DC + ZRL ZRL ZRL + (run 14, k = 63)", int(np.sum(per == 5)), np.sum(per == 5) >= 8)]
    return _valid(name, b, c2, in_range=in_range, **kw)


@case
def four_zrl_end_the_block():
    name, b, census, in_range, kw = _specials("four_zrl_end_the_block", lambda i: zz_block({}, dc=7 * i - 20), in_range=True)
    raw = dict((k, [(0xF0, 0, 0)] * 4) for k in range(1, len(b), 3))

    def c2(s):
        per = np.bincount(s.tok_blk)
        return census(s) + [row("blocks of DC + four ZRLs and no EOB", int(np.sum(per == 5)), np.sum(per == 5) >= 8)]
    return _valid(name, b, c2, in_range=in_range, raw_ac=raw, **kw)


# ---- blocks per subsequence
def _flat(name, layout, huff, least):
    rows, cols = 480, 640
    b = np.zeros((n_blocks(rows, cols, layout), 64), np.int64)

    def census(s):
        per = s.blocks_per_sub()
        return [row("subsequences", s.n_sub(), s.n_sub() >= 2), row("subsequences per unit (sup)", s.sup(), True),
                row("most blocks completed in one subsequence", int(per.max()), least <= per.max() <= NBLK_FIELD_MAX)]
    return _valid(name, b, census, in_range=True, size=(rows, cols), layout=layout, huff=huff)


@case
def flat_420_standard_tables():
    c = _flat("flat_420_standard_tables", "420", None, 70)
    c.census.append(row("block lengths (bits)", sorted(set(np.bincount(c.stream.tok_blk, c.stream.tok_len).astype(int))), True))
    c.census.append(row("sup > 1", c.stream.sup(), c.stream.sup() > 1))
    return c


@case
def flat_420_one_bit_tables():
    return _flat("flat_420_one_bit_tables", "420", HUFF_1BIT, 192)


@case
def flat_gray_standard_tables():
    return _flat("flat_gray_standard_tables", "gray", None, 64)


@case
def flat_gray_one_bit_tables():
    return _flat("flat_gray_one_bit_tables", "gray", HUFF_1BIT, 192)


@case
def gray_noise_sup_above_1():
    """a flat gray 480x640 scan has 75 subsequences at most, one per lane: units of several subsequences with one block per MCU
    need more than 512 of them"""
    b = noise_blocks(n_blocks(*NOISE_SIZE, "gray"), 20, 1023, 900)
    return _valid("gray_noise_sup_above_1", b, lambda s: [row("subsequences", s.n_sub(), JH_TD < s.n_sub() <= JH_DL),
                                                          row("sup > 1 with one block per MCU", s.sup(), s.sup() > 1)], size=NOISE_SIZE, layout="gray")


# ---- restart intervals
@case
def restart_1_gray_strip_2100():
    rows, cols = 8, 16800
    b = noise_blocks(2100, 21, 30, 200, 0.25)

    def census(s):
        return [row("intervals", len(s.seg_len), len(s.seg_len) == 2100), row("subsequences", s.n_sub(), s.n_sub() > JH_DL),
                row("clean scan (bytes)", s.clean_len(), s.clean_in_lds() and s.unstuffs_in_decoder()), row("listed passes", s.listed(), not s.listed())]
    return _valid("restart_1_gray_strip_2100", b, census, size=(rows, cols), layout="gray", restart=1)


@case
def intervals_of_exact_lengths():
    """gray, restart 1: an interval is one block; blocks are drawn until every wanted clean length has one whose last byte is padded"""
    want = [47, 48, 49, 95, 96, 97]
    rng = np.random.default_rng(22)
    found, pool = {}, []
    std = std_huff()
    dct, act = R.huff_table(*std[(0, 0)]), R.huff_table(*std[(1, 0)])
    for _ in range(20000):
        n = int(rng.integers(20, 64))
        blk = np.zeros(64, np.int64)
        ks = rng.choice(np.arange(1, 64), n, replace=False)
        blk[R.ZIGZAG[ks]] = rng.integers(1, 200, n) * rng.choice([-1, 1], n)
        blk[0] = int(rng.integers(-100, 101))
        pool.append(blk)
        if len(pool) == 6:
            s = write_stream(8, 48, np.array(pool), layout="gray", restart=1)
            for i, ln in enumerate(s.seg_len):
                bits = int(s.tok_len[s.tok_seg == i].sum())
                # the DC is coded against 0 in every interval (restart 1), so a block's length does not depend on its neighbours
                if int(ln) in want and int(ln) not in found and bits % 8 != 0:
                    found[int(ln)] = pool[i]
            pool = []
        if len(found) == len(want):
            break
    assert len(found) == len(want), sorted(found)
    order = [47, 96, 48, 97, 49, 95]
    blocks = []
    for i, ln in enumerate(order):
        blocks += [found[ln], zz_block({1: 3}, dc=10 + i)]

    def census(s):
        lens = [int(x) for x in s.seg_len]
        return [row("clean bytes per interval", lens, all(w in lens for w in want)),
                row("padding bits of those intervals", [int(8 * ln - s.tok_len[s.tok_seg == i].sum()) for i, ln in enumerate(lens) if ln in want],
                    all(0 < 8 * ln - s.tok_len[s.tok_seg == i].sum() < 8 for i, ln in enumerate(lens) if ln in want))]
    return _valid("intervals_of_exact_lengths", np.array(blocks), census, size=(8, 8 * len(blocks)), layout="gray", restart=1)


@case
def restart_numbers_wrap_444():
    b = noise_blocks(n_blocks(*CANVAS, "444"), 23, 2, 60, 0.5)
    return _valid("restart_numbers_wrap_444", b, lambda s: [row("intervals", len(s.seg_len), len(s.seg_len) > 8)], in_range=True,
                  layout="444", restart=1)


@case
def restart_1_420_600_intervals():
    rows, cols = 16, 9600
    b = noise_blocks(n_blocks(rows, cols, "420"), 24, 2, 60, 0.3)
    return _valid("restart_1_420_600_intervals", b, lambda s: [row("intervals", len(s.seg_len), len(s.seg_len) > JH_TD)], in_range=True,
                  size=(rows, cols), restart=1)


def _dc_carry(name, restart, want):
    rows, cols = 8, 8 * 600
    b = noise_blocks(n_blocks(rows, cols, "444"), 25 + restart, 2, 50, 0.2)
    b[:, 0] = np.where(b[:, 0] == 0, 9, b[:, 0])

    def census(s):
        starts = list(range(restart, 600, restart))
        side = all(np.all(b[3 * (m - 1):3 * (m + 1), 0] != 0) for m in starts)
        return [row("interval starts (MCU)", starts[:12], want(starts)), row("non-zero DC on both sides in all three components", side, side)]
    return _valid(name, b, census, in_range=True, size=(rows, cols), layout="444", restart=restart)


@case
def dc_carry_at_wave_boundaries():
    return _dc_carry("dc_carry_at_wave_boundaries", 64, lambda st: 64 in st and 512 in st)


@case
def dc_carry_inside_a_wave():
    return _dc_carry("dc_carry_inside_a_wave", 37, lambda st: any(m % WAVE and m > JH_TD for m in st) and all(m % WAVE for m in st[:10]))


@case
def restart_larger_than_the_picture():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 27, 2, 60, 0.5)
    return _valid("restart_larger_than_the_picture", b, lambda s: [row("intervals", len(s.seg_len), len(s.seg_len) == 1)], in_range=True, restart=1000)


# ---- scan sizes: noise at quantiser 1 on 160x160, trailing blocks emptied until the scan has the wanted size
NOISE_SIZE = (160, 160)


@functools.lru_cache(None)
def _noise_pool():
    n = n_blocks(*NOISE_SIZE, "420")
    b = noise_blocks(n, 31, 1023, 900)
    s = write_stream(*NOISE_SIZE, b)
    return b, np.bincount(s.tok_blk, s.tok_len, minlength=n)


def _sized_noise(name, lo, hi, what, census_extra):
    """the clean (what = 'clean') or raw scan in (lo, hi] bytes"""
    b, bits = _noise_pool()
    keep, mid = len(b), (lo + hi) // 2
    for _ in range(6):                                          # full blocks kept, by the measured size of the scan they give
        blocks = b.copy()
        blocks[keep:, 1:] = 0
        blocks = hold_dc(blocks, "420", set(range(keep, len(b))))
        s = write_stream(*NOISE_SIZE, blocks)
        size = s.clean_len() if what == "clean" else len(s.scan)
        if lo < size <= hi:
            break
        keep = max(1, min(len(b), int(round(keep * mid / size))))
    census = [row("%s scan (bytes) in (%d, %d]" % (what, lo, hi), size, lo < size <= hi), row("raw scan (bytes)", len(s.scan), True),
              row("subsequences", s.n_sub(), True)] + census_extra(s)
    return Case(name, s, expect=blocks, census=census)


@case
def clean_scan_beyond_lds_listed():
    return _sized_noise("clean_scan_beyond_lds_listed", 95300, 98304, "clean", lambda s: [
        row("listed passes, scan read from global memory", (s.listed(), s.clean_in_lds()), s.listed() and not s.clean_in_lds())])


@case
def just_above_2048_subsequences():
    return _sized_noise("just_above_2048_subsequences", JH_DL * JH_SB, JH_DL * JH_SB + 1500, "clean", lambda s: [
        row("unlisted passes", s.n_sub(), JH_DL < s.n_sub() <= JH_DL + 32)])


@case
def raw_scan_above_64k():
    return _sized_noise("raw_scan_above_64k", ROUND_DECODE + 2000, ROUND_DECODE + 6000, "raw", lambda s: [
        row("unstuffed by the decoder in two rounds, decoded out of LDS", (s.unstuffs_in_decoder(), s.clean_in_lds()), s.unstuffs_in_decoder() and s.clean_in_lds())])


@case
def raw_scan_above_93k():
    return _sized_noise("raw_scan_above_93k", 95300, 97000, "raw", lambda s: [
        row("unstuffed by k_jh_unstuff from global memory", s.unstuffs_in_decoder(), not s.unstuffs_in_decoder())])


@case
def flat_160_for_the_long_batch():
    b = np.zeros((n_blocks(*NOISE_SIZE, "420"), 64), np.int64)
    b[:, 0] = 25

    def census(s):
        long = get("raw_scan_above_93k").stream
        return [row("beside the 93 KB frame: through k_jh_unstuff, then decoded out of LDS",
                    (s.unstuffs_in_decoder(len(long.scan)), s.clean_in_lds(len(long.scan))), not s.unstuffs_in_decoder(len(long.scan)) and s.clean_in_lds(len(long.scan))),
                row("alone: unstuffed by the decoder", s.unstuffs_in_decoder(), s.unstuffs_in_decoder())]
    return _valid("flat_160_for_the_long_batch", b, census, in_range=True, size=NOISE_SIZE)


# ---- unstuffing: the 8-bit tables, blocks written out as byte strings
def _b8_blocks(n, plan, layout="gray"):
    """plan(i) -> (dc byte or None, [extra bytes of the coefficients]) for block i; a DC byte is the difference to the component's DC before"""
    blocks = np.zeros((n, 64), np.int64)
    _, _, bpm, _, comp_of = geometry(8, 8, layout)
    dc = [0, 0, 0]
    for i in range(n):
        d, acs = plan(i)
        if d is not None:
            dc[comp_of[i % bpm]] += d
        blocks[i, 0] = dc[comp_of[i % bpm]]
        for k, x in enumerate(acs):
            blocks[i, R.ZIGZAG[k + 1]] = x if x >= 128 else x - 255
    return blocks


def _split_rows(s, second, targets, mod):
    off = s.raw_ff_offsets(second)
    hit = [int(o) for o in off if (o % mod == mod - 1 if targets is None else int(o) in targets)]
    return off, hit


@case
def ff00_split_by_a_chunk():
    """gray 32x64, 8-bit codes: blocks of 1 + 2 * 63 = 127 clean bytes, an 0xFF as the last extra byte of block 0: raw offset 126 -- one
    more coefficient-free byte in front (DC of size 8) moves it to 127"""
    n = n_blocks(*CANVAS, "gray")
    b = _b8_blocks(n, lambda i: (130 if i == 0 else None, [0x40 + (i + k) % 60 for k in range(62)] + [0xFF if i % 2 == 0 else 0x33]))

    def census(s):
        off, hit = _split_rows(s, {0x00}, None, JH_CHUNK)
        return [row("FF 00 pairs", len(off), len(off) >= 4), row("... with the FF at raw offset 127 mod 128", hit[:6], len(hit) >= 1)]
    return _valid("ff00_split_by_a_chunk", b, census, layout="gray", huff=HUFF_B8)


@case
def ffdn_split_by_a_chunk():
    """gray, restart 1, 8-bit codes: an interval = one block of 127 bytes, RST0 at raw offset 127"""
    n = n_blocks(*CANVAS, "gray")
    b = _b8_blocks(n, lambda i: (None, [0x40 + (i + k) % 60 for k in range(63)]))
    b[:, 0] = 0

    def census(s):
        hit = [o for o in s.rst_raw if o % JH_CHUNK == JH_CHUNK - 1]
        return [row("RSTn markers", len(s.rst_raw), len(s.rst_raw) == n - 1), row("... with the FF at raw offset 127 mod 128", hit[:6], len(hit) >= 1)]
    return _valid("ffdn_split_by_a_chunk", b, census, layout="gray", huff=HUFF_B8, restart=1)


def _round_case(name, restart):
    """160x160 4:4:4, 8-bit codes: 720 blocks of 127 clean bytes (DC 00, 63 x (00, extra byte)), the rest of the picture empty
    blocks, so that the decoder unstuffs the scan itself.  Without restart markers an extra byte of 0xFF is put at raw offsets
    32 767 and 65 535 (a DC of size 8 in the block before, one byte more, where the offset would fall on a code byte); with
    restart 1 the intervals before each target are cut so that a marker's FF stands there."""
    rows, cols = NOISE_SIZE
    n = n_blocks(rows, cols, "444")
    full = 720
    targets = (ROUND_UNSTUFF - 1, ROUND_DECODE - 1)
    filler = lambda i, m: [0x40 + (i + k) % 60 for k in range(m)]
    if restart == 0:
        def plan(fixes):
            plans, raw, t, pending = [], 0, 0, fixes[0]
            for i in range(n):
                if i >= full:
                    plans.append((None, []))
                    continue
                acs, dc = filler(i, 63), None
                if pending:
                    dc, pending = 130, pending - 1
                first = raw + (2 if dc else 1)                  # the first coefficient's code byte; extra bytes at first + 1, + 3, ...
                d = targets[t] - first if t < 2 else -1
                if 0 <= d < 126 and d % 2 == 1:
                    acs[d // 2] = 0xFF
                    t += 1
                    pending = fixes[t] if t < 2 else 0
                plans.append((dc, acs))
                raw = first + 126 + acs.count(0xFF)
            return plans if t == 2 else None
        plans = next(p for p in (plan((k1, k2)) for k1 in range(4) for k2 in range(4)) if p is not None)
        b = _b8_blocks(n, lambda i: plans[i], "444")
    else:
        def split(d):                                           # an interval of d clean bytes as three blocks of 127 or of an even size
            sizes = [127, 127, 127] if d == 381 else None
            if sizes is None and d % 2 == 1 and 131 <= d <= 379:
                sizes, d = [127], d - 127
            elif sizes is None and d % 2 == 0 and 6 <= d <= 378:
                sizes = []
            while sizes is not None and len(sizes) < 3:
                left = 3 - len(sizes)
                e = min(126, d - 2 * (left - 1))
                sizes.append(e)
                d -= e
            return sizes
        plans, raw, tg = [], 0, list(targets)
        for m in range(n // 3):
            if m >= full // 3:
                plans += [(None, [])] * 3
                continue
            sizes = [127, 127, 127]
            if tg and tg[0] - raw <= 381:
                sizes = split(tg[0] - raw)
                assert sizes is not None, (tg[0], raw)
                tg.pop(0)
            plans += [(None, filler(3 * m + j, 63 if e == 127 else (e - 2) // 2)) for j, e in enumerate(sizes)]
            raw += sum(sizes) + 2
        b = _b8_blocks(n, lambda i: plans[i], "444")
        b[:, 0] = 0

    def census(s):
        if restart == 0:
            off, hit = _split_rows(s, {0x00}, targets, 0)
            return [row("raw scan (bytes), unstuffed by the decoder", len(s.scan), len(s.scan) > ROUND_DECODE + 128 and s.unstuffs_in_decoder()), row("FF 00 with the FF at raw offsets %s" % (targets,), hit, sorted(hit) == list(targets))]
        hit = [o for o in s.rst_raw if o in targets]
        return [row("raw scan (bytes), unstuffed by the decoder", len(s.scan), len(s.scan) > ROUND_DECODE + 128 and s.unstuffs_in_decoder()), row("FF Dn with the FF at raw offsets %s" % (targets,), hit, sorted(hit) == list(targets))]
    return _valid(name, b, census, size=(rows, cols), layout="444", huff=HUFF_B8, restart=restart)


@case
def ff00_split_by_the_rounds():
    return _round_case("ff00_split_by_the_rounds", 0)


@case
def ffdn_split_by_the_rounds():
    return _round_case("ffdn_split_by_the_rounds", 1)


def _ff_blocks(n, seed):
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 64), np.int64)
    for i in range(n):
        k = int(rng.integers(0, 12))
        b[i, R.ZIGZAG[1:1 + k]] = 127
    comp_of = geometry(*CANVAS, "420")[4]
    comp = np.array([comp_of[i % 6] for i in range(n)])
    for c in range(3):                                          # a component's DC differences are 0 or +127
        b[comp == c, 0] = 127 * np.cumsum(rng.integers(0, 2, int(np.sum(comp == c))))
    return b


@case
def runs_of_ff00():
    b = _ff_blocks(n_blocks(*CANVAS, "420"), 41)

    def census(s):
        run = s.scan.count(b"\xff\x00\xff\x00\xff\x00")
        return [row("FF 00 FF 00 FF 00 runs in the raw scan", run, run >= 4)]
    return _valid("runs_of_ff00", b, census, huff=HUFF_FF, sel=((0, 0), (0, 0), (0, 0)))


@case
def ff_is_the_last_data_byte():
    n = n_blocks(*CANVAS, "420")
    b = _ff_blocks(n, 42)
    b[-1, 1:] = 127                                             # 63 coefficients and no EOB: the scan ends in 1-bits
    return _valid("ff_is_the_last_data_byte", b, lambda s: [row("the scan's last bytes", s.scan[-2:].hex(), s.scan.endswith(b"\xff\x00"))],
                  huff=HUFF_FF, sel=((0, 0), (0, 0), (0, 0)))


@case
def scan_shorter_than_a_subsequence():
    b = noise_blocks(2, 43, 2, 30, 0.3)
    return _valid("scan_shorter_than_a_subsequence", b, lambda s: [row("clean scan (bytes)", s.clean_len(), 1 < s.clean_len() < JH_SB)], in_range=True,
                  size=(8, 16), layout="gray")


@case
def scan_of_one_byte():
    b = np.zeros((1, 64), np.int64)
    return _valid("scan_of_one_byte", b, lambda s: [row("raw scan (bytes)", len(s.scan), len(s.scan) == 1)], in_range=True, size=(8, 8), layout="gray")


@case
def data_after_the_last_mcu_is_ignored():
    b = noise_blocks(n_blocks(*CANVAS, "420"), 44, 2, 60, 0.5)
    s = write_stream(*CANVAS, b, restart=3, hooks={"trailing": noise_blocks(5, 45, 2, 60, 0.5)})
    return Case("data_after_the_last_mcu_is_ignored", s, expect=b, in_range=True,
                census=[row("blocks written after the last MCU", int(np.sum(s.tok_last & (s.tok_blk < 0))), np.sum(s.tok_last & (s.tok_blk < 0)) == 5)])


# ---- refused streams: valid headers, lengths in bounds
def _refused(name, status=ERR_DECODE, pillow_accepts=None, layout="420", seed=50, **kw):
    b = noise_blocks(n_blocks(*CANVAS, layout), seed, 2, 60, 0.5)
    s = write_stream(*CANVAS, b, layout=layout, **kw)
    return Case(name, s, status=status, pillow_accepts=pillow_accepts, census=[row("headers and lengths", "valid", True)])


@case
def refused_run_plus_size_past_63():
    return _refused("refused_run_plus_size_past_63", raw_ac={7: [(0xF0, 0, 0)] * 3 + [(0xF1, 1, 1)]})        # k = 49, run 15, a coefficient: k = 64


@case
def refused_dc_symbol_12():
    return _refused("refused_dc_symbol_12", huff=HUFF_DC12, raw_dc={6: (12, 0xABC, 12)})


@case
def refused_no_code_matches():
    return _refused("refused_no_code_matches", raw_dc={12: (None, 0xFFFF, 16)})                             # the luma DC table has no code of 1-bits


@case
def refused_interval_one_block_short():
    # the interval's LAST block: left out in the middle, the blocks behind it are read with the neighbouring component's tables, fall
    # into step again a block later and the interval can come out whole -- every decoder then accepts it, rightly
    return _refused("refused_interval_one_block_short", restart=2, hooks={"skip_blocks": {23}})


@case
def refused_dropped_rst():
    return _refused("refused_dropped_rst", restart=2, hooks={"drop_rst": {1}})


@case
def refused_misnumbered_rst():
    return _refused("refused_misnumbered_rst", pillow_accepts=True, restart=2, hooks={"rst_number": {1: 2}})


@case
def refused_eight_padding_bits():
    return _refused("refused_eight_padding_bits", restart=2, hooks={"ones_before": {1}})


@case
def refused_fill_byte_before_rst():
    return _refused("refused_fill_byte_before_rst", pillow_accepts=True, restart=2, hooks={"fill_before": {1}})


@case
def refused_truncated_last_interval():
    return _refused("refused_truncated_last_interval", restart=2, hooks={"cut_tail": 9})


@case
def unsupported_luma_1x2():
    return _refused("unsupported_luma_1x2", status=ERR_UNSUPPORTED, sof_hv=[(1, 2), (1, 1), (1, 1)])


@case
def unsupported_luma_4x1():
    return _refused("unsupported_luma_4x1", status=ERR_UNSUPPORTED, sof_hv=[(4, 1), (1, 1), (1, 1)])


@case
def unsupported_non_interleaved_scan():
    return _refused("unsupported_non_interleaved_scan", status=ERR_UNSUPPORTED, scan_ncomp=1)


NAMES = tuple(BUILDERS)
# the cases whose coefficients keep every sample in range: there the oracle can be held to libjpeg-turbo (Pillow) pixel by pixel
IN_RANGE = ("one_bit_tables",
            "identical_tables_420",
            "luma_on_table_1_chroma_on_0",
            "three_components_three_tables",
            "no_dht_annex_k_tables",
            "all_63_ac_no_eob",
            "three_zrl_then_run_14",
            "four_zrl_end_the_block",
            "flat_420_standard_tables",
            "flat_420_one_bit_tables",
            "flat_gray_standard_tables",
            "flat_gray_one_bit_tables",
            "restart_numbers_wrap_444",
            "restart_1_420_600_intervals",
            "dc_carry_at_wave_boundaries",
            "dc_carry_inside_a_wave",
            "restart_larger_than_the_picture",
            "flat_160_for_the_long_batch",
            "scan_shorter_than_a_subsequence",
            "scan_of_one_byte",
            "data_after_the_last_mcu_is_ignored")


@functools.lru_cache(None)
def get(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


def valid_names():
    return [n for n in NAMES if not n.startswith(("refused_", "unsupported_"))]


def refused_names():
    return [n for n in NAMES if n.startswith(("refused_", "unsupported_"))]


def census_table(names=NAMES):
    lines = []
    for n in names:
        c = get(n)
        lines.append("%-36s %5dx%-5d %6d B  status %d" % (n, c.rows, c.cols, len(c.data), c.status))
        for text, observed, holds in c.census:
            lines.append("    %-4s %s: %s" % ("ok" if holds else "FAIL", text, observed))
    return "\n".join(lines)
