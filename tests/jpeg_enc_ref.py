"""The reference's jpg_from_image_cv restated in numpy (duckietown_utils/jpg.py:16-18, cv2.imencode('.jpg', image)): the checker of
lf_jpeg_encode_batch (lane_slam_amd/csrc/k_jenc.hip).  Not a product path.

cv2.imencode hands the image to libjpeg(-turbo) with its defaults: quality 95 through jpeg_set_quality(q, force_baseline = TRUE),
YCbCr with 2x2 luma sampling (4:2:0), the integer "islow" forward DCT, the standard Huffman tables of the JPEG specification's
annex K (no optimisation), one interleaved scan, no restart markers, the default JFIF APP0 segment.  What is restated here is
libjpeg's published behaviour, stage by stage:

* Colour (jccolor.c).  16-bit fixed point, FIX(x) = int(x * 65536 + 0.5):
  Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16, Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16,
  Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16.
* Edges (jcprepct.c, jcsample.c).  Each component plane is widened to whole blocks by repeating its last column BEFORE the
  downsampling (luma to ceil(cols / 8) blocks, the chroma input to 16 * ceil(cols / 16) columns); the colour rows are made an even
  count by repeating the last row, and AFTER the downsampling each plane is made a whole MCU row high by repeating its last row.
* Chroma (h2v2_downsample): (a + b + c + d + bias) >> 2 with bias 1 in even output columns and 2 in odd ones.
* DCT (jfdctint.c): samples - 128, the Loeffler-Ligtenberg-Moschytz butterflies with CONST_BITS 13 and PASS1_BITS 2 in 32-bit
  integers, rows first; the result is 8 times the DCT.
* Quantisation (jcdctmgr.c): tables scaled by jpeg_quality_scaling (q < 50: 5000 / q, else 200 - 2 q; (base * scale + 50) / 100
  clamped to 1 .. 255), divisor q << 3, rounded half away from zero.  libjpeg-turbo multiplies by a reciprocal instead; it is meant
  to equal the division and the comparison with Pillow's files (tests/test_jpeg_encode_cpu.py) is what decides.
* Dummy blocks (jccoefct.c).  An MCU holds 2 x 2 luma blocks; where the luma plane has an odd number of block columns or rows, the
  blocks past its end are not transformed: zero AC and the DC of the preceding block of the MCU, so their DC difference is 0.
* Entropy coding (jchuff.c): DC difference per component in scan order, AC run / size symbols with ZRL (0xF0) for runs above 15 and
  EOB (0x00) when the block ends in zeros; a negative value v is sent as the low bits of v - 1; bytes of 0xFF are followed by 0x00;
  the last byte is filled with 1-bits.
* Header (jcmarker.c): SOI, APP0 (JFIF 1.01, density 1:1, no units), DQT 0, DQT 1, SOF0, DHT DC 0, AC 0, DC 1, AC 1, SOS; EOI after
  the scan.

The target the tests hold this to is Pillow linked against libjpeg-turbo, Image.save(format="JPEG", quality=q, subsampling=2): the whole
file, byte for byte (tests/golden/jpeg_encode_vectors.npz).  That OpenCV 3.3.1's imencode writes the same bytes is a statement about
OpenCV that no test here can check.
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                       87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                       72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                         99, 99, 99, 99] + [99] * 32)

# annex K.3: code counts per length 1 .. 16, and the symbols in code order
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa]


def quant_tables(quality):
    """The two quantisation tables of jpeg_set_quality(quality, TRUE), natural order, int32 [2][64]."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q)]).astype(np.int32)


def huff_table(bits, vals):
    """code and length per symbol (jchuff.c jpeg_make_c_derived_tbl), uint32 [256] each; length 0 where the table has no code."""
    code = np.zeros(256, np.uint32)
    size = np.zeros(256, np.uint32)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c += 1
            k += 1
        c <<= 1
    return code, size


def header(rows, cols, quality):
    """Everything libjpeg writes before the entropy-coded data."""
    qt = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in qt[i][ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([rows >> 8, rows & 255, cols >> 8, cols & 255]) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for cls, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS),
                            (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        n = 2 + 1 + 16 + len(vals)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, cls]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def ycc(bgr):
    """jccolor.c rgb_ycc_convert on a BGR u8 image: Y, Cb, Cr int32 planes."""
    def fix(x):
        return int(x * 65536 + 0.5)
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    half, off = 1 << 15, 128 << 16
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.50000) * b + off + half - 1) >> 16
    cr = (fix(0.50000) * r - fix(0.41869) * g - fix(0.08131) * b + off + half - 1) >> 16
    return y.astype(np.int32), cb.astype(np.int32), cr.astype(np.int32)


def _pad(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def planes(bgr):
    """The three component planes as the DCT reads them, whole MCUs: Y [16 mr][16 mc], Cb and Cr [8 mr][8 mc]."""
    rows, cols = bgr.shape[:2]
    mr, mc = (rows + 15) // 16, (cols + 15) // 16
    y, cb, cr = ycc(bgr)
    out = [_pad(y, 16 * mr, 16 * mc)]          # (columns past ceil(cols / 8) blocks and rows past ceil(rows / 8) belong to dummy blocks)
    for c in (cb, cr):
        c = _pad(c, rows + (rows & 1), 16 * mc)
        bias = np.tile(np.array([1, 2], np.int32), 4 * mc)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(d, 8 * mr, 8 * mc))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint.c over the last axis of d (int32 [..., 8])."""
    CB, PB = 13, 2
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    n = CB - PB if first else CB + PB
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << PB, (t10 - t11) << PB
    else:
        o[..., 0], o[..., 4] = _descale(t10 + t11, PB), _descale(t10 - t11, PB)
    z1 = (t12 + t13) * 4433
    o[..., 2] = _descale(z1 + t13 * 6270, n)
    o[..., 6] = _descale(z1 + t12 * -15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7] = _descale(t4 + z1 + z3, n)
    o[..., 5] = _descale(t5 + z2 + z4, n)
    o[..., 3] = _descale(t6 + z2 + z3, n)
    o[..., 1] = _descale(t7 + z1 + z4, n)
    return o


def fdct_quant(plane, qtab):
    """plane int32 [8 br][8 bc] -> quantised coefficients int32 [br][bc][64] in zigzag order."""
    br, bc = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(br, 8, bc, 8).transpose(0, 2, 1, 3).astype(np.int32) - 128
    d = _fdct_pass(blk, True)                                   # rows
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    d = d.reshape(br, bc, 64)
    div = (qtab.astype(np.int32) << 3)[None, None, :]
    mag = (np.abs(d) + (div >> 1)) // div
    return np.where(d < 0, -mag, mag)[..., ZIGZAG].astype(np.int32)


def coefficients(bgr, quality):
    """The scan's blocks in order: (coef int32 [n][64] zigzag, comp int32 [n], dummy bool [n]); an MCU is Y00 Y01 Y10 Y11 Cb Cr.
    A dummy block's coefficients are zero here; its DC is the preceding block's, which the entropy coder handles as difference 0."""
    rows, cols = bgr.shape[:2]
    mr, mc = (rows + 15) // 16, (cols + 15) // 16
    qt = quant_tables(quality)
    py, pcb, pcr = planes(bgr)
    cy = fdct_quant(py, qt[0]).reshape(mr, 2, mc, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mr, mc, 4, 64)
    ccb, ccr = fdct_quant(pcb, qt[1]), fdct_quant(pcr, qt[1])
    coef = np.concatenate([cy, ccb[:, :, None, :], ccr[:, :, None, :]], axis=2)            # [mr][mc][6][64]
    by = 2 * np.arange(mr)[:, None, None] + np.array([0, 0, 1, 1])[None, None, :]
    bx = 2 * np.arange(mc)[None, :, None] + np.array([0, 1, 0, 1])[None, None, :]
    dummy = np.zeros((mr, mc, 6), bool)
    dummy[:, :, :4] = (by >= (rows + 7) // 8) | (bx >= (cols + 7) // 8)
    coef[dummy] = 0
    comp = np.broadcast_to(np.array([0, 0, 0, 0, 1, 2]), (mr, mc, 6))
    return coef.reshape(-1, 64), comp.reshape(-1).copy(), dummy.reshape(-1)


def _nbits(v):
    """bit length of |v| (int64 array, |v| < 2^15)"""
    a = np.abs(v)
    n = np.zeros(a.shape, np.int64)
    for k in range(15):
        n += (a >> k) > 0
    return n


def entropy_bits(coef, comp, dummy):
    """The scan as one string of bits (uint8 0/1 array) before padding and stuffing, and every block's bit length."""
    n = coef.shape[0]
    tabs = [huff_table(DC_LUMA_BITS, DC_VALS), huff_table(AC_LUMA_BITS, AC_LUMA_VALS), huff_table(DC_CHROMA_BITS, DC_VALS),
            huff_table(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    chroma = (comp > 0).astype(np.int64)
    # token value / length per block and position: 0 the DC, 1 .. 63 the AC coefficients (with the ZRLs in front), 64 the EOB
    val = np.zeros((n, 65), np.uint64)
    length = np.zeros((n, 65), np.int64)
    # DC: difference to the preceding block of the component; a dummy block repeats that block's DC
    dc = coef[:, 0].astype(np.int64)
    diff = np.zeros(n, np.int64)
    for c in range(3):
        idx = np.nonzero((comp == c) & ~dummy)[0]
        diff[idx] = np.diff(dc[idx], prepend=0)
    nb = _nbits(diff)
    low = np.where(diff < 0, diff - 1, diff) & ((1 << nb) - 1)
    for t in range(2):
        m = chroma == t
        code, size = tabs[2 * t]
        val[m, 0] = (code[nb[m]].astype(np.uint64) << nb[m].astype(np.uint64)) | low[m].astype(np.uint64)
        length[m, 0] = size[nb[m]].astype(np.int64) + nb[m]
    # AC
    b, k = np.nonzero(coef[:, 1:])
    k = k + 1
    v = coef[b, k].astype(np.int64)
    prev = np.zeros(b.size, np.int64)                        # position of the preceding non-zero coefficient of the block, 0 if none
    if b.size:
        same = np.zeros(b.size, bool)
        same[1:] = b[1:] == b[:-1]
        prev[1:] = np.where(same[1:], k[:-1], 0)
    run = k - prev - 1
    nzrl, r = run >> 4, run & 15
    nb = _nbits(v)
    low = np.where(v < 0, v - 1, v) & ((1 << nb) - 1)
    ch = chroma[b]
    tv = np.zeros(b.size, np.uint64)
    tl = np.zeros(b.size, np.int64)
    for t in range(2):
        m = ch == t
        code, size = tabs[2 * t + 1]
        zc, zs = int(code[0xF0]), int(size[0xF0])
        acc = np.zeros(int(m.sum()), np.uint64)
        al = np.zeros(acc.size, np.int64)
        for j in range(3):                                   # a run is at most 62: three ZRLs
            has = nzrl[m] > j
            acc = np.where(has, (acc << np.uint64(zs)) | np.uint64(zc), acc)
            al = al + np.where(has, zs, 0)
        sym = (r[m] << 4) | nb[m]
        bits = size[sym].astype(np.int64) + nb[m]
        acc = (acc << bits.astype(np.uint64)) | (code[sym].astype(np.uint64) << nb[m].astype(np.uint64)) | low[m].astype(np.uint64)
        tv[m], tl[m] = acc, al + bits
    val[b, k], length[b, k] = tv, tl
    eob = coef[:, 63] == 0
    for t in range(2):
        m = eob & (chroma == t)
        code, size = tabs[2 * t + 1]
        val[m, 64], length[m, 64] = np.uint64(code[0]), int(size[0])
    block_bits = length.sum(axis=1)
    keep = length.reshape(-1) > 0
    tv, tl = val.reshape(-1)[keep], length.reshape(-1)[keep]
    total = int(tl.sum())
    tok = np.repeat(np.arange(tl.size), tl)
    start = np.cumsum(tl) - tl
    pos = np.arange(total) - start[tok]
    bits = ((tv[tok] >> (tl[tok] - 1 - pos).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return bits, block_bits


def scan_bytes(bits):
    """Pad the last byte with 1-bits, pack, and follow every 0xFF by 0x00."""
    pad = (-bits.size) % 8
    by = np.packbits(np.concatenate([bits, np.ones(pad, np.uint8)]))
    ff = np.nonzero(by == 0xFF)[0]
    return np.insert(by, ff + 1, 0).tobytes()


def encode(bgr, quality=95):
    """The JPEG file libjpeg writes for a BGR u8 image (rows, cols, 3) with cv2.imencode's settings."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3 and bgr.shape[0] >= 1 and bgr.shape[1] >= 1
    coef, comp, dummy = coefficients(bgr, quality)
    bits, _ = entropy_bits(coef, comp, dummy)
    return header(bgr.shape[0], bgr.shape[1], quality) + scan_bytes(bits) + b"\xff\xd9"
