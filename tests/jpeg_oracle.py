"""Numpy restatement of the baseline JPEG encoder contract (include/sdfa_jpeg.h, DESIGN.md "GPU JPEG"): the CPU oracle of
csrc/jpeg.hip.  Written from ITU T.81 and the contract alone; it is pinned to PIL (speech_anime.video.encode_jpeg) by
tests/test_jpeg_cpu.py, and the GPU is pinned to it stage by stage (coefficients) and byte by byte (files).

Every stage is integer arithmetic: colour conversion in 16-bit fixed point, 2x2 downsampling by a rounded average with
an alternating bias, edge padding to whole 16 x 16 MCUs, the integer "islow" forward DCT (13-bit constants, 2 pass
bits), rounding quantisation, zigzag, and Huffman coding with the T.81 Annex K tables.  The entropy coder is written the
way the GPU lays it out -- one field list per (block, coefficient) -- so the two read alike."""
import numpy as np

# ---- T.81 Annex K tables ----
LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)          # K.1, natural order
CHROMA_Q = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)                                     # K.2, natural order

ZIGZAG = np.array([                        # ZIGZAG[k] = natural (row-major) index of the k-th zigzag coefficient
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
    62, 63], np.int64)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
    "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
assert len(AC_LUMA_VALS) == sum(AC_LUMA_BITS) == 162 and len(AC_CHROMA_VALS) == sum(AC_CHROMA_BITS) == 162

# islow constants: FIX(x) = round(x * 2^13)
CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765 = 2446, 3196, 4433, 6270
F_0_899, F_1_175, F_1_501, F_1_847 = 7373, 9633, 12299, 15137
F_1_961, F_2_053, F_2_562, F_3_072 = 16069, 16819, 20995, 25172


def huff_codes(bits, vals):
    """T.81 Annex C: canonical codes.  -> (code[256], length[256]) indexed by symbol (length 0 = absent)."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


DC_TABLES = (huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS))
AC_TABLES = (huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def quant_tables(quality):
    """libjpeg quality scaling, baseline-clamped: (luma, chroma) int64 (64,) in natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA_Q, CHROMA_Q))


# ---- header ----

def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def header(width, height, quality):
    """SOI .. SOS: every byte before the entropy-coded data."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tid, tab in enumerate((ql, qc)):
        out += _seg(0xDB, bytes([tid]) + bytes(int(v) for v in tab[ZIGZAG]))
    out += _seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls_id, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                               (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _seg(0xC4, bytes([cls_id] + bits + vals))
    out += _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


# ---- pixels -> planes ----

def ycc(rgb):
    """(H, W, 3) uint8 -> Y, Cb, Cr int64 planes: 16-bit fixed point, rounded, chroma offset 128."""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    half, off = 1 << 15, 128 << 16
    y = (19595 * r + 38470 * g + 7471 * b + half) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + off + half - 1) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + off + half - 1) >> 16
    return y, cb, cr


def geometry(width, height):
    """MCU columns and rows, luma blocks across and down (the true block extent)."""
    return -(-width // 16), -(-height // 16), -(-width // 8), -(-height // 8)


def planes(rgb):
    """Padded component planes: Y (16 mcy, 16 mcx) by edge replication; Cb, Cr (8 mcy, 8 mcx), each sample the 2 x 2
    average (+ bias 1, 2, 1, 2, ... along the row) >> 2 of the image padded to even height and 16 mcx columns by
    replication, the rows past ceil(H / 2) repeating the last one."""
    H, W = rgb.shape[:2]
    mcx, mcy, _, _ = geometry(W, H)
    y, cb, cr = ycc(rgb)
    ys = np.minimum(np.arange(16 * mcy), H - 1)
    xs = np.minimum(np.arange(16 * mcx), W - 1)
    Y = y[ys][:, xs]
    hc = (H + 1) // 2
    cy = np.minimum(np.arange(8 * mcy), hc - 1)
    r0, r1 = 2 * cy, np.minimum(2 * cy + 1, H - 1)
    c0, c1 = xs[0::2], xs[1::2]
    bias = np.tile([1, 2], 4 * mcx)
    C = [(p[r0][:, c0] + p[r0][:, c1] + p[r1][:, c0] + p[r1][:, c1] + bias) >> 2 for p in (cb, cr)]
    return Y, C[0], C[1]


# ---- forward DCT and quantisation ----

def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One islow pass over axis -1 of int64 d (..., 8)."""
    tmp0, tmp7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    tmp1, tmp6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    tmp2, tmp5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    tmp3, tmp4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    out = np.empty_like(d)
    if first:
        out[..., 0] = (tmp10 + tmp11) << PASS1_BITS
        out[..., 4] = (tmp10 - tmp11) << PASS1_BITS
    else:
        out[..., 0] = _descale(tmp10 + tmp11, PASS1_BITS)
        out[..., 4] = _descale(tmp10 - tmp11, PASS1_BITS)
    z1 = (tmp12 + tmp13) * F_0_541
    out[..., 2] = _descale(z1 + tmp13 * F_0_765, sh)
    out[..., 6] = _descale(z1 - tmp12 * F_1_847, sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F_1_175
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F_0_298, tmp5 * F_2_053, tmp6 * F_3_072, tmp7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[..., 7] = _descale(tmp4 + z1 + z3, sh)
    out[..., 5] = _descale(tmp5 + z2 + z4, sh)
    out[..., 3] = _descale(tmp6 + z2 + z3, sh)
    out[..., 1] = _descale(tmp7 + z1 + z4, sh)
    return out


def fdct_quant(blocks, qtab):
    """(..., 8, 8) samples 0..255 -> (..., 64) quantised coefficients in zigzag order."""
    d = blocks.astype(np.int64) - 128
    d = _fdct_1d(d, True)
    d = np.swapaxes(_fdct_1d(np.swapaxes(d, -1, -2), False), -1, -2)       # columns; result x 8
    d = d.reshape(d.shape[:-2] + (64,))
    div = 8 * qtab
    q = (np.abs(d) + (div >> 1)) // div
    return (np.where(d < 0, -q, q))[..., ZIGZAG]


def _blocks(plane, by, bx):
    """(8 by, 8 bx) -> (by, bx, 8, 8)."""
    return plane.reshape(by, 8, bx, 8).swapaxes(1, 2)


def coefficients(rgb, quality):
    """(H, W, 3) uint8 -> (mcy * mcx, 6, 64) int16: quantised zigzag coefficients in coding order (MCU raster; Y00 Y01
    Y10 Y11 Cb Cr), dummy luma blocks (outside the true extent) already AC zero with the DC of the block before them."""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    mcx, mcy, bw, bh = geometry(W, H)
    ql, qc = quant_tables(quality)
    Y, Cb, Cr = planes(rgb)
    cy = fdct_quant(_blocks(Y, 2 * mcy, 2 * mcx), ql)                       # (2 mcy, 2 mcx, 64)
    out = np.empty((mcy, mcx, 6, 64), np.int64)
    out[:, :, 0] = cy[0::2, 0::2]
    out[:, :, 1] = cy[0::2, 1::2]
    out[:, :, 2] = cy[1::2, 0::2]
    out[:, :, 3] = cy[1::2, 1::2]
    out[:, :, 4] = fdct_quant(_blocks(Cb, mcy, mcx), qc)
    out[:, :, 5] = fdct_quant(_blocks(Cr, mcy, mcx), qc)
    if bw & 1:                                                              # right dummies: Y01, Y11 of the last MCU column
        for b in (1, 3):
            out[:, -1, b] = 0
            out[:, -1, b, 0] = out[:, -1, b - 1, 0]
    if bh & 1:                                                              # bottom dummies: Y10, Y11 take Y01's DC
        for b in (2, 3):
            out[-1, :, b] = 0
            out[-1, :, b, 0] = out[-1, :, 1, 0]
    return out.reshape(mcy * mcx, 6, 64).astype(np.int16)


# ---- entropy coding ----

def _size(v):
    """Bit length of |v| (0 for 0)."""
    a = np.abs(v)
    s = np.zeros(a.shape, np.int64)
    while (a >> s).any():
        s += (a >> s) > 0
    return s


def _mag(v, s):
    """The s low bits that code v: v if v > 0, else v - 1 (ones' complement)."""
    return np.where(v < 0, v + (1 << s) - 1, v) & ((1 << s) - 1)


def fields(coefs):
    """(n_mcu, 6, 64) coefficients -> (value, nbits) int64 arrays of shape (n_blocks, 64, 6): per block and zigzag
    position k, up to 3 ZRL codes, the symbol's code, its magnitude bits and an EOB (after the last nonzero coefficient,
    at k = 0 when every AC coefficient is zero).  Position 0 carries the DC difference's code and bits."""
    c = np.asarray(coefs, np.int64)
    n_mcu = c.shape[0]
    comp = np.array([0, 0, 0, 0, 1, 2])
    tab = np.array([0, 0, 0, 0, 1, 1])
    dc = c[:, :, 0]
    prev = np.zeros_like(dc)
    ylin = dc[:, :4].reshape(-1)
    prev[:, :4] = np.concatenate([[0], ylin[:-1]]).reshape(n_mcu, 4)
    prev[1:, 4:] = dc[:-1, 4:]
    diff = (dc - prev).reshape(-1)
    t = np.tile(tab, n_mcu)
    ac = c.reshape(-1, 64)
    nb = ac.shape[0]
    val, nbits = np.zeros((nb, 64, 6), np.int64), np.zeros((nb, 64, 6), np.int64)

    s = _size(diff)
    for ti in (0, 1):
        code, ln = DC_TABLES[ti]
        m = t == ti
        val[m, 0, 3], nbits[m, 0, 3] = code[s[m]], ln[s[m]]
    val[:, 0, 4], nbits[:, 0, 4] = _mag(diff, s), s

    k = np.arange(64)
    nz = (ac != 0) & (k > 0)
    last = np.where(nz, k, 0)
    prevnz = np.maximum.accumulate(np.concatenate([np.zeros((nb, 1), np.int64), last[:, :-1]], 1), axis=1)
    run = k - prevnz - 1
    sz = _size(ac)
    sym = ((run % 16) << 4) | sz
    lastnz = last.max(1)
    for ti in (0, 1):
        code, ln = AC_TABLES[ti]
        m = (t == ti)[:, None] & nz
        for z in range(3):
            mz = m & (run >= 16 * (z + 1))
            val[mz, z], nbits[mz, z] = code[0xF0], ln[0xF0]
        val[m, 3], nbits[m, 3] = code[sym[m]], ln[sym[m]]
        me = (t == ti) & (lastnz < 63)
        val[me, lastnz[me], 5], nbits[me, lastnz[me], 5] = code[0x00], ln[0x00]
    val[:, 1:, 4] = np.where(nz[:, 1:], _mag(ac[:, 1:], sz[:, 1:]), 0)
    nbits[:, 1:, 4] = np.where(nz[:, 1:], sz[:, 1:], 0)
    return val, nbits


def block_bits(coefs):
    """(n_blocks,) bit length of each block's entropy-coded data."""
    return fields(coefs)[1].sum((1, 2))


def entropy(coefs):
    """Entropy-coded segment: the fields' bits, padded with 1-bits to a byte, every 0xFF followed by 0x00."""
    val, nbits = (a.reshape(-1) for a in fields(coefs))
    keep = nbits > 0
    val, nbits = val[keep], nbits[keep]
    total = int(nbits.sum())
    start = np.cumsum(nbits) - nbits
    j = np.arange(total) - np.repeat(start, nbits)
    bits = (np.repeat(val, nbits) >> (np.repeat(nbits, nbits) - 1 - j)) & 1
    bits = np.concatenate([bits, np.ones(-total % 8, np.int64)]).astype(np.uint8)
    data = np.packbits(bits)
    ff = data == 0xFF
    out = np.zeros(len(data) + int(ff.sum()), np.uint8)
    out[np.arange(len(data)) + np.concatenate([[0], np.cumsum(ff)[:-1]])] = data
    return out.tobytes()


def encode(rgb, quality=90):
    """(H, W, 3) uint8 -> the JPEG file PIL writes with quality=quality and its other defaults."""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    return header(W, H, quality) + entropy(coefficients(rgb, quality)) + b"\xff\xd9"


def max_frame_bytes(width, height):
    """The encoder's per-frame capacity bound (include/sdfa_jpeg.h): header + 2 x (ceil(1660 n_blocks / 8) + 1) + EOI."""
    mcx, mcy, _, _ = geometry(width, height)
    return len(header(width, height, 90)) + 2 * ((1660 * 6 * mcx * mcy + 7) // 8 + 1) + 2
