"""numpy restatement of the baseline JPEG encoder of csrc/mjpeg.hip: integers only, so the scan is the same bytes
in any execution order.  Written from the definition and the tables of ITU T.81 Annex K; nothing here calls the library.

    planes(rgb)          -> Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2], level-shifted int64
    blocks(rgb, quality) -> zig-zag coefficients int64 [H/16, W/16, 6, 64] (four Y blocks in raster order, Cb, Cr)
    encode(rgb, quality) -> the bytes between SOS and EOI: one restart interval per MCU row, RSTm between them
"""
import numpy as np

# ---- T.81 Annex K.1 / K.2, natural (row-major) order
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                       72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                        + [99] * 32, np.int64)

# ---- T.81 Annex K.3 - K.6: (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
            0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a]
           + [r << 4 | s for r in range(2, 8) for s in range(5 if r == 2 else 4 if r == 3 else 3, 11)]
           + [r << 4 | s for r in range(8, 14) for s in range(3 if r == 8 else 2, 11)]
           + [r << 4 | s for r in range(14, 16) for s in range(1, 11)])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
              0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1,
              0x17, 0x18, 0x19, 0x1a]
             + [r << 4 | s for r in range(2, 8) for s in range(6 if r == 2 else 5 if r == 3 else 3, 11)]
             + [r << 4 | s for r in range(8, 16) for s in range(2, 11)])

# zig-zag: ZIGZAG[k] = the natural index of the k-th coefficient of the scan
ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) & 1 else i % 8)), np.int64)

# T[u][x] = rint(8192 alpha(u) cos((2x+1) u pi / 16)) as literal integers
DCT = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], np.int64)


def quant_tables(quality):
    """the IJG quality rule on the Annex K tables -> int64 [2, 64], natural order, each in 1..255"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('quality must be in 1..100')
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA)])


def huffman_codes(table):
    """(bits, symbols) -> {symbol: (code, length)}: the canonical codes of T.81 Annex C"""
    bits, vals = table
    assert sum(bits) == len(vals)
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def planes(rgb):
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.shape[0] % 16 == 0 and rgb.shape[1] % 16 == 0
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = np.clip((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32768) >> 16, 0, 255)
    cr = np.clip((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32768) >> 16, 0, 255)

    def half(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return y - 128, half(cb) - 128, half(cr) - 128


def _quantised(plane, q):
    """plane int64 [h, w] -> zig-zag coefficients [h/8, w/8, 64]"""
    h, w = plane.shape
    s = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)                   # [by, bx, y, x]
    f = np.einsum('vy,abyx,ux->abvu', DCT, s, DCT)                                   # exact in int64: |F| < 2^38
    qq = q.reshape(8, 8)
    c = np.sign(f) * ((np.abs(f) + (qq << 25)) // (qq << 26))
    return c.reshape(h // 8, w // 8, 64)[..., ZIGZAG]


def blocks(rgb, quality):
    qt = quant_tables(quality)
    y, cb, cr = planes(rgb)
    yq, cbq, crq = _quantised(y, qt[0]), _quantised(cb, qt[1]), _quantised(cr, qt[1])
    my, mx = cbq.shape[:2]
    out = np.empty((my, mx, 6, 64), np.int64)
    for k in range(4):
        out[:, :, k] = yq[k >> 1::2, k & 1::2]
    out[:, :, 4], out[:, :, 5] = cbq, crq
    return out


class BitWriter:
    """MSB-first bits into bytes; a 0x00 follows every 0xFF; ``flush`` pads the last byte with 1 bits"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xff
            self.out.append(byte)
            if byte == 0xff:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value(v):
    """(category, extra bits) of a non-zero difference or coefficient"""
    cat = int(abs(v)).bit_length()
    return cat, (v if v > 0 else v - 1) & ((1 << cat) - 1)


def encode_block(w, zz, pred, dc, ac, stats=None):
    diff = int(zz[0]) - pred
    if diff == 0:
        w.put(*dc[0])
    else:
        cat, extra = _value(diff)
        code, length = dc[cat]
        w.put(code << cat | extra, length + cat)
        if stats is not None:
            stats['dc_cat'] = max(stats.get('dc_cat', 0), cat)
    last = 0
    for k in np.nonzero(zz[1:])[0] + 1:
        run = int(k) - last - 1
        while run >= 16:
            w.put(*ac[0xf0])
            run -= 16
            if stats is not None:
                stats['zrl'] = stats.get('zrl', 0) + 1
        cat, extra = _value(int(zz[k]))
        code, length = ac[run << 4 | cat]
        w.put(code << cat | extra, length + cat)
        if stats is not None:
            stats['ac_cat'] = max(stats.get('ac_cat', 0), cat)
        last = int(k)
    if last < 63:
        w.put(*ac[0x00])
    elif stats is not None:
        stats['no_eob'] = stats.get('no_eob', 0) + 1
    return int(zz[0])


def encode(rgb, quality, stats=None):
    """rgb uint8 [H, W, 3], H and W multiples of 16 -> the entropy-coded scan.  ``stats``: a dict that collects which branches ran."""
    coef = blocks(rgb, quality)
    dcs = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
    acs = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]
    out = bytearray()
    rows = coef.shape[0]
    for r in range(rows):
        w, pred = BitWriter(), [0, 0, 0]
        for m in range(coef.shape[1]):
            for k in range(6):
                comp = max(0, k - 3)
                pred[comp] = encode_block(w, coef[r, m, k], pred[comp], dcs[min(comp, 1)], acs[min(comp, 1)], stats)
        w.flush()
        if stats is not None:
            stats['stuffed'] = stats.get('stuffed', 0) + w.out.count(b'\xff')
        out += w.out
        if r < rows - 1:
            out += bytes([0xff, 0xd0 + (r & 7)])
    return bytes(out)


# ---- the fixtures of tests/test_mjpeg_cpu.py and tests/test_mjpeg_gpu.py: seeded, the smallest shapes that reach each branch of the coder
def _smooth(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    field = np.stack([128 + 100 * np.sin(xx / 9 + yy / 23), 128 + 90 * np.cos(yy / 17 - xx / 31), 40 + 170 * xx / w], -1)
    return np.clip(np.rint(field + rng.normal(0, 6, (h, w, 3))), 0, 255).astype(np.uint8)


def _grey(plane):
    return np.repeat(np.asarray(plane, np.uint8)[..., None], 3, axis=2)


def fixtures():
    """name -> (rgb uint8 [H, W, 3], the qualities it is coded at)"""
    yy, xx = np.mgrid[0:32, 0:48]
    cells = np.random.default_rng(3).integers(0, 2, (18, 4)) * 255
    return {
        'flat': (np.full((16, 16, 3), (200, 30, 90), np.uint8), (75,)),
        'two_tone': (_grey(np.repeat([[0, 255]], 16, axis=0).repeat(16, axis=1)), (100,)),
        'cells': (_grey(cells.repeat(8, axis=0).repeat(8, axis=1)), (100,)),                       # 144 x 32: 9 MCU rows
        'checker': (_grey(((yy + xx) & 1) * 255), (100,)),
        'grey_checker': (_grey(120 + ((yy + xx) & 1) * 16), (50,)),
        'noise': (np.random.default_rng(5).integers(0, 256, (32, 32, 3), dtype=np.uint8), (25, 75, 100)),
        'smooth': (_smooth(160, 48, 7), (25, 75, 90, 100)),
        'smooth_wide': (_smooth(128, 384, 8), (90,)),
    }


def mixed_batch():
    """five different 32 x 48 frames for one call"""
    f = fixtures()
    rng = np.random.default_rng(11)
    return np.stack([f['checker'][0], f['grey_checker'][0], rng.integers(0, 256, (32, 48, 3), dtype=np.uint8), _smooth(32, 48, 12),
                     np.full((32, 48, 3), (7, 250, 128), np.uint8)])
