"""numpy and pure-Python restatement of the GIF pipeline (DESIGN.md sections 2 and 4.4, evaluate.py --gif): the 5-5-5 colour histogram, the
median cut, the nearest-palette-entry search with the ordered dither, GIF's LZW and the GIF89a container.  Written from the rules, not from
the code under test: the CPU tests hold kpx_amd.gif and kpx_gif_lzw_u8 to it byte for byte, the GPU tests the two kernels bit for bit."""
import struct

import numpy as np

BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)


def cell_of(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return ((rgb[..., 0] >> 3) << 10) | ((rgb[..., 1] >> 3) << 5) | (rgb[..., 2] >> 3)


def hist_add(hist, rgb):
    """hist uint32 [G, 32768, 4] += (count, sum r, sum g, sum b) per cell of rgb uint8 [G, n, 3]; modulo 2^32 like the device's integers"""
    for g in range(rgb.shape[0]):
        px = rgb[g].reshape(-1, 3).astype(np.int64)
        cells = cell_of(px)
        acc = np.zeros((32768, 4), np.int64)
        acc[:, 0] = np.bincount(cells, minlength=32768)
        for c in range(3):
            acc[:, 1 + c] = np.bincount(cells, weights=px[:, c].astype(np.float64), minlength=32768).astype(np.int64)   # < 2^53: exact
        hist[g] = ((hist[g].astype(np.int64) + acc) & 0xffffffff).astype(np.uint32)
    return hist


def median_cut(hist, P=256):
    """-> (palette uint8 [n, 3], boxes: lists of cell indices); plain Python over the occupied cells"""
    hist = np.asarray(hist).astype(np.int64)
    occupied = [int(c) for c in np.nonzero(hist[:, 0])[0]]
    if not occupied:
        return np.zeros((1, 3), np.uint8), [[]]
    coord = lambda cell, axis: (cell >> (10, 5, 0)[axis]) & 31
    count = lambda box: sum(int(hist[c, 0]) for c in box)

    def extent(box):                              # (largest extent, its axis: the first of r, g, b)
        ext = [max(coord(c, a) for c in box) - min(coord(c, a) for c in box) for a in range(3)]
        return max(ext), ext.index(max(ext))

    boxes = [occupied]
    facts = [extent(occupied) + (count(occupied),)]                            # per box, kept beside it: (extent, axis, pixel count)
    while len(boxes) < P:
        best = None
        for i, box in enumerate(boxes):
            if len(box) < 2:
                continue
            key = (facts[i][0], facts[i][2], -i)
            if best is None or key > best[0]:
                best = (key, i)
        if best is None:
            break
        i = best[1]
        box, (_, axis, total) = boxes[i], facts[i]
        ordered = sorted(box, key=lambda c: (coord(c, axis), c))
        run, cut = 0, None
        for k, c in enumerate(ordered):
            run += int(hist[c, 0])
            if 2 * run >= total:
                cut = k + 1
                break
        cut = min(max(cut, 1), len(ordered) - 1)
        boxes[i] = ordered[:cut]
        boxes.append(ordered[cut:])
        facts[i] = extent(boxes[i]) + (count(boxes[i]),)
        facts.append(extent(boxes[-1]) + (count(boxes[-1]),))
    pal = np.zeros((len(boxes), 3), np.uint8)
    for i, box in enumerate(boxes):
        n = count(box)
        for ch in range(3):
            s = sum(int(hist[c, 1 + ch]) for c in box)
            pal[i, ch] = (2 * s + n) // (2 * n)
    return pal, boxes


def dithered(rgb, amp):
    """rgb uint8 [..., H, Wc, 3] -> int64, each channel clamp(c + (((2 M[y & 3][x & 3] - 15) A + 16) >> 5), 0, 255)"""
    rgb = np.asarray(rgb).astype(np.int64)
    h, w = rgb.shape[-3], rgb.shape[-2]
    m = BAYER[np.arange(h)[:, None] & 3, np.arange(w)[None, :] & 3]
    off = ((2 * m - 15) * int(amp) + 16) >> 5                                  # numpy's >> on int64 is arithmetic
    return np.clip(rgb + off[:, :, None], 0, 255)


def palette_map(rgb, palette, amp=0):
    """rgb uint8 [T, H, Wc, 3], palette uint8 [P, 3] -> uint8 [T, H, Wc]: the smallest index among the nearest entries"""
    c = dithered(rgb, amp) if amp else np.asarray(rgb).astype(np.int64)
    pal = np.asarray(palette).astype(np.int64)
    out = np.empty(c.shape[:-1], np.uint8)
    flat, o = c.reshape(-1, 3), out.reshape(-1)
    if flat.shape[0] <= 1 << 16:                                               # the rule as written
        for s in range(0, flat.shape[0], 1 << 14):
            d = ((flat[s:s + (1 << 14), None, :] - pal[None, :, :]) ** 2).sum(axis=2)
            o[s:s + (1 << 14)] = np.argmin(d, axis=1)                          # the first minimum
        return out
    # Whole rollouts: the same argmin from |p|^2 - 2 c.p (|c|^2 is common to a pixel's candidates) as one float32 matrix product per
    # chunk.  Every product is <= 255^2 and every sum < 2^24, so float32 holds them exactly whatever the order of the additions
    # (test_gif_cpu.py holds the two forms equal).
    pp = (pal ** 2).sum(axis=1).astype(np.float32)
    pt = np.ascontiguousarray(pal.T.astype(np.float32))
    for s in range(0, flat.shape[0], 1 << 16):
        d = pp[None, :] - 2.0 * (flat[s:s + (1 << 16)].astype(np.float32) @ pt)
        o[s:s + (1 << 16)] = np.argmin(d, axis=1)
    return out


def quantise(canvas, amp=0, P=256):
    """the whole pipeline for one canvas uint8 [T, H, Wc, 3] -> (idx, palette)"""
    hist = hist_add(np.zeros((1, 32768, 4), np.uint32), canvas.reshape(1, -1, 3))
    pal, _ = median_cut(hist[0], P)
    return palette_map(canvas, pal, amp), pal


def lzw(indices, min_code):
    """GIF's LZW with a dict: clear first, LSB-first packing, width + 1 when the next free code equals 2^width (checked after a code is
    emitted, before its string is added), clear and reset when 4096 codes are taken, end code last"""
    clear, end = 1 << min_code, (1 << min_code) + 1
    acc = have = 0
    out = bytearray()

    def put(code, width):
        nonlocal acc, have
        acc |= code << have
        have += width
        while have >= 8:
            out.append(acc & 255)
            acc >>= 8
            have -= 8

    table, nxt, width = {}, end + 1, min_code + 1
    put(clear, width)
    indices = [int(v) for v in indices]
    if indices:
        prefix = indices[0]
        for k in indices[1:]:
            hit = table.get((prefix, k))
            if hit is not None:
                prefix = hit
                continue
            put(prefix, width)
            if nxt == 4096:
                put(clear, width)
                table, nxt, width = {}, end + 1, min_code + 1
            else:
                if nxt == 1 << width:
                    width += 1
                table[(prefix, k)] = nxt
                nxt += 1
            prefix = k
        put(prefix, width)
        if nxt == 1 << width and width < 12:
            width += 1
    put(end, width)
    if have:
        out.append(acc & 255)
    return bytes(out)


def gif_bytes(idx, palette, delay_cs):
    idx, palette = np.asarray(idx), np.asarray(palette)
    t, h, w = idx.shape
    p = palette.shape[0]
    bits = 1
    while (1 << bits) < p:
        bits += 1
    code = max(2, bits)
    out = bytearray(b'GIF89a')
    out += struct.pack('<HH', w, h) + bytes([0x80 | ((bits - 1) << 4) | (bits - 1), 0, 0])
    out += palette.astype(np.uint8).tobytes() + bytes(3 * ((1 << bits) - p))
    out += bytes([0x21, 0xff, 11]) + b'NETSCAPE2.0' + bytes([3, 1, 0, 0, 0])
    for f in range(t):
        out += bytes([0x21, 0xf9, 4, 0x04]) + struct.pack('<H', delay_cs) + bytes([0, 0])
        out += bytes([0x2c]) + struct.pack('<HHHH', 0, 0, w, h) + bytes([0])
        out.append(code)
        data = lzw(idx[f].reshape(-1), code)
        while data:
            out.append(min(255, len(data)))
            out += data[:255]
            data = data[255:]
        out.append(0)
    out.append(0x3b)
    return bytes(out)


def decode_gif(path):
    """-> (frames uint8 [T, H, W, 3], durations ms, loop) through PIL"""
    from PIL import Image
    im = Image.open(path)
    frames, durations = [], []
    for t in range(getattr(im, 'n_frames', 1)):
        im.seek(t)
        frames.append(np.array(im.convert('RGB')))
        durations.append(im.info.get('duration'))
    return np.stack(frames), durations, im.info.get('loop')
