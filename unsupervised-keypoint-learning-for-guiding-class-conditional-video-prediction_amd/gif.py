"""Animated GIFs of rollouts (evaluate.py --gif; DESIGN.md sections 2 and 4.4).

The frames stay on the device until they are one byte per pixel: ``ops.sheet_paste`` composes the 8-bit canvases, ``ops.color_hist_add``
counts their colours, ``median_cut`` (here, numpy: 512 KB per sample) picks ONE palette per GIF from all its frames -- a global palette is
what keeps a flat background from flickering --, ``ops.palette_map`` finds the nearest palette entry of every pixel, and ``write_gif`` packs
the indices with the library's LZW encoder (``kpx_gif_lzw_u8``, host code) into a GIF89a file.  Integer arithmetic throughout.
"""
import json
import os
import struct

import numpy as np

from . import _lib

CELLS = 32768                                     # 5-5-5 cells: (r >> 3) << 10 | (g >> 3) << 5 | b >> 3
MAX_COLORS = 256
FPS_RANGE = (1, 50)
DITHER_RANGE = (0, 64)
BAYER4 = ((0, 8, 2, 10), (12, 4, 14, 6), (3, 11, 1, 9), (15, 7, 13, 5))     # the mapping kernel's ordered-dither matrix


def median_cut(hist, P=MAX_COLORS, return_boxes=False):
    """hist: integer [32768, 4] = (count, sum r, sum g, sum b) per 5-5-5 cell -> palette uint8 [n, 3], 1 <= n <= P.

    Boxes are sets of occupied cells, one box first.  While there are fewer than P boxes and some box has two or more cells: take the box
    with the largest extent along any axis in cell units (ties: the larger pixel count, then the lower box index); split it along its longest
    axis (ties in r, g, b order): sort its cells by (coordinate, cell index), cut after the first prefix that holds at least half of the
    box's pixels, clamped so that both parts are non-empty; the lower part keeps the index, the upper part is appended.  A palette entry is
    (2 sum c + n) // (2 n) per channel over its box.  So a canvas with at most P occupied cells gets one entry per cell.  An empty histogram
    gives one black entry.  ``return_boxes``: also the boxes, a list of int64 arrays of cell indices."""
    hist = np.asarray(hist)
    if hist.shape != (CELLS, 4) or hist.dtype.kind not in 'iu':
        raise ValueError('median_cut: hist must be an integer [%d, 4] array (got %s %s)' % (CELLS, hist.shape, hist.dtype))
    if not 1 <= int(P) <= MAX_COLORS:
        raise ValueError('median_cut: P must be in [1, %d] (got %r)' % (MAX_COLORS, P))
    hist = hist.astype(np.int64)
    cells = np.nonzero(hist[:, 0])[0]
    if cells.size == 0:
        pal = np.zeros((1, 3), np.uint8)
        return (pal, [cells]) if return_boxes else pal
    coords = np.stack([cells >> 10, (cells >> 5) & 31, cells & 31], axis=1)           # [n, 3]
    counts = hist[cells, 0]

    def describe(members):                        # members: positions into cells, ascending -> (extent, axis, pixel count)
        c = coords[members]
        ext = c.max(axis=0) - c.min(axis=0)
        axis = int(np.argmax(ext))                # the first maximum: ties in r, g, b order
        return int(ext[axis]), axis, int(counts[members].sum())

    boxes = [np.arange(cells.size)]
    axes = [0] * P
    rank = np.full(P, -1, np.int64)               # per box extent << 32 | pixel count (< 2^32); -1: fewer than two cells, never split
    total = np.zeros(P, np.int64)

    def put(i, members):
        ext, axes[i], total[i] = describe(members)
        rank[i] = (ext << 32) | total[i] if members.size >= 2 else -1

    put(0, boxes[0])
    while len(boxes) < P:
        pick = int(np.argmax(rank))               # the first maximum: a tie stays with the lower index
        if rank[pick] < 0:
            break
        members, axis = boxes[pick], axes[pick]
        order = members[np.argsort(coords[members, axis], kind='stable')]             # members ascend: the sort is by (coordinate, cell)
        cum = np.cumsum(counts[order])
        k = int(np.searchsorted(2 * cum, total[pick], side='left')) + 1               # the first prefix with 2 cum >= total
        k = min(max(k, 1), order.size - 1)
        lower, upper = np.sort(order[:k]), np.sort(order[k:])
        boxes[pick] = lower
        put(pick, lower)
        boxes.append(upper)
        put(len(boxes) - 1, upper)
    pal = np.empty((len(boxes), 3), np.uint8)
    for i, members in enumerate(boxes):
        s = hist[cells[members]].sum(axis=0)
        pal[i] = (2 * s[1:] + s[0]) // (2 * s[0])
    return (pal, [cells[m] for m in boxes]) if return_boxes else pal


def palette_bits(p):
    """bits of the colour table of a palette of p entries: max(1, ceil(log2 p))"""
    return max(1, int(p - 1).bit_length())


def lzw(idx, min_code_size):
    """flat uint8 indices -> the LZW byte stream (``kpx_gif_lzw_u8``: host code of the library)"""
    idx = np.ascontiguousarray(idx, np.uint8).reshape(-1)
    out = np.empty(int(_lib.lib.kpx_gif_lzw_bound(idx.size)), np.uint8)
    n = _lib.lib.kpx_gif_lzw_u8(idx.ctypes.data if idx.size else out.ctypes.data, idx.size, int(min_code_size), out.ctypes.data, out.size)
    if n < 0:
        raise _lib.KpxError('kpx_gif_lzw_u8 failed with code %d (an index outside the colour table?)' % n)
    return out[:n].tobytes()


def gif_bytes(idx, palette, delay_cs):
    """idx uint8 [T, H, W] (T frames of palette indices), palette uint8 [P, 3], delay in centiseconds -> the bytes of a GIF89a file: logical
    screen descriptor with a global colour table of 2^bits entries (bits = max(1, ceil(log2 P)), zero-padded), a NETSCAPE2.0 loop-forever
    block, per frame a graphic control extension (disposal 1, the delay, no transparency), an image descriptor of the full frame without a
    local table and the LZW data (minimum code size max(2, bits)) in 255-byte sub-blocks, then the trailer."""
    idx = np.asarray(idx)
    palette = np.asarray(palette)
    if idx.dtype != np.uint8 or idx.ndim != 3 or min(idx.shape) < 1 or max(idx.shape[1:]) > 65535:
        raise ValueError('gif_bytes: idx must be uint8 [T, H, W] with T, H, W >= 1 and H, W <= 65535 (got %s %s)' % (idx.dtype, idx.shape))
    if palette.dtype != np.uint8 or palette.ndim != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= MAX_COLORS:
        raise ValueError('gif_bytes: palette must be uint8 [P, 3], 1 <= P <= 256 (got %s %s)' % (palette.dtype, palette.shape))
    if not 0 <= int(delay_cs) <= 65535:
        raise ValueError('gif_bytes: delay_cs must be in [0, 65535] (got %r)' % (delay_cs,))
    p = palette.shape[0]
    if int(idx.max()) >= p:
        raise ValueError('gif_bytes: index %d outside a palette of %d entries' % (int(idx.max()), p))
    t, h, w = idx.shape
    bits = palette_bits(p)
    code = max(2, bits)
    table = np.zeros((1 << bits, 3), np.uint8)
    table[:p] = palette
    parts = [b'GIF89a', struct.pack('<HHBBB', w, h, 0x80 | ((bits - 1) << 4) | (bits - 1), 0, 0), table.tobytes(),
             b'\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00']
    for f in range(t):
        parts.append(struct.pack('<BBBBHBB', 0x21, 0xf9, 4, 1 << 2, int(delay_cs), 0, 0))
        parts.append(struct.pack('<BHHHHB', 0x2c, 0, 0, w, h, 0))
        parts.append(bytes([code]))
        data = lzw(idx[f], code)
        for s in range(0, len(data), 255):
            blk = data[s:s + 255]
            parts.append(bytes([len(blk)]))
            parts.append(blk)
        parts.append(b'\x00')
    parts.append(b'\x3b')
    return b''.join(parts)


def write_gif(path, idx, palette, delay_cs):
    data = gif_bytes(idx, palette, delay_cs)
    with open(path, 'wb') as f:
        f.write(data)


def delay_of_fps(fps):
    """the GIF delay in centiseconds of --gif-fps"""
    return int(round(100.0 / fps))


class RolloutGifs:
    """evaluate.py --gif: per batch, the canvases of pred.gif and compare.gif composed and quantised on the device (one byte per pixel
    reaches the host), written per sample; gif.json at the end."""

    def __init__(self, fps, dither):
        self.fps, self.dither, self.delay = int(fps), int(dither), delay_of_fps(fps)
        self.columns = self.frames = self.cell = None
        self.sizes = {'pred': [], 'compare': []}
        self._pinned = {}

    def _host(self, t):
        import torch
        key = tuple(t.shape)
        if key not in self._pinned:
            self._pinned[key] = torch.empty(key, dtype=torch.uint8, pin_memory=True)
        self._pinned[key].copy_(t)                # synchronous
        return self._pinned[key].numpy()

    def _canvas(self, columns):
        """columns: [(first [B,H,W,C], seq [B,F,H,W,C], premap)] -> uint8 [B, F + 1, H, len(columns) * W, 3] on the device"""
        import torch
        from . import ops
        b, f, h, w = columns[0][1].shape[:4]
        canvas = torch.empty((b * (f + 1), h, len(columns) * w, 3), dtype=torch.uint8, device=columns[0][1].device)
        for col, (first, seq, premap) in enumerate(columns):
            stack = torch.empty((b, f + 1) + tuple(seq.shape[2:]), dtype=torch.float32, device=seq.device)
            stack[:, 0].copy_(first)
            stack[:, 1:].copy_(seq)
            ops.sheet_paste(canvas, stack.view((b * (f + 1), 1) + tuple(seq.shape[2:])), [0], 0, col, premap)
        return canvas.view(b, f + 1, h, len(columns) * w, 3)

    def write(self, save_dir, first_sample, columns):
        """columns: [(name, first, seq, premap)] in the order of compare.gif; the column named 'pred' alone is pred.gif"""
        from . import ops
        names = [c[0] for c in columns]
        self.columns = names
        for kind, cols in (('pred', [c[1:] for c in columns if c[0] == 'pred']), ('compare', [c[1:] for c in columns])):
            canvas = self._canvas(cols)
            idx, palettes, sizes = ops.gif_indices(canvas, self.dither)
            host = self._host(idx)
            self.frames, self.cell = int(canvas.shape[1]), [int(canvas.shape[2]), int(canvas.shape[3]) // len(cols)]
            for i in range(canvas.shape[0]):
                d = os.path.join(save_dir, '%04d' % (first_sample + i))
                os.makedirs(d, exist_ok=True)
                write_gif(os.path.join(d, kind + '.gif'), host[i], palettes[i, :sizes[i]], self.delay)
                self.sizes[kind].append(int(sizes[i]))

    def write_json(self, save_dir):
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, 'gif.json'), 'w') as f:
            json.dump({'columns': self.columns, 'fps': self.fps, 'delay_cs': self.delay, 'dither': self.dither, 'frames': self.frames,
                       'cell': self.cell, 'palette_sizes': self.sizes}, f, indent=1)
