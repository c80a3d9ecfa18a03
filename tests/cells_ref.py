"""numpy restatement of the animated grids (DESIGN.md sections 2 and 4.4, animate.py): the cell composition of kpx_cell_frames_u8_f32 and its
key-point markers, written from the rules (include/kpx.h), not from the kernel.  numpy only."""
import numpy as np

from sheet_ref import QUANTISERS

LIMIT = np.float32(4.0)


def centre16(v, n):
    """The marker centre in 1/16 pixel along an axis of n pixels: (int) rint(fl(fl(fl(v + 1) * 0.5) * fl(16 (n - 1)))), float32 steps, ties to
    even.  v: finite float32 array -> int64."""
    v = np.asarray(v, dtype=np.float32)
    a = (v + np.float32(1)).astype(np.float32)
    a = (a * np.float32(0.5)).astype(np.float32)
    a = (a * np.float32(16 * (n - 1))).astype(np.float32)
    return np.rint(a).astype(np.int64)


def drawn(pts):
    """pts float32 [..., 2] -> bool [...]: the key point draws a marker (finite, |x| <= 4 and |y| <= 4)"""
    pts = np.asarray(pts, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return np.isfinite(pts).all(axis=-1) & (np.abs(pts) <= LIMIT).all(axis=-1)


def marker_layers(pts, h, w, radius):
    """pts float32 [K, 2] (x, y) -> (covered bool [H, W], rgb-index int [H, W], inner bool [H, W]): for every pixel the LOWEST k whose disc
    d2 <= (16 r)^2 covers it, and whether it lies within (16 (r - 1))^2 of that k's centre (fill) or not (outline)."""
    pts = np.asarray(pts, dtype=np.float32)
    covered = np.zeros((h, w), bool)
    who = np.zeros((h, w), np.int64)
    inner = np.zeros((h, w), bool)
    ok = drawn(pts)
    py, px = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing='ij')
    for k in range(pts.shape[0] - 1, -1, -1):                     # descending: the lowest k is written last
        if not ok[k]:
            continue
        cx, cy = int(centre16(pts[k, 0], w)), int(centre16(pts[k, 1], h))
        d2 = (16 * px - cx) ** 2 + (16 * py - cy) ** 2
        hit = d2 <= (16 * radius) ** 2
        covered |= hit
        who[hit] = k
        inner[hit] = (d2 <= (16 * (radius - 1)) ** 2)[hit]
    return covered, who, inner


def draw_markers(frame, pts, colors, radius):
    """frame uint8 [H, W, 3] (changed in place and returned), pts float32 [K, 2], colors uint8 [K, 3]"""
    if radius < 1:
        return frame
    covered, who, inner = marker_layers(pts, frame.shape[0], frame.shape[1], radius)
    frame[covered & inner] = np.asarray(colors, np.uint8)[who[covered & inner]]
    frame[covered & ~inner] = 0
    return frame


def quantise_colors(colors):
    """FinalModel.colors (float in [0, 1], [K, 3]) -> the uint8 marker colours: trunc(c * 255)"""
    return np.trunc(np.asarray(colors, dtype=np.float64) * 255.0).astype(np.uint8)


def cell_frames(canvas, first, seq, row, col, premap, pts_first=None, pts_seq=None, colors=None, radius=0):
    """canvas uint8 [B, T+1, rows*H, cols*W, 3] (changed in place and returned); first float32 [B,H,W,C], seq float32 [B,T,H,W,C], C in (1, 3);
    pts_first [B,K,2], pts_seq [B,T,K,2], colors uint8 [K,3] when radius >= 1."""
    b, t, h, w, c = seq.shape
    assert first.shape == (b, h, w, c) and canvas.dtype == np.uint8 and canvas.shape[:2] == (b, t + 1) and canvas.shape[4] == 3 and c in (1, 3)
    assert canvas.shape[2] % h == 0 and canvas.shape[3] % w == 0 and (row + 1) * h <= canvas.shape[2] and (col + 1) * w <= canvas.shape[3]
    q = QUANTISERS[premap]
    frames = np.empty((b, t + 1, h, w, 3), np.uint8)
    frames[:, 0] = q(first)                                        # (C = 1 broadcasts)
    frames[:, 1:] = q(seq)
    if radius >= 1:
        for i in range(b):
            draw_markers(frames[i, 0], pts_first[i], colors, radius)
            for j in range(t):
                draw_markers(frames[i, j + 1], pts_seq[i, j], colors, radius)
    canvas[:, :, row * h:(row + 1) * h, col * w:(col + 1) * w, :] = frames
    return canvas
