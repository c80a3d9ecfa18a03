"""numpy float64 restatement of the two kernels of csrc/stability.hip (make_pseudo_labels.py --stability), operation for
operation in the kernels' order: numpy rounds every product and sum once, as the kernels do (no fma).  numpy only: the CPU tests check it on
cases whose answer is known exactly, the GPU tests hold the kernels to it -- the warp bit for bit, the scores within one float32 ulp (the
device's float64 square root is not promised to be correctly rounded)."""
import numpy as np


def _axis(s, size):
    """clamp, integer part lowered to size - 2 at the far edge, fraction, neighbour"""
    hi = np.float64(size - 1)
    with np.errstate(invalid='ignore'):
        s = np.where(s >= 0.0, np.where(s > hi, hi, s), 0.0)                # NaN -> 0
    i0 = np.floor(s).astype(np.int64)
    i0 = np.where(i0 > size - 2, max(size - 2, 0), i0)
    return i0, s - i0.astype(np.float64), np.minimum(i0 + 1, size - 1)


def affine_warp(frames, rows, coef):
    """frames float32 [N,H,W,C], rows int [R], coef float64 [R,6] (the inverse maps in pixel units) -> float32 [R,H,W,C]"""
    frames, coef = np.asarray(frames, np.float32), np.asarray(coef, np.float64)
    n, h, w, c = frames.shape
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    out = np.empty((len(rows), h, w, c), np.float32)
    for r, src in enumerate(rows):
        m = coef[r]
        with np.errstate(invalid='ignore', over='ignore'):
            sx = (m[0] * x + m[1] * y) + m[2]
            sy = (m[3] * x + m[4] * y) + m[5]
        x0, fx, x1 = _axis(sx, w)
        y0, fy, y1 = _axis(sy, h)
        v = frames[int(src)].astype(np.float64)
        fx, fy = fx[..., None], fy[..., None]
        gx, gy = 1.0 - fx, 1.0 - fy
        top = gx * v[y0, x0] + fx * v[y0, x1]
        bot = gx * v[y1, x0] + fx * v[y1, x1]
        out[r] = (gy * top + fy * bot).astype(np.float32)
    return out


# inverse maps in pixel units that send the pixels of a 16 x 16 frame to pixels: the warp copies input bits
EXACT = {'identity': [1.0, 0, 0, 0, 1.0, 0], 'shift': [1.0, 0, -3.0, 0, 1.0, 2.0], 'flip': [-1.0, 0, 15.0, 0, 1.0, 0],
         'quarter': [0, 1.0, 0, -1.0, 0, 15.0]}


def exact_case(name, f):
    """What the map EXACT[name] makes of the 16 x 16 frames f [N,16,16,C], by indexing alone."""
    if name == 'identity':
        return f
    if name == 'shift':                                       # out(x, y) = in(x - 3, y + 2), edges replicated
        xs, ys = np.clip(np.arange(16) - 3, 0, 15), np.clip(np.arange(16) + 2, 0, 15)
        return f[:, ys][:, :, xs]
    if name == 'flip':                                        # out(x, y) = in(15 - x, y)
        return f[:, :, ::-1]
    return np.transpose(f[:, ::-1], (0, 2, 1, 3))             # quarter turn: out(x, y) = in(y, 15 - x)


def equivariance_scores(pts, pts_w, rows, fwd):
    """pts float32 [N,K,2], pts_w float32 [R,K,2], rows int [R], fwd float64 [R,6] -> (scores float64 [R,K,2] = (err, moved) before the
    rounding to float32, valid uint8 [R,K], frame_mean float64 [R,2] before the rounding, n_valid int32 [R])"""
    pts, pts_w, fwd = np.asarray(pts, np.float32), np.asarray(pts_w, np.float32), np.asarray(fwd, np.float64)
    p, q = pts[np.asarray(rows, np.int64)].astype(np.float64), pts_w.astype(np.float64)
    m = fwd[:, None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        tx = (m[..., 0] * p[..., 0] + m[..., 1] * p[..., 1]) + m[..., 2]
        ty = (m[..., 3] * p[..., 0] + m[..., 4] * p[..., 1]) + m[..., 5]
        dx, dy, ux, uy = q[..., 0] - tx, q[..., 1] - ty, tx - p[..., 0], ty - p[..., 1]
        err, moved = np.sqrt(dx * dx + dy * dy), np.sqrt(ux * ux + uy * uy)
        valid = (np.isfinite(p).all(axis=-1) & np.isfinite(q).all(axis=-1) & (tx >= -1.0) & (tx <= 1.0) & (ty >= -1.0) & (ty <= 1.0))
    r, k = valid.shape
    s_err, s_moved = np.zeros(r, np.float64), np.zeros(r, np.float64)
    for kk in range(k):                                                     # ascending k, one chain per row
        s_err = s_err + np.where(valid[:, kk], err[:, kk], 0.0)
        s_moved = s_moved + np.where(valid[:, kk], moved[:, kk], 0.0)
    n = valid.sum(axis=1).astype(np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(n[:, None] > 0, np.stack([s_err, s_moved], axis=1) / n[:, None].astype(np.float64), np.nan)
    return np.stack([err, moved], axis=-1), valid.astype(np.uint8), mean, n


def targets(pts, rows, fwd):
    """The mapped originals, float64 [R,K,2] (the scores' `target`)."""
    p, m = np.asarray(pts, np.float32)[np.asarray(rows, np.int64)].astype(np.float64), np.asarray(fwd, np.float64)[:, None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([(m[..., 0] * p[..., 0] + m[..., 1] * p[..., 1]) + m[..., 2],
                         (m[..., 3] * p[..., 0] + m[..., 4] * p[..., 1]) + m[..., 5]], axis=-1)
