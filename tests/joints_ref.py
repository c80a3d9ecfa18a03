"""numpy float64 restatement of the three kernels of csrc/joints.hip (make_pseudo_labels.py --joints), written as loops
over the frames in the kernels' order.  numpy rounds every product and sum once, as the targets and scores kernels do (no fma).  The moments
kernel adds each frame with ONE fma per element: with ``math.fma`` (Python >= 3.13) ``moments_add(..., fused=True)`` restates that bit for
bit, element by element (slow: small shapes only); without it the product is rounded before the sum.  For float32 key points and targets
the product of two of them is exact in float64 (48 bits), so both forms give the same bits; for other inputs they differ by at most one
rounding of the running sum per frame, which is what ``moments_abs`` bounds.  numpy only: runs without a GPU."""
import math

import numpy as np

HAVE_FMA = hasattr(math, 'fma')


def features(pts):
    """pts float32 [F,K,2] -> (phi float64 [F,2K+1], finite bool [F])"""
    pts = np.asarray(pts, np.float32)
    f = pts.shape[0]
    phi = np.concatenate([pts.reshape(f, -1).astype(np.float64), np.ones((f, 1), np.float64)], axis=1)
    return phi, np.isfinite(phi).all(axis=1)


def joint_targets(xy, vis, bbox, cmap):
    """xy float32 [F,J,2], vis uint8 [F,J], bbox float32 [F,4], cmap float64 [4] -> (target float64 [F,J,2] before the rounding to float32,
    mask uint8 [F,J], norm float64 [F] before the rounding)"""
    xy, bbox, cmap = np.asarray(xy, np.float32).astype(np.float64), np.asarray(bbox, np.float32).astype(np.float64), np.asarray(cmap, np.float64)
    ax, bx, ay, by = cmap
    with np.errstate(invalid='ignore', over='ignore'):
        tx, ty = ax * xy[..., 0] + bx, ay * xy[..., 1] + by
        mask = ((np.asarray(vis) != 0) & np.isfinite(xy[..., 0]) & np.isfinite(xy[..., 1])
                & (tx >= -1.0) & (tx <= 1.0) & (ty >= -1.0) & (ty <= 1.0))
        ok = np.isfinite(bbox).all(axis=1) & (bbox[:, 2] > bbox[:, 0]) & (bbox[:, 3] > bbox[:, 1])
        w, h = abs(ax) * (bbox[:, 2] - bbox[:, 0]), abs(ay) * (bbox[:, 3] - bbox[:, 1])
        norm = np.where(ok, np.where(w > h, w, h), np.nan)
    return np.stack([tx, ty], axis=-1), mask.astype(np.uint8), norm


def moments_add(pts, target, mask, G, Bm, n, fused=False):
    """The accumulators after the frames pts float32 [F,K,2], target float32 [F,J,2], mask uint8 [F,J], starting from G [J,D,D], Bm [J,D,2],
    n [J] (not modified) -> (G, Bm, n).  Frames in ascending order; a frame counts for joint j when mask[f,j] is set and its key points are
    finite.  ``fused``: one ``math.fma`` per element and frame, the kernel's bits."""
    phi, fin = features(pts)
    target, mask = np.asarray(target, np.float32).astype(np.float64), np.asarray(mask) != 0
    G, Bm, n = np.array(G, np.float64), np.array(Bm, np.float64), np.array(n, np.int64)
    d = phi.shape[1]
    for f in range(phi.shape[0]):
        if not fin[f]:
            continue
        use = np.nonzero(mask[f])[0]
        if fused:
            for j in use:
                for a in range(d):
                    for b in range(d):
                        G[j, a, b] = math.fma(phi[f, a], phi[f, b], G[j, a, b])
                    for c in range(2):
                        Bm[j, a, c] = math.fma(phi[f, a], target[f, j, c], Bm[j, a, c])
        else:
            G[use] = G[use] + np.outer(phi[f], phi[f])[None]
            Bm[use] = Bm[use] + phi[f][None, :, None] * target[f, use][:, None, :]
        n[use] += 1
    return G, Bm, n


def moments_abs(pts, target, mask):
    """(sum_f |use phi_a phi_b| [J,D,D], sum_f |use phi_a t_c| [J,D,2]): what the error bound of the moments scales with."""
    phi, fin = features(pts)
    target = np.asarray(target, np.float32).astype(np.float64)
    use = ((np.asarray(mask) != 0) & fin[:, None]).astype(np.float64)
    phi = np.where(fin[:, None], phi, 0.0)
    target = np.where(use[..., None] > 0, target, 0.0)
    a = np.abs(phi)
    return np.einsum('fj,fa,fb->jab', use, a, a), np.einsum('fj,fa,fjc->jac', use, a, np.abs(target))


def joint_scores(pts, target, mask, norm, W, alpha):
    """-> (pred float64 [F,J,2], err float64 [F,J] (both before the rounding to float32), hits uint8 [F,J], sum_err float64 [J], count,
    pck_count int64 [J], hit_count int64 [J,A], valid bool [F,J], pck bool [F,J])"""
    phi, fin = features(pts)
    target, mask = np.asarray(target, np.float32).astype(np.float64), np.asarray(mask) != 0
    norm, W, alpha = np.asarray(norm, np.float32).astype(np.float64), np.asarray(W, np.float64), np.asarray(alpha, np.float64)
    f, d = phi.shape
    j = W.shape[0]
    pred = np.zeros((f, j, 2), np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(d):                                                  # ascending d: every product and sum rounded once
            pred = pred + phi[:, i, None, None] * W[None, :, i, :]
        dx, dy = pred[..., 0] - target[..., 0], pred[..., 1] - target[..., 1]
        err = np.sqrt(dx * dx + dy * dy)
        valid = mask & fin[:, None]
        pck = valid & np.isfinite(norm)[:, None]
        hit = pck[..., None] & (err[..., None] <= alpha[None, None, :] * norm[:, None, None])
    hits = (hit.astype(np.uint16) << np.arange(len(alpha), dtype=np.uint16)).sum(axis=-1).astype(np.uint8)
    sum_err = np.zeros(j, np.float64)
    for i in range(f):                                                      # ascending f, one chain per joint
        sum_err = sum_err + np.where(valid[i], err[i], 0.0)
    return (pred, err, hits, sum_err, valid.sum(axis=0).astype(np.int64), pck.sum(axis=0).astype(np.int64),
            hit.sum(axis=0).astype(np.int64), valid, pck)
