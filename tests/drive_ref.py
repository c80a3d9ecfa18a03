"""numpy restatement of kpx_points_retarget_f32 (FinalModel.run(drive=...)): the key-point sequence of a driven rollout
in float64, in the kernel's order of operations, rounded to float32 once.  numpy only: the CPU tests check its degenerate cases, the GPU
tests hold the kernel to it."""
import numpy as np

MODES = ('hold', 'absolute', 'relative')


def spread(p):
    """p float32 [K,2] -> sum_k |p_k - c|^2 with c = (sum_k p_k) / K, float64, both sums in the order k = 0..K-1"""
    p = np.asarray(p, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.zeros(2, np.float64)
        for k in range(p.shape[0]):
            s = s + p[k]
        c = s / np.float64(p.shape[0])
        v = np.float64(0.0)
        for k in range(p.shape[0]):
            d = p[k] - c
            v = v + (d[0] * d[0] + d[1] * d[1])
    return v


def scale(src, drv):
    """s = sqrt(v_src / v_drv) of two constellations [K,2] when both spreads are finite and > 0, else 1"""
    vs, vd = spread(src), spread(drv)
    if np.isfinite(vs) and np.isfinite(vd) and vs > 0 and vd > 0:
        return np.sqrt(vs / vd)
    return np.float64(1.0)


def retarget(src_first, mode, drv_first=None, drv_seq=None, shift=0, scaled=False, frames=None):
    """src_first float32 [B,K,2]; drv_first [B,K,2] and drv_seq [B,T,K,2] for 'absolute' / 'relative'; ``frames`` = T for 'hold'
    -> float32 [B,T,K,2]; sample b is driven by sample (b + shift) mod B."""
    assert mode in MODES and not (scaled and mode != 'relative')
    src_first = np.asarray(src_first, np.float32)
    b, k, _ = src_first.shape
    assert 0 <= shift < b
    if mode == 'hold':
        return np.ascontiguousarray(np.broadcast_to(src_first[:, None], (b, frames, k, 2)))
    drv_seq = np.asarray(drv_seq, np.float32)
    j = (np.arange(b) + shift) % b
    if mode == 'absolute':
        return np.ascontiguousarray(drv_seq[j])
    drv_first = np.asarray(drv_first, np.float32)
    out = np.empty(drv_seq.shape, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(b):
            delta = drv_seq[j[i]].astype(np.float64) - drv_first[j[i]].astype(np.float64)[None]
            if scaled:
                delta = scale(src_first[i], drv_first[j[i]]) * delta
            out[i] = (src_first[i].astype(np.float64)[None] + delta).astype(np.float32)
    return out
