"""float64 / longdouble restatement of evaluate.py --frechet, numpy only and written without kpx_amd.frechet:

    pool        p[n, c] = mean over the H * W positions of f[n, :, :, c]
    descriptor  per rollout of T pooled frames  v = concat(mean_t p_t, mean_{t < T-1} |p_{t+1} - p_t|)
    moments     n, sum_m x_m, sum_m x_m x_m^T;  mean = sum / n,  cov = (outer - n mean mean^T) / (n - 1)  (None for n < 2)
    distance    |m1 - m2|^2 + tr C1 + tr C2 - 2 sum_i sqrt(max(l_i, 0)),  l = eigvalsh(S C2 S),  S = C1^(1/2) by eigh, clamped at 0

The CPU tests hold kpx_amd.frechet to the closed forms of the distance, the GPU tests hold the kernels, the scorer and evaluate.py to this."""
import numpy as np

LD = np.longdouble


def pool(f, dtype=np.float64):
    f = np.asarray(f)
    n, h, w, c = f.shape
    return (f.astype(dtype).reshape(n, h * w, c).sum(axis=1) / dtype(h * w))


def descriptor(pooled, frames_per_video):
    p = np.asarray(pooled, np.float64)
    p = p.reshape(-1, frames_per_video, p.shape[1])
    if frames_per_video > 1:
        motion = np.abs(np.diff(p, axis=1)).mean(axis=1)
    else:
        motion = np.zeros_like(p[:, 0])
    return np.concatenate([p.mean(axis=1), motion], axis=1)


def moments(x, sum0=None, outer0=None):
    """-> (sum, outer) in longdouble: the optional starting values plus the rows' contributions"""
    x = np.asarray(x).astype(LD)
    s = x.sum(axis=0)
    o = np.einsum('mi,mj->ij', x, x)
    if sum0 is not None:
        s = s + np.asarray(sum0).astype(LD)
    if outer0 is not None:
        o = o + np.asarray(outer0).astype(LD)
    return s, o


def abs_moments(x, sum0=None, outer0=None):
    """the same sums over absolute values: the scale of the rounding-error bound"""
    return moments(np.abs(np.asarray(x)), None if sum0 is None else np.abs(sum0), None if outer0 is None else np.abs(outer0))


def stats(rows):
    """{n, mean, cov} of float64 rows [n, D], two-pass (the textbook form, not the one-pass form the accumulators use)"""
    x = np.asarray(rows, np.float64)
    n = x.shape[0]
    mean = x.mean(axis=0)
    if n < 2:
        return {'n': n, 'mean': mean, 'cov': None}
    d = x - mean
    return {'n': n, 'mean': mean, 'cov': d.T @ d / (n - 1)}


def distance(m1, c1, m2, c2):
    if c1 is None or c2 is None:
        return float('nan')
    m1, c1, m2, c2 = (np.asarray(v, np.float64) for v in (m1, c1, m2, c2))
    w, v = np.linalg.eigh(c1)
    s = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    lam = np.linalg.eigvalsh(s @ c2 @ s)
    return float(((m1 - m2) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


def scale(m1, c1, m2, c2):
    """tr C1 + tr C2 + |m1 - m2|^2: what an error of the distance is measured against"""
    return float(np.trace(c1) + np.trace(c2) + ((np.asarray(m1) - np.asarray(m2)) ** 2).sum())
