"""Restatement of csrc/resample.hip in numpy float64, operation by operation in the order include/kpx.h writes them, one rounding to fp32 at
the end; and of kpx_points_speed_f64 in longdouble.  numpy only."""
import numpy as np

LINEAR, CUBIC = 0, 1
MODES = {'linear': LINEAR, 'cubic': CUBIC}


def knots(first, seq):
    """first [B,K,2], seq [B,N,K,2] -> the knots P_0..P_N as fp32 [B,N+1,K,2]"""
    first, seq = np.asarray(first, np.float32), np.asarray(seq, np.float32)
    return np.concatenate([first[:, None], seq], 1)


def stencil(i, n, mode):
    """The knots an in-between frame of the interval [i, i+1] reads (0 <= i < n)"""
    if mode == LINEAR:
        return [i, i + 1]
    return [j for j in (i - 1, i, i + 1, i + 2) if 0 <= j <= n]


def resample(first, seq, rate, mode):
    """-> fp32 [B,N*rate,K,2]; frame j = 1..N*rate at index j - 1.  r == 0: the knot's bits.  Otherwise fp64, every operation on its own."""
    p32 = knots(first, seq)
    p = p32.astype(np.float64)
    b, n1, k, _ = p.shape
    n = n1 - 1
    out = np.empty((b, n * rate, k, 2), np.float32)
    with np.errstate(all='ignore'):
        for j in range(1, n * rate + 1):
            i, r = divmod(j, rate)
            if r == 0:
                out[:, j - 1] = p32[:, i]
                continue
            s = np.float64(r) / np.float64(rate)
            a, c = p[:, i], p[:, i + 1]
            if mode == LINEAR:
                out[:, j - 1] = (a + s * (c - a)).astype(np.float32)
                continue
            s2 = s * s
            s3 = s2 * s
            h00 = (2.0 * s3 - 3.0 * s2) + 1.0
            h10 = (s3 - 2.0 * s2) + s
            h01 = -2.0 * s3 + 3.0 * s2
            h11 = s3 - s2
            m0 = c - a if i == 0 else (c - p[:, i - 1]) / 2.0
            m1 = c - a if i + 1 == n else (p[:, i + 2] - a) / 2.0
            out[:, j - 1] = (((h00 * a + h10 * m0) + h01 * c) + h11 * m1).astype(np.float32)
    return out


def speed(first, seq, scale=1.0):
    """-> longdouble [B,T]: scale * mean_k |P_t[k] - P_{t-1}[k]|, P_0 = first"""
    p = knots(first, seq).astype(np.longdouble)
    d = p[:, 1:] - p[:, :-1]
    return np.longdouble(scale) * (np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).sum(-1) / np.longdouble(p.shape[2]))


def ulp_distance(a, b):
    """Distance in fp32 ulps between two fp32 arrays of finite values (0 where the bits are equal)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return np.abs(key(a) - key(b))
