"""numpy restatement of the motion metrics (evaluate.py --motion-metrics): the integer accumulators and the diversity
of D draws of 8-bit frames in int64 (metrics_ref.png8 is the quantisation), the key-point error and diversity in float64 in the kernel's
order of operations.  numpy only: the CPU tests check it against the sum over pairs, the GPU tests hold the kernels to it."""
import numpy as np

from metrics_ref import png8

MAX_DRAWS = 4096


def moments(draws):
    """draws: D arrays of one shape in [-1,1] -> (sum q, sum q^2) as int64 arrays of that shape, q = png8(draw)."""
    s = ss = 0
    for x in draws:
        q = png8(x).astype(np.int64)
        s, ss = s + q, ss + q * q
    return s, ss


def pair_sums(s, ss, d):
    """V = D * sum q^2 - (sum q)^2 = sum over the pairs i < j of draws of (q_i - q_j)^2, int64"""
    s, ss = np.asarray(s, np.int64), np.asarray(ss, np.int64)
    return d * ss - s * s


def pair_sums_brute_force(q):
    """The same from the D draws themselves, q integer [D, ...]: the sum over the pairs, one by one."""
    q = np.asarray(q, np.int64)
    v = np.zeros(q.shape[1:], np.int64)
    for i in range(q.shape[0]):
        for j in range(i + 1, q.shape[0]):
            v += (q[i] - q[j]) ** 2
    return v


def draw_diversity(s, ss, d, frame_shape):
    """Accumulators of d draws of N frames [H,W,C] (flat or shaped) -> (div_mse float32 [N], std_map uint8 [N,H,W])."""
    h, w, c = frame_shape
    v = pair_sums(s, ss, d).reshape(-1, h, w, c)
    total = [int(x) for x in v.reshape(v.shape[0], -1).sum(axis=1)]                      # python integers: exact
    denom = np.float64(d * (d - 1) // 2 * 65025) * np.float64(h * w * c)
    div_mse = np.array([np.float64(t) / denom for t in total], np.float64).astype(np.float32)
    m = 4 * v.sum(axis=3) // (c * d * d)                                                # [N,H,W], floor division of non-negative integers
    return div_mse, np.minimum(255, isqrt_array(m)).astype(np.uint8)


def isqrt_array(m):
    """floor(sqrt(m)) of non-negative int64 values below 2^62, exactly (math.isqrt element by element, without the Python loop)"""
    m = np.asarray(m, np.int64)
    r = np.floor(np.sqrt(m.astype(np.float64))).astype(np.int64)
    r = r - (r * r > m)
    return r + ((r + 1) * (r + 1) <= m)


def _dist(a, b):
    dx = a[..., 0].astype(np.float64) - b[..., 0].astype(np.float64)
    dy = a[..., 1].astype(np.float64) - b[..., 1].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.sqrt(dx * dx + dy * dy)


def keypoint_draw_metrics(pts, real):
    """pts float32 [D,N,T,K,2], real float32 [N,T,K,2] -> (l2 float64 [D,N,T], div float64 [N,T] or None for D == 1), before the rounding to
    float32: one float64 chain per output, k ascending for l2 and (i, j, k) ascending for div."""
    pts, real = np.asarray(pts, np.float32), np.asarray(real, np.float32)
    d, n, t, k, _ = pts.shape
    with np.errstate(invalid='ignore', over='ignore'):
        l2 = np.zeros((d, n, t), np.float64)
        for kk in range(k):
            l2 = l2 + _dist(pts[:, :, :, kk], real[None, :, :, kk])
        l2 = l2 / np.float64(k)
        if d == 1:
            return l2, None
        acc = np.zeros((n, t), np.float64)
        for i in range(d):
            for j in range(i + 1, d):
                for kk in range(k):
                    acc = acc + _dist(pts[i, :, :, kk], pts[j, :, :, kk])
        div = acc * 2.0 / (np.float64(d) * np.float64(d - 1) * np.float64(k))
    return l2, div


def within_one_ulp(got, want64):
    """got float32 against the float64 expectation: at most 1 float32 ulp of the expected value apart, non-finite values equal in kind."""
    got = np.asarray(got, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        want = np.asarray(want64, np.float64).astype(np.float32)
    fin = np.isfinite(want)
    if not np.array_equal(np.isfinite(got), fin):
        return False
    if not (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])):
        return False
    ulp = np.spacing(np.abs(want[fin]))
    return bool((np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) <= ulp.astype(np.float64)).all())
