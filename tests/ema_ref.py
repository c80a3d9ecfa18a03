"""The averaged generator (csrc/ema.hip, kpx_amd/ema.py) restated: the update in float64 from the float32 operands, the two float32 forms a
kernel could take, the rate schedule written a second time, and the case table of tests/test_ema_cpu.py and tests/test_ema_gpu.py.

Bound of the update, per element: |error| <= 4 fp32 ulps of S = |e| + |p|.  The uncontracted float32 form rounds three times -- d = p - e,
d * rate and the sum -- each by at most 2^-24 of a quantity that is at most S (0 <= rate <= 1), so it stays within 3 * 2^-24 * S, and one
ulp of S is at least 2^-24 * S; the form the kernel takes (d, then one fused multiply-add) rounds twice.  Results in the subnormal range
are exact sums or round by at most 2^-150, and the bound never falls below 4 * 2^-149.
"""
import numpy as np

from loss_optim_ref import ADAM_GRID_ELEMS

SIZES = (1, 5, 1003, ADAM_GRID_ELEMS + 1027)       # below one vector, the tail, and past one full pass of the capped grid
RATES = tuple(np.float32(r) for r in (0.0, np.float32(1) - np.float32(0.999), 0.9, 1.0))
DECAYS = (0.9, 0.999, 0.9999)
STEPS = (0, 1, 8, 9, 10 ** 4, 10 ** 7)
SUFFIX = '/ExponentialMovingAverage'


def rate(decay, t, warmup=True):
    """tf.train.ExponentialMovingAverage(decay, num_updates=t) -> 1 - decay', on float32 arrays (numpy's array arithmetic keeps float32)."""
    one, ten = np.ones(1, np.float32), np.full(1, 10.0, np.float32)
    d = np.array([decay]).astype(np.float32)
    if warmup:
        tt = np.array([t]).astype(np.float32)
        d = np.minimum(d, (one + tt) / (ten + tt))
    out = one - d
    assert out.dtype == np.float32
    return out[0]


def update(e, p, r):
    """e + (p - e) * rate in float64 from the float32 operands."""
    e64, p64 = np.asarray(e, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    return e64 + (p64 - e64) * np.float64(np.float32(r))


def update_f32_plain(e, p, r):
    """The uncontracted float32 form: three roundings."""
    e, p, r = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(r)
    d = (p - e).astype(np.float32)
    return (e + (d * r).astype(np.float32)).astype(np.float32)


def update_f32_fma(e, p, r):
    """d = p - e in float32, then fma(d, rate, e): the product of two float32 is exact in float64, the sum is taken in longdouble and
    rounded to float32 (a double rounding at worst half an ulp of the longdouble away from the fused result)."""
    e, p, r = np.asarray(e, np.float32), np.asarray(p, np.float32), np.float32(r)
    d = (p - e).astype(np.float32)
    prod = d.astype(np.float64) * np.float64(r)
    return (prod.astype(np.longdouble) + e.astype(np.longdouble)).astype(np.float32)


def ulp32(x):
    """Spacing of float32 at magnitude x (float64 array), 2^-149 below the normal range."""
    x = np.abs(np.asarray(x, np.float64))
    expo = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return np.exp2(np.maximum(expo, -126.0) - 23.0)


def bound(e, p):
    s = np.abs(np.asarray(e, np.float32).astype(np.float64)) + np.abs(np.asarray(p, np.float32).astype(np.float64))
    return 4.0 * ulp32(s)


def operands(n, r, seed=0):
    """(e, p) float32 [n].  By index modulo 4:  0, 3  magnitudes log-uniform from the subnormals (1e-45) to 1e38, random signs;
    1  e == p (never -0);  2  the cancelling case e ~ -p * rate / (1 - rate), whose exact result is near zero (rates 0 and 1: e = -p)."""
    rs = np.random.RandomState(1000 * seed + n % 9973)
    with np.errstate(under='ignore'):
        mag = lambda: (10.0 ** rs.uniform(-45.0, 38.0, size=n) * rs.choice([-1.0, 1.0], size=n)).astype(np.float32)
        e, p = mag(), mag()
    i = np.arange(n)
    same = i % 4 == 1
    e[same] = p[same] = np.where(p[same] == 0, np.float32(1.5), p[same])
    canc = i % 4 == 2
    pc = (rs.randn(n) * 3.0).astype(np.float32)
    r64 = float(np.float32(r))
    p[canc] = pc[canc]
    e[canc] = (-pc[canc].astype(np.float64) * (r64 / (1.0 - r64) if 0.0 < r64 < 1.0 else 1.0)).astype(np.float32)
    assert np.isfinite(e).all() and np.isfinite(p).all() and np.abs(e).max() <= 1.01e38 and np.abs(p).max() <= 1.01e38
    return e, p


def swap_operands(n, seed=0):
    """Two float32 [n] ranges as uint32 bit patterns: random words (NaNs with payloads among them), with +-Inf, -0, a quiet and a
    signalling NaN with payloads planted at the ends and in the middle."""
    rs = np.random.RandomState(77 * seed + n % 9973)
    a = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    b = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc12345, 0xff800000, 0x80000000, 0x7f800000, 0x7fa00bad, 0xffc0ffee], np.uint32)
    for k, w in enumerate(special):
        a[(k * 7) % n if k else n - 1] = w
        b[(n // 2 + k * 5) % n] = special[(k + 3) % len(special)]
    return a, b


def shadow_fixture():
    """A checkpoint dict with a fused-head pair, slots, counters and moving statistics -> (arrays, what select must return)."""
    rs = np.random.RandomState(5)
    f = lambda *s: rs.randn(*s).astype(np.float32)
    names = {'translator/conv_8_0/conv2d/kernel': (3, 3, 4, 3), 'translator/conv_8_1/conv2d/kernel': (3, 3, 4, 1),
             'pose_encoder/conv_1/conv2d/bias': (6,)}
    arrays, want = {}, {}
    for n, s in names.items():
        arrays[n], arrays[n + '/Adam'], arrays[n + '/Adam_1'], arrays[n + SUFFIX] = f(*s), f(*s), f(*s), f(*s)
        want[n] = arrays[n + SUFFIX]
    for n, s in {'img_discr/conv_1/conv2d/kernel': (3, 3, 3, 2)}.items():        # the discriminator is never averaged
        arrays[n], arrays[n + '/Adam'], arrays[n + '/Adam_1'] = f(*s), f(*s), f(*s)
        want[n] = arrays[n]
    for n in ('pose_encoder/conv_1/batch_normalization/moving_mean', 'pose_encoder/conv_1/batch_normalization/moving_variance'):
        arrays[n] = want[n] = f(6)
    for n, v in (('global_step', np.int32(41)), ('beta1_power', np.float32(0.25)), ('beta2_power', np.float32(0.998)),
                 ('beta1_power_1', np.float32(0.25)), ('beta2_power_1', np.float32(0.998))):
        arrays[n] = want[n] = np.asarray(v)
    return arrays, want
