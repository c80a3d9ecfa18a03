"""Restatements, seeded inputs, case lists and bounds for the streaming kernels of csrc/pointwise.hip that the batch-norm, key-point and loss
suites leave out: the x2 bilinear resize (fp32 / bf16, forward / backward), the 2x2 max-pool and its gradient, the one-pass VGG feature
gradient, the VGG input transform, the activation backward, the casts / channel copies, axpy and fill.

Plain numpy.  Every restatement takes ``dtype``: float64 is the reference, float32 repeats the kernel's expression in the kernel's order of
operations, so that the result can be held to the kernel BIT FOR BIT.  Why that is possible:

* resize forward: ``top = tl + (tr - tl) * tx; bot = bl + (br - bl) * tx; r = top + (bot - top) * ty`` with tx, ty in {0, 0.5}.  A product with 0
  or 0.5 is exact for normal numbers (no rounding, only the exponent moves), so fma(d, t, tl) rounds the same real number as the separate multiply
  and add: whether the compiler contracts the expression or not, the bits are the same.  (Subnormals are kept out of the seeded data: half of
  an odd subnormal is not representable.)
* resize backward: sequential fp32 accumulation over a = 0..2 (rows), b = 0..2 (columns) of wy[a] * wx[b] * dy[2i-1+a][2j-1+b]; taps with
  oy < 0 or ox < 0 are skipped; the weights are 0.5, 1, and 1 (not 0.5) at the clamped last row / column, so every product is with 0.25, 0.5
  or 1: exact, and the fma equals an fp32 add.
* pools and feature gradient: comparisons, at most one fp32 add (dy_pooled + l1) and one fp32 product (g = gscale_host * *gscale_dev).
* vgg_prep_bwd (* 127.5), act_bwd relu / leaky / none (* 0, * 0.01, * 1), copy, fill: at most one rounding each.
* bf16 entries: the fp32 restatement, then round-to-nearest-even to bf16 (to_bf16 below: integer bit operations; tests/test_streaming_cpu.py
  holds it to torch.Tensor.bfloat16()).

Three operations may legitimately be evaluated two ways in fp32 (contracted into an fma or not) and are held to a bound around float64
instead, u = 2^-24, every rounding of either evaluation counted, second-order terms covered by the factor (1 + 4u):

* kpx_vgg_prep_fwd_f32: out = ((x + 1) / 2 * 255) - mean, the means being the fp32 constants the kernel holds.  a = fl(x + 1): u |x + 1|; the
  halving is exact; p = fl(a/2 * 255): u 127.5 |x + 1| more, and 127.5 times the error of a; r = fl(p - mean): u |r|.  Contracted, p is not
  rounded.  Bound: u (255 |x + 1| + |ref|) (1 + 4u).
* kpx_act_bwd_f32, tanh: dz = g * (1 - v * v).  q = fl(v v): u v^2; s = fl(1 - q): u |1 - v^2|; contracted, only s is rounded; dz = fl(g s):
  u |g| |1 - v^2|.  Bound: u |g| (v^2 + 2 |1 - v^2|) (1 + 4u).
* kpx_axpy_f32: y + a x.  fl(a x): u |a x|, then the sum u |y + a x|; as an fma only the latter.  Bound: u (|a x| + |y + a x|) (1 + 4u).

The pool and feature-gradient restatements implement the rule the kernel documents: the gradient goes to the FIRST maximum of the window in
row-major order (strict ``>`` from -inf), out-of-image taps of an odd H or W never win and are never written, and
``d = [pred > 0] * ((first max ? dy_pooled : 0) + l1)`` with l1 = -g, +g or 0 by the sign of gt - pred.

Seeded inputs make the edges certain: tie data is drawn from {0, 1, 2} with all 15 patterns of "which window positions hold the maximum"
planted (and asserted), all-zero windows, gt == pred elements; the bf16 data carries fp32 values exactly half-way between bf16 neighbours at both
parities of the kept bit, values around the largest bf16, +-inf, +-0 and (kinds 0 and 3) a NaN.

SLIPS lists wrong restatements (``slip=`` of the function concerned); tests/test_streaming_cpu.py shows each rejected on the GPU test's cases.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SLACK = 1.0 + 4 * U
VGG_MEAN_BGR = np.array([103.939, 116.779, 123.68], F32)         # the kernel's fp32 constants
GHOST, GDEV = 0.01, 0.37                                          # gscale_host, *gscale_dev
LRELU = F32(0.01)
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3


# ----------------------------------------------------------------------------------------------- bf16
def bf16_bits(x):
    """fp32 -> the 16 bits of the nearest bf16, ties to even (NaN: quiet bit set; its payload is not compared anywhere)."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = np.isnan(np.asarray(x, F32))
    return np.where(nan, (u >> 16).astype(np.uint32) | 0x40, r).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(F32)


def to_bf16(x, slip=None):
    """fp32 values rounded to bf16, as fp32.  slip 'bf16_trunc': the low 16 bits dropped."""
    if slip == 'bf16_trunc':
        return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xffff0000)).view(F32)
    return from_bf16_bits(bf16_bits(x))


def _bits(words):
    return np.array(words, np.uint32).view(F32)


# fp32 inputs of a cast and the bf16 bits they must round to
HALFWAY = _bits([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,          # exactly half-way: kept bit 0 -> down (even), kept bit 1 -> up (even)
                 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001,          # one fp32 unit to either side of half-way
                 0x7f7e8000, 0x7f7effff, 0x7f7f0000, 0x7f7f7fff, 0x7f7f8000,   # around the largest bf16 (the last one rounds to infinity)
                 0x7f800000, 0xff800000, 0x00000000, 0x80000000,          # +-inf, +-0
                 0x00800000, 0x42c88000, 0xc2c98000])                     # the smallest normal, two more ties
HALFWAY_BF16 = np.array([0x3f80, 0x3f82, 0xbf80, 0xbf82, 0x3f80, 0x3f81, 0x3f81, 0x3f82, 0x7f7e, 0x7f7f, 0x7f7f, 0x7f7f, 0x7f80,
                         0x7f80, 0xff80, 0x0000, 0x8000, 0x0080, 0x42c8, 0xc2ca], np.uint16)


def worst(err, bound):
    """max |err| / bound; an exact result counts as 0 whatever the bound, a NaN as infinity."""
    err, bound = np.abs(np.asarray(err, F64)).ravel(), np.asarray(bound, F64).ravel()
    if err.size == 0:
        return 0.0
    if np.any(np.isnan(err)):
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.max(np.where(err == 0, 0.0, err / bound)))


def differing(got, want):
    """Number of elements whose fp32 bits differ from the restatement's; where that has a NaN the other side must have one too (the payload of
    a NaN is not compared).  This is the count tests/test_streaming_gpu.py demands to be 0."""
    g, w = np.ascontiguousarray(got, dtype=F32).ravel(), np.ascontiguousarray(want, dtype=F32).ravel()
    assert g.shape == w.shape, (g.shape, w.shape)
    nan = np.isnan(w)
    return int(np.count_nonzero(g.view(np.uint32)[~nan] != w.view(np.uint32)[~nan]) + np.count_nonzero(~np.isnan(g[nan])))


def fma32(a, b, c):
    """fl32(a b + c) with one rounding, through float64: a b is exact there (48 bits); the sum is rounded to 53 bits first, which moves the
    fp32 result only when it lands within 2^-29 units of a tie."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


# ----------------------------------------------------------------------------------------------- resize x2 (legacy TF sampling)
def _taps(n_in, dtype, slip, axis):
    o = np.arange(2 * n_in)
    if slip == 'half_pixel':                         # src = (dst + 0.5) / 2 - 0.5 in place of dst / 2
        src = np.maximum((o + 0.5) / 2 - 0.5, 0.0)
        lo = np.floor(src).astype(np.int64)
        t = (src - lo).astype(dtype)
    else:
        lo, t = o >> 1, np.where(o & 1, 0.5, 0.0).astype(dtype)
    hi = np.minimum(lo + 1, n_in - 1)
    if slip == 'no_clamp_last_row' and axis == 0:    # row H of the image = row 0 of the next one (modelled as a wrap)
        hi = (lo + 1) % n_in
    return lo, hi, t


def resize2x_fwd(x, dtype=F64, slip=None):
    """[N,H,W,C] -> [N,2H,2W,C]: out[2i] = in[i], out[2i+1] = in[i] + (in[min(i+1, n-1)] - in[i]) * 0.5, along x first, then y."""
    x = np.asarray(x, dtype)
    ylo, yhi, ty = _taps(x.shape[1], dtype, slip, 0)
    xlo, xhi, tx = _taps(x.shape[2], dtype, slip, 1)
    tx, ty = tx[None, None, :, None], ty[None, :, None, None]
    r0, r1 = x[:, ylo], x[:, yhi]
    tl, tr, bl, br = r0[:, :, xlo], r0[:, :, xhi], r1[:, :, xlo], r1[:, :, xhi]
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    return top + (bot - top) * ty


def resize2x_bwd(dy, dtype=F64, slip=None):
    """[N,2H,2W,C] -> [N,H,W,C], the kernel's tap order.  slip 'bwd_neg_tap': the oy = -1 tap of the first row is read (weight 0) -- in front of
    image 0 lies the guard, a NaN; in front of the others a finite row that 0 annihilates."""
    dy = np.asarray(dy, dtype)
    n, h2, w2, c = dy.shape
    h, w = h2 // 2, w2 // 2
    iy, ix = np.arange(h), np.arange(w)
    last = 0.5 if slip == 'bwd_last_half' else 1.0
    wy = [np.where(iy >= 1, 0.5, 0.0), np.ones(h), np.where(iy == h - 1, last, 0.5)]
    wx = [np.where(ix >= 1, 0.5, 0.0), np.ones(w), np.where(ix == w - 1, 1.0, 0.5)]
    acc = np.zeros((n, h, w, c), dtype)
    with np.errstate(invalid='ignore'):
        for a in range(3):
            oy = 2 * iy - 1 + a
            for b in range(3):
                ox = 2 * ix - 1 + b
                wgt = (wy[a][:, None] * wx[b][None, :]).astype(dtype)[None, :, :, None]
                v = dy[:, np.maximum(oy, 0)][:, :, np.maximum(ox, 0)]
                valid = ((oy >= 0)[:, None] & (ox >= 0)[None, :])[None, :, :, None]
                if slip == 'bwd_neg_tap' and a == 0:
                    v = v.copy()
                    v[0, oy < 0] = np.nan
                    valid = (ox >= 0)[None, None, :, None] & np.ones((1, h, 1, 1), bool)
                acc = np.where(valid, acc + wgt * v, acc)
    return acc


# ----------------------------------------------------------------------------------------------- max-pool 2x2 s2 SAME, feature gradient
def _windows(x):
    """[N,H,W,C] -> values [4,N,Ho,Wo,C] in scan order (-inf outside the image) and the validity [4,1,Ho,Wo,1] of each tap."""
    n, h, w, c = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    xp = np.full((n, 2 * ho, 2 * wo, c), -np.inf, x.dtype)
    xp[:, :h, :w] = x
    okp = np.zeros((1, 2 * ho, 2 * wo, 1), bool)
    okp[:, :h, :w] = True
    pick = lambda a: np.stack([a[:, 0::2, 0::2], a[:, 0::2, 1::2], a[:, 1::2, 0::2], a[:, 1::2, 1::2]])
    return pick(xp), pick(okp)


def first_max(x, slip=None):
    """Index 0..3 of the window position that takes the gradient, per [N,Ho,Wo,C]."""
    v, ok = _windows(np.asarray(x))
    best, bi = np.full(v.shape[1:], -np.inf, v.dtype), np.zeros(v.shape[1:], np.int64)
    for k in range(4):
        upd = ((v[k] >= best) if slip == 'tie_last' else (v[k] > best)) & ok[k]
        best, bi = np.where(upd, v[k], best), np.where(upd, k, bi)
    return bi, best


def maxpool2_fwd(x, dtype=F64):
    return first_max(np.asarray(x, dtype))[1]


def maxpool2_bwd(dy, x, dtype=F64, slip=None):
    """dx [N,H,W,C]: dy at the first maximum of each window, +0 at every other in-image position."""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    n, h, w, c = x.shape
    bi, _ = first_max(x, slip)
    dxp = np.zeros((n, 2 * bi.shape[1], 2 * bi.shape[2], c), dtype)
    for k in range(4):
        dxp[:, (k >> 1)::2, (k & 1)::2] = np.where(bi == k, dy, dtype(0))
    return dxp[:, :h, :w]


def gscale(host, devv, dtype=F64):
    """g = gscale_host * *gscale_dev: one fp32 product (times 1 without a device scalar)."""
    return dtype(F32(host)) * dtype(F32(1.0 if devv is None else devv))


def vgg_feat_bwd(gt, pred, g, dyp=None, dtype=F64, slip=None):
    """Gradient at a VGG feature y = relu(conv): gt, pred [B,H,W,C], dyp [B,Ho,Wo,C] or None."""
    gt, pred, g = np.asarray(gt, dtype), np.asarray(pred, dtype), dtype(g)
    df = gt - pred
    if slip == 'l1_sign':
        df = -df
    l1 = np.where(df > 0, -g, np.where(df < 0, g, dtype(0))).astype(dtype)
    mask = (gt if slip == 'relu_from_gt' else pred) > 0
    if dyp is None:
        return np.where(mask, l1, dtype(0))
    pooled = maxpool2_bwd(dyp, pred, dtype, slip)
    if slip == 'l1_dropped_with_pool':
        first = maxpool2_bwd(np.ones_like(np.asarray(dyp, dtype)), pred, dtype) > 0
        return np.where(mask, np.where(first, pooled, l1), dtype(0))
    return np.where(mask, pooled + l1, dtype(0))


# ----------------------------------------------------------------------------------------------- VGG input transform
def vgg_prep_fwd(rgb, dtype=F64, slip=None, contracted=False):
    """rgb [P,3] in [-1,1] -> bgr on the 0..255 scale minus the mean.  contracted (fp32 only): p * 255 - mean as one fma."""
    x = np.asarray(rgb, dtype)
    half = (x + dtype(1)) / dtype(2)
    mean = VGG_MEAN_BGR.astype(dtype)
    if slip != 'prep_no_swap':
        half = half[:, ::-1]
    if contracted:
        assert dtype == F32
        return fma32(half, F32(255), -mean)
    return half * dtype(255) - mean


def vgg_prep_fwd_bound(rgb):
    x = np.asarray(rgb, F64)
    return U * (255.0 * np.abs(x + 1.0)[:, ::-1] + np.abs(vgg_prep_fwd(rgb))) * SLACK


def vgg_prep_bwd(dbgr, dtype=F64, slip=None):
    return np.asarray(dbgr, dtype)[:, ::-1] * dtype(255.0 if slip == 'prep_bwd_255' else 127.5)


# ----------------------------------------------------------------------------------------------- activation backward, axpy, casts
def act_bwd(dy, y, act, dtype=F64, slip=None, contracted=False):
    """dz = dy * act'(y) from the ACTIVATED tensor: y > 0 ? dy : dy * neg (neg = 1, 0, 0.01: the sign of a zero follows dy); tanh
    dy * (1 - y y).  contracted (fp32, tanh): 1 - y y as one fma."""
    g, v = np.asarray(dy, dtype), np.asarray(y, dtype)
    if act == ACT_TANH:
        if contracted:
            assert dtype == F32
            return g * fma32(-v, v, F32(1))
        return g * (dtype(1) - v * v)
    neg = dtype({ACT_NONE: F32(1), ACT_RELU: F32(0), ACT_LRELU: LRELU}[act])
    pos = (v >= 0) if slip == 'leaky_at_zero' else (v > 0)
    return np.where(pos, g, g * neg)


def tanh_bwd_bound(dy, y):
    g, v = np.asarray(dy, F64), np.asarray(y, F64)
    return U * np.abs(g) * (v * v + 2 * np.abs(1 - v * v)) * SLACK


def axpy(y, x, a, dtype=F64, contracted=False):
    y, x, a = np.asarray(y, dtype), np.asarray(x, dtype), dtype(F32(a))
    if contracted:
        assert dtype == F32
        return fma32(a, x, y)
    return y + a * x


def axpy_bound(y, x, a):
    ax = np.asarray(x, F64) * F64(F32(a))
    return U * (np.abs(ax) + np.abs(np.asarray(y, F64) + ax)) * SLACK


def cast(src, kind, slip=None):
    """kpx_cast_channels on [P,C] values held as fp32: kind 0 rounds, 1 and 2 keep the value, 3 rounds and pads to 8 channels with +0."""
    src = np.asarray(src, F32)
    if kind in (1, 2):
        return src.copy()
    out = to_bf16(src, slip)
    if kind == 3:
        out = np.concatenate([out, np.zeros((src.shape[0], 8 - src.shape[1]), F32)], axis=1)
    return out


# ----------------------------------------------------------------------------------------------- seeded inputs
def _seed(tag, shape):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(tag))] + [int(s) for s in shape])


def no_subnormals(a):
    a = np.abs(np.asarray(a, F32))
    return bool(np.all((a == 0) | (a >= np.finfo(F32).tiny) | ~np.isfinite(a)))


def normal(tag, shape, bf16=False):
    x = _seed(tag, shape).standard_normal(shape).astype(F32)
    x = to_bf16(x) if bf16 else x
    assert no_subnormals(x)
    return x


PATTERNS = [tuple(bool(m >> k & 1) for k in range(4)) for m in range(1, 16)]      # which window positions hold the maximum


def max_patterns(x):
    """The set of patterns that occur among the FULL windows of x [N,H,W,C]."""
    n, h, w, c = x.shape
    if h < 2 or w < 2:
        return set()
    v, _ = _windows(np.asarray(x[:, :h // 2 * 2, :w // 2 * 2], F64))
    hit = (v == v.max(axis=0)).reshape(4, -1).T
    return set(map(tuple, hit.tolist()))


def full_windows(shape):
    n, h, w, c = shape
    return n * (h // 2) * (w // 2) * c


def tie_features(shape):
    """A post-ReLU feature on the grid {0, 1, 2}.  With 16 full windows or more: each of the 15 patterns planted in one (asserted), and one
    all-zero window; smaller shapes keep the random grid values, which tie by themselves."""
    rng = _seed('ties', shape)
    x = rng.integers(0, 3, size=shape).astype(F32)
    n, h, w, c = shape
    if full_windows(shape) >= 16:
        spots = [(i, oy, ox, ch) for i in range(n) for oy in range(h // 2) for ox in range(w // 2) for ch in range(c)]
        order = rng.permutation(len(spots))[:16]
        for pat, s in zip(PATTERNS + [None], order):
            i, oy, ox, ch = spots[s]
            top = int(rng.integers(1, 3))
            for k in range(4):
                val = 0 if pat is None else (top if pat[k] else int(rng.integers(0, top)))
                x[i, 2 * oy + (k >> 1), 2 * ox + (k & 1), ch] = val
        assert max_patterns(x) >= set(PATTERNS), 'a maximum pattern is missing from the tie case'
        v, _ = _windows(x[:, :h // 2 * 2, :w // 2 * 2])
        assert np.any(v.max(axis=0) == 0), 'no all-zero window'
    return x


def features(kind, shape, bf16=False):
    """(gt, pred) halves of a feature tensor.  'ties': both on {0, 1, 2}, a third of gt equal to pred (l1 exactly 0).  'cont': relu(N(0,1)),
    a tenth of gt equal to pred."""
    rng = _seed('feat' + kind, shape)
    if kind == 'ties':
        pred = tie_features(shape)
        gt = rng.integers(0, 3, size=shape).astype(F32)
        same = rng.random(shape) < 1 / 3
    else:
        pred = np.maximum(rng.standard_normal(shape), 0).astype(F32)
        gt = np.maximum(rng.standard_normal(shape), 0).astype(F32)
        same = rng.random(shape) < 0.1
        if bf16:
            pred, gt = to_bf16(pred), to_bf16(gt)
    gt = np.where(same, pred, gt)
    assert np.any((gt == pred) & (pred > 0)) or pred.size < 64
    assert no_subnormals(pred) and no_subnormals(gt)
    return gt, pred


def pooled_gradient(shape, bf16=False):
    """dy_pooled for a feature of ``shape``.  bf16: half of it in +-[1, 2), where half a bf16 unit is 2^-8 = 0.0039: above |l1| = g = 0.0037
    with the device scalar (the sum rounds back to dy_pooled) and below g = 0.01 without it (it moves to a neighbour); the rest N(0, 1)."""
    n, h, w, c = shape
    ps = (n, (h + 1) // 2, (w + 1) // 2, c)
    rng = _seed('dyp', shape)
    d = rng.standard_normal(ps).astype(F32)
    if bf16:
        big = rng.random(ps) < 0.5
        d = to_bf16(np.where(big, np.copysign(1 + rng.random(ps), d), d).astype(F32))
    assert no_subnormals(d)
    return d


def cast_values(P, C, bf16_exact=False, nan=False):
    """[P,C] fp32 with the half-way values planted from the front (as many as fit).  bf16_exact: the source of kinds 1 and 2 (already bf16)."""
    x = _seed('cast', (P, C)).standard_normal((P, C)).astype(F32) * F32(3)
    flat = x.reshape(-1)
    k = min(HALFWAY.size, flat.size - 1)
    flat[:k] = HALFWAY[:k]
    if bf16_exact:
        with np.errstate(over='ignore'):
            x = to_bf16(x)
    elif nan:
        flat[-1] = np.nan
    return x


def act_values(n, bf16=False):
    """(dy, y): y with +0, -0, +-1e-30 and +-1 at the front, else tanh-like values in (-1, 1); dy N(0, 1) with both signs at the zeros."""
    rng = _seed('act', (n,))
    y = np.tanh(rng.standard_normal(n) * 1.5).astype(F32)
    dy = rng.standard_normal(n).astype(F32)
    front = np.array([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 0.0, -0.0], F32)
    k = min(n, front.size)
    y[:k] = front[:k]
    if n >= 8:
        dy[:8] = np.abs(dy[:8]) * np.array([1, 1, 1, 1, 1, 1, -1, -1], F32)        # a negative gradient at +0 and -0: dz = -0 under ReLU
    if bf16:
        y, dy = to_bf16(y), to_bf16(dy)
    assert no_subnormals(y) and no_subnormals(dy)
    return dy, y


def prep_values(P):
    x = _seed('prep', (P,)).uniform(-1, 1, (P, 3)).astype(F32)
    x[0] = [-1.0, 0.0, 1.0]
    if P > 3:
        x[1], x[2], x[3] = [1.0, -1.0, 0.0], [0.0, 1.0, -1.0], [-1.0, -1.0, -1.0]
    return x


# ----------------------------------------------------------------------------------------------- cases (N, H, W, C)
# the smallest shapes that reach each branch; ld = pixel stride (default C), lead = words in front of every buffer of the call
RESIZE_F32 = {
    'quad_2x5x7x16_ldy24': dict(shape=(2, 5, 7, 16), ldy=24),
    'quad_1x1x1x4': dict(shape=(1, 1, 1, 4)),
    'quad_3x1x9x8_ldx12': dict(shape=(3, 1, 9, 8), ldx=12),
    'quad_2x6x1x4': dict(shape=(2, 6, 1, 4)),
    'scalar_2x3x5x3': dict(shape=(2, 3, 5, 3)),                   # C % 4
    'scalar_2x3x5x8_ldy10': dict(shape=(2, 3, 5, 8), ldy=10),     # ld % 4
    'scalar_1x2x3x4_lead': dict(shape=(1, 2, 3, 4), lead=1),      # 4-byte-offset base
}
RESIZE_BF16 = {
    '2x5x7x16_ld24': dict(shape=(2, 5, 7, 16), ldy=24),
    '1x1x1x8': dict(shape=(1, 1, 1, 8)),
    '2x1x6x8': dict(shape=(2, 1, 6, 8)),
    '2x6x1x8': dict(shape=(2, 6, 1, 8)),
}
POOL_F32 = {
    'vec_2x7x9x8': dict(shape=(2, 7, 9, 8)),
    'scalar_2x7x9x3': dict(shape=(2, 7, 9, 3)),
    'vec_1x1x5x4': dict(shape=(1, 1, 5, 4)),
    'vec_1x5x1x4': dict(shape=(1, 5, 1, 4)),
    'vec_3x1x1x4': dict(shape=(3, 1, 1, 4)),
    'scalar_2x4x6x4_lead': dict(shape=(2, 4, 6, 4), lead=1),
}
POOL_BF16 = [(2, 4, 6, 8), (1, 2, 2, 16)]
FEAT_F32 = [(2, 7, 9, 4), (1, 1, 1, 4), (2, 4, 6, 8)]
FEAT_BF16 = [(2, 4, 6, 8), (1, 2, 2, 16)]
FEAT_BF16_FLAT = [(2, 3, 5, 8)]                                   # odd sizes are fine without dy_pooled
PREP_P = [1, 257]
ACT_N = [1, 3, 4, 5, 1027]
ACT_N_BF16 = [8, 1032]
AXPY_N, AXPY_A = [1, 1027], [1.0, -0.5, 1.0 / 3.0]
FILL_N = [0, 1, 1027]
CAST_VEC = (37, 16, 24, 16)                                       # (P, C, ldsrc, lddst)
CAST_SCALAR = (37, 5, 7, 6)
CAST_PAD_C = [1, 4, 8]
COPY = {'vec_ldsrc': (37, 8, 12, 8), 'vec_lddst': (37, 8, 8, 16), 'scalar_c5': (37, 5, 7, 6), 'scalar_ld': (37, 8, 10, 8), 'flat': (37, 4, 4, 4)}

# capped grids: 2048 blocks x 256 items in one sweep, so 723 x 726 = 2048 * 256 + 610 items make a second, ragged one
SWEEP = 2048 * 256
CAP_HW = (723, 726)
CAP_FILL = SWEEP + 77
# the two input-pixel resize forwards sweep 16384 x 256 items: 2047 x 2051 = 16384 * 256 + 4093
SWEEP_FWD = 16384 * 256
CAP_FWD_HW = (2047, 2051)
assert CAP_HW[0] * CAP_HW[1] == SWEEP + 610 and CAP_FWD_HW[0] * CAP_FWD_HW[1] == SWEEP_FWD + 4093


def resize_input(name_or_shape, bf16=False):
    shape = name_or_shape if isinstance(name_or_shape, tuple) else {**RESIZE_F32, **RESIZE_BF16}[name_or_shape]['shape']
    return normal('resize_x', shape, bf16)


def resize_gradient(shape, bf16=False):
    n, h, w, c = shape
    return normal('resize_dy', (n, 2 * h, 2 * w, c), bf16)


# ----------------------------------------------------------------------------------------------- planted slips
# name -> what goes wrong; each is the ``slip`` argument of the restatement it belongs to
SLIPS = {
    'half_pixel': 'resize forward samples at half-pixel centres (weights 0.25 / 0.75)',
    'no_clamp_last_row': 'resize forward reads row H instead of clamping to H - 1',
    'bwd_last_half': 'resize backward gives the clamped last row the weight 0.5',
    'bwd_neg_tap': 'resize backward reads the oy = -1 tap (weight 0) instead of skipping it',
    'tie_last': 'the gradient goes to the LAST maximum of a window',
    'relu_from_gt': 'the ReLU mask of the feature gradient is taken from the gt half',
    'l1_sign': 'the L1 gradient has the wrong sign',
    'l1_dropped_with_pool': 'l1 is dropped where dy_pooled arrives',
    'bf16_trunc': 'bf16 stores truncate instead of rounding',
    'prep_no_swap': 'the VGG transform keeps RGB order',
    'prep_bwd_255': 'the VGG transform backward scales by 255',
    'leaky_at_zero': 'the activation backward treats y == 0 as positive',
}


# ----------------------------------------------------------------------------------------------- what the GPU test expects, bit for bit
def expect_resize_fwd(x, bf16=False, slip=None):
    r = resize2x_fwd(x, F32, slip)
    return to_bf16(r, slip) if bf16 else r


def expect_resize_bwd(dy, bf16=False, slip=None):
    r = resize2x_bwd(dy, F32, slip)
    return to_bf16(r, slip) if bf16 else r


def expect_feat(gt, pred, host, devv, dyp, bf16=False, slip=None):
    r = vgg_feat_bwd(gt, pred, gscale(host, devv, F32), dyp, F32, slip)
    return to_bf16(r, slip) if bf16 else r


def expect_act(dy, y, act, bf16=False, slip=None):
    r = act_bwd(dy, y, act, F32, slip)
    return to_bf16(r, slip) if bf16 else r


def pool_inputs(shape, kind):
    """The tensor a pool case runs on: 'cont' N(0, 1) (no ties), 'ties' the grid {0, 1, 2}."""
    return tie_features(shape) if kind == 'ties' else normal('pool_x', shape)


def pool_gradient(shape):
    n, h, w, c = shape
    return normal('pool_dy', (n, (h + 1) // 2, (w + 1) // 2, c))
