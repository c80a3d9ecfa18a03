"""Restatements, seeded inputs and error bounds for the loss, optimiser and rollout kernels
(csrc/loss_optim.hip, the head blend of csrc/pointwise.hip, csrc/rollout.hip); shared by test_loss_optim_cpu.py,
test_loss_optim_gpu.py and test_rollout_ops_gpu.py.

Every restatement is plain numpy and takes ``dtype``: float64 is the reference, float32 evaluates the same formulas in the
precision of the kernels (the CPU suite holds that evaluation to the bounds below, so a bound no fp32 code could meet cannot
sit here unnoticed).  Sums are accumulated in float64 under either dtype, as the kernels do.  Scalars that cross the C ABI as
``float`` (Adam's alpha, eps, gscale, 1-beta; the labels) are rounded to fp32 first.

Bounds (fixed before measuring): the bar of this suite's pointwise kernels, 16 fp32 ulps of the magnitudes involved plus 1e-30
(tests/test_motion_ops_gpu.py).  A result computed as 1 - mask counts at magnitude 1: it inherits the rounding of mask.
  Adam            m' 16e(|m|+|gr|) ; v' 16e(|v|+gr^2) ; p' 2e|p| + 16e*alpha(|m|+|gr|)/(sqrt(v'_64)+eps)     (gr = gscale*g)
  cross-entropy   group mean 16e*mean(max(x,0)+|x z|+log1p(e^-|x|)), out[0] both plus e|out[0]| ; gradient 16e(sigmoid(x)+|z|)|g|/n
  pair L1         forward 4e*ref (subtraction, fp32 pair sum, final cast: one rounding each, every term non-negative; through
                  ops.l1_mean the product with the scale is the fourth) ; gradient exact: -g, 0 or +g with g = ghost*gdev rounded once
  head blend      final 16e(|im| mask + |raw|) ; mask 16e*mask ; crude the bits of raw (of clamp(raw) for the clipped tiled entry) ;
                  d raw[0:3] 16e|g| ; d raw[3] 16e*mask*sum|g|(|im|+|raw|) ; clip is 1-Lipschitz: clip(got) against clip(ref) keeps
                  the unclipped bound
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TINY = 1e-30
F32 = np.float32


def _f32(x):
    """A scalar as the C ABI receives it: rounded to fp32 (returned as a Python float)."""
    return float(F32(x))


# ----------------------------------------------------------------------------------------------- Adam
BETA1, BETA2, ADAM_EPS, LR = 0.5, 0.999, 1e-8, 1e-4
ADAM_GRID_ELEMS = 2048 * 256 * 4                      # one pass of the capped grid: past it the grid-stride loop runs
ADAM_SIZES = (1, 3, 4, 5, 1003, 4100, ADAM_GRID_ELEMS + 1027)
ADAM_GSCALES = (1.0, 0.125, 1.0 / 3.0)
ADAM_KINDS = ('zero', 'tiny', 'huge', 'cancel')


def adam_alpha(step, lr=LR, beta1=BETA1, beta2=BETA2):
    """ApplyAdam's step size lr*sqrt(1-b2^t)/(1-b1^t) with the beta powers kept as fp32 variables (step counts from 1)."""
    b1p, b2p = F32(beta1), F32(beta2)
    for _ in range(step - 1):
        b1p, b2p = F32(b1p * F32(beta1)), F32(b2p * F32(beta2))
    return float(F32(F32(lr) * np.sqrt(F32(1) - b2p) / (F32(1) - b1p)))


def adam_step(p, g, m, v, alpha, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, gscale=1.0, dtype=np.float64):
    """One ApplyAdam step -> (p', m', v')."""
    omb1, omb2 = dtype(F32(1) - F32(beta1)), dtype(F32(1) - F32(beta2))
    a, e, gs = dtype(_f32(alpha)), dtype(_f32(eps)), dtype(_f32(gscale))
    p, g, m, v = (np.asarray(x).astype(dtype) for x in (p, g, m, v))
    gr = gs * g
    m2 = m + (gr - m) * omb1
    v2 = v + (gr * gr - v) * omb2
    p2 = p - m2 * a / (np.sqrt(v2) + e)
    return p2, m2, v2


def adam_bounds(p, g, m, v, alpha, eps=ADAM_EPS, gscale=1.0):
    """(bound p', bound m', bound v') around the float64 step on these fp32 inputs."""
    p, g, m, v = (np.asarray(x).astype(np.float64) for x in (p, g, m, v))
    gr = _f32(gscale) * g
    v2 = adam_step(p, g, m, v, alpha, eps=eps, gscale=gscale)[2]
    mag = np.abs(m) + np.abs(gr)
    bp = 2 * EPS32 * np.abs(p) + 16 * EPS32 * _f32(alpha) * mag / (np.sqrt(v2) + _f32(eps)) + TINY
    return bp, 16 * EPS32 * mag + TINY, 16 * EPS32 * (np.abs(v) + gr * gr) + TINY


def adam_state(n, seed=0):
    """(p, m, v) fp32: a running state in the first half, the zero state of a fresh optimiser in the second."""
    rs = np.random.RandomState(1000 + seed)
    p = rs.randn(n).astype(F32)
    m = (0.1 * rs.randn(n)).astype(F32)
    v = ((0.1 * rs.randn(n)) ** 2).astype(F32)
    m[n // 2:] = 0
    v[n // 2:] = 0
    return p, m, v


def adam_grad(n, step, seed=0):
    return (0.1 * np.random.RandomState(2000 + 10 * seed + step).randn(n)).astype(F32)


def adam_planted(n):
    """kind -> indices: the first after element 0 and, from 16 elements on, the last (the scalar tail of an n % 4 != 0 bucket)."""
    out = {}
    for k, kind in enumerate(ADAM_KINDS):
        idx = [1 + k] if 1 + k < n else []
        if n >= 16:
            idx.append(n - 1 - k)
        out[kind] = np.array(idx, dtype=np.int64)
    return out


def adam_plant(g, m, v, gscale):
    """Copies of (g, m, v) with the special elements planted:  zero: g = m = v = 0 (the update must leave p, m, v bit-unchanged);
    tiny: g = 1e-20 (g^2 is subnormal);  huge: g = 1e15;  cancel: m = -gscale*g (m' is a pure cancellation)."""
    g, m, v = g.copy(), m.copy(), v.copy()
    idx = adam_planted(g.size)
    g[idx['zero']] = 0
    m[idx['zero']] = 0
    v[idx['zero']] = 0
    g[idx['tiny']] = 1e-20
    g[idx['huge']] = 1e15
    m[idx['cancel']] = -(F32(gscale) * g[idx['cancel']])
    return g, m, v, idx


# ----------------------------------------------------------------------------------------------- sigmoid cross-entropy
XENT_SIZES = ((72, 72), (1, 0), (300, 0), (5, 300), (257, 255), (4608, 4608))
XENT_RAW_SIZE = (0, 7)                                 # an empty first group: reachable through the C ABI only
XENT_LABELS = ((1.0, 0.0), (0.0, 1.0), (0.9, 0.1))
XENT_SPECIALS = (100.0, -100.0, 20.0, -20.0, 0.0, 1e-10)


def xent_logits(n0, n1, seed=0):
    """3*randn with saturated (+-100, +-20), zero and tiny logits planted (in both groups where they fit)."""
    n = n0 + n1
    x = (3.0 * np.random.RandomState(3000 + 7 * n0 + n1 + seed).randn(n)).astype(F32)
    for k, s in enumerate(XENT_SPECIALS):
        if n > 8:
            x[1 + k::max(n // 2 - 3, 8)] = s
        elif 1 + k < n:
            x[1 + k] = s
    if n == 1:
        x[0] = -20.0
    return x


def _xent_terms(x, z, dtype):
    return np.maximum(x, dtype(0)) - x * z + np.log1p(np.exp(-np.abs(x)))


def _labels(n0, z0, n1, z1, dtype):
    return np.concatenate([np.full(n0, _f32(z0)), np.full(n1, _f32(z1))]).astype(dtype)


def xent_fwd(x, n0, z0, n1, z1, dtype=np.float64):
    """[m0 + m1, m0, m1]: the means of sigmoid_cross_entropy_with_logits over the two label groups (an empty group counts 0)."""
    x = np.asarray(x).astype(dtype)
    l = _xent_terms(x, _labels(n0, z0, n1, z1, dtype), dtype)
    m0 = dtype(l[:n0].sum(dtype=np.float64) / n0) if n0 else dtype(0)
    m1 = dtype(l[n0:].sum(dtype=np.float64) / n1) if n1 else dtype(0)
    return np.array([m0 + m1, m0, m1], dtype=dtype)


def xent_bwd(x, n0, z0, n1, z1, g, dtype=np.float64):
    """d (g * out[0]) / d x."""
    x = np.asarray(x).astype(dtype)
    cnt = np.concatenate([np.full(n0, n0), np.full(n1, n1)]).astype(dtype)
    sg = _sigmoid(x, dtype)
    return (sg - _labels(n0, z0, n1, z1, dtype)) * (dtype(_f32(g)) / cnt)


def xent_fwd_bounds(x, n0, z0, n1, z1):
    x = np.asarray(x).astype(np.float64)
    z = _labels(n0, z0, n1, z1, np.float64)
    mag = np.maximum(x, 0) + np.abs(x * z) + np.log1p(np.exp(-np.abs(x)))
    b0 = 16 * EPS32 * mag[:n0].mean() + TINY if n0 else 0.0
    b1 = 16 * EPS32 * mag[n0:].mean() + TINY if n1 else 0.0
    total = xent_fwd(x, n0, z0, n1, z1)[0]
    return np.array([b0 + b1 + EPS32 * abs(total), b0, b1])


def xent_bwd_bounds(x, n0, z0, n1, z1, g):
    x = np.asarray(x).astype(np.float64)
    cnt = np.concatenate([np.full(n0, n0), np.full(n1, n1)]).astype(np.float64)
    sg = 1.0 / (1.0 + np.exp(-x))
    return 16 * EPS32 * (sg + np.abs(_labels(n0, z0, n1, z1, np.float64))) * abs(_f32(g)) / cnt + TINY


# ----------------------------------------------------------------------------------------------- pair L1
L1_FWD_GRID_ELEMS = 1024 * 256 * 4                    # forward block cap x 256 lanes x 4 floats; the backward cap is 2048 * 256
L1_SIZES = (1, 3, 4, 1027, L1_FWD_GRID_ELEMS + 2052, L1_FWD_GRID_ELEMS + 2053)        # 1 050 628 (vector), 1 050 629 (scalar)
L1_TIE_FIRST, L1_TIE_EVERY = 2, 9
# kpx_l1_pair_fwd_bf16 takes multiples of 8 only: the sizes above rounded up, and one past its own cap of 1024 * 256 * 8
L1_BF16_SIZES = (8, 1032, L1_FWD_GRID_ELEMS + 2056, 2 * L1_FWD_GRID_ELEMS + 1032)


def l1_pair_inputs(half, seed=0):
    """[gt | pred] fp32, every 9th pair from the third on equal (gradient exactly 0 there)."""
    rs = np.random.RandomState(4000 + seed + half % 1000)
    f = rs.randn(2 * half).astype(F32)
    f[half + L1_TIE_FIRST::L1_TIE_EVERY] = f[L1_TIE_FIRST:half:L1_TIE_EVERY]
    return f


def l1_pair_fwd(f, half, dtype=np.float64):
    f = np.asarray(f).astype(dtype)
    return dtype(np.abs(f[:half] - f[half:]).sum(dtype=np.float64) / half)


def l1_pair_bwd(f, half, ghost, gdev=1.0):
    """d (ghost*gdev * sum|gt - pred|) / d pred, exactly: g is the fp32 product rounded once, sign(0) = 0."""
    f = np.asarray(f).astype(np.float64)
    g = F32(F32(ghost) * F32(gdev))
    d = f[:half] - f[half:]
    return np.where(d > 0, -g, np.where(d < 0, g, F32(0))).astype(F32)


def l1_fwd_bound(ref):
    return 4 * EPS32 * abs(float(ref))


def to_bf16(a):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32 values."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(F32)


# ----------------------------------------------------------------------------------------------- head blend
BLEND_SHAPES = ((1, 1, 1), (1, 15, 17), (1, 1, 257), (9, 256, 256))          # P = 1, 255, 257 and 589 824 > 2048 * 256
TILED_SHAPES = ((1, 1, 3, 5), (2, 3, 7, 9), (2, 32, 16, 16), (3, 32, 37, 41))        # (B, T, h, w)
TILED_SEED = 1     # with it every tiled shape has >= 1/4 of the blended and >= 1/2 of the raw values outside [-1, 1] (asserted by the tests)


def blend_inputs(n_im, n, h, w, seed=0):
    """(im [n_im,h,w,3] in [-1,1], raw4 [n,h,w,4], g [n,h,w,3]): |raw| > 1 on most elements, mask logits saturated at +-40 and +-100
    and in the range [10, 18] where 1 - mask has lost most of its bits."""
    rs = np.random.RandomState(5000 + seed + n * h * w % 997)
    im = rs.uniform(-1, 1, (n_im, h, w, 3)).astype(F32)
    raw = (3.0 * rs.randn(n, h, w, 4)).astype(F32)
    logit = (2.0 * rs.randn(n * h * w)).astype(F32)
    logit[4::5] = rs.uniform(10, 18, logit[4::5].shape)
    logit[::7] = 40.0
    logit[1::11] = -40.0
    logit[2::13] = 100.0
    logit[3::17] = -100.0
    raw[..., 3] = logit.reshape(n, h, w)
    g = rs.randn(n, h, w, 3).astype(F32)
    return im, raw, g


def _sigmoid(x, dtype):
    with np.errstate(over='ignore'):                            # e^100 is inf in fp32 and the quotient 0, as on the device
        return dtype(1) / (dtype(1) + np.exp(-x))


def blend_fwd(im, raw, dtype=np.float64):
    """-> (final, crude, mask)"""
    im, raw = np.asarray(im).astype(dtype), np.asarray(raw).astype(dtype)
    mask = _sigmoid(raw[..., 3:], dtype)
    return im * mask + raw[..., :3] * (dtype(1) - mask), raw[..., :3], mask


def blend_bwd(g, im, raw, dtype=np.float64):
    """d sum(g * final) / d raw4"""
    g, im, raw = (np.asarray(x).astype(dtype) for x in (g, im, raw))
    mask = _sigmoid(raw[..., 3:], dtype)
    dm = (g * (im - raw[..., :3])).sum(-1, keepdims=True)
    return np.concatenate([g * (dtype(1) - mask), dm * mask * (dtype(1) - mask)], -1)


def blend_tiled_fwd(im, raw, t, clip=True, dtype=np.float64):
    """Frame f blends image f // t; with clip, final and crude go through clip_by_value(-1, 1)."""
    fin, crude, mask = blend_fwd(np.repeat(np.asarray(im), t, axis=0), raw, dtype)
    if clip:
        fin, crude = np.clip(fin, dtype(-1), dtype(1)), np.clip(crude, dtype(-1), dtype(1))
    return fin, crude, mask


def blend_fwd_bounds(im, raw):
    """(bound final, bound mask); im already tiled to the frames of raw."""
    im, raw = np.asarray(im).astype(np.float64), np.asarray(raw).astype(np.float64)
    mask = _sigmoid(raw[..., 3:], np.float64)
    return 16 * EPS32 * (np.abs(im) * mask + np.abs(raw[..., :3])) + TINY, 16 * EPS32 * mask + TINY


def blend_bwd_bounds(g, im, raw):
    g, im, raw = (np.asarray(x).astype(np.float64) for x in (g, im, raw))
    mask = _sigmoid(raw[..., 3:], np.float64)
    s = (np.abs(g) * (np.abs(im) + np.abs(raw[..., :3]))).sum(-1, keepdims=True)
    return np.concatenate([16 * EPS32 * np.abs(g), 16 * EPS32 * mask * s], -1) + TINY


# ----------------------------------------------------------------------------------------------- rollout: tiling, LSTM cell, dense
TILE_CASES = ((3, 32, 1, 30), (2, 32, 1, 80), (1, 1, 5, 4), (2, 3, 7, 6), (3, 32, 256, 128))          # (B, T, pix, C)
TILE_SLICE_CASE, TILE_SLICE_LD, TILE_SLICE_OFFSETS = (2, 4, 64, 128), 160, (0, 4, 2)
LSTM_CELL_SHAPES = ((3, 30, 1024), (16, 80, 1024), (1, 80, 1024), (2, 7, 13))                           # (bsz, In, U)
DENSE_SHAPES = ((3, 103, 32), (16, 1024, 80))                                                           # (rows, In, Out)
DENSE_ACTS = (0, 1, 3)                                                                                  # none, relu, tanh


def tile_batch(x, t):
    """tf.tile over a new time axis + reshape: [B, ...] -> [B*T, ...], row b*T + s is x[b]."""
    return np.repeat(np.asarray(x), t, axis=0)


def tile_input(b, pix, c):
    """All values distinct and exact in fp32: a wrong source index cannot pass."""
    return (np.arange(b * pix * c, dtype=np.float64) + 0.5).astype(F32).reshape(b, pix, c)


def lstm_cell_inputs(bsz, n_in, u, seed=0):
    rs = np.random.RandomState(6000 + seed + bsz + n_in + u)
    lim = np.sqrt(6.0 / (n_in + 5 * u))                         # glorot_uniform of the [In+U, 4U] kernel
    x = rs.uniform(-1, 1, (bsz, n_in)).astype(F32)
    h = rs.uniform(-1, 1, (bsz, u)).astype(F32)
    c = rs.randn(bsz, u).astype(F32)
    kernel = rs.uniform(-lim, lim, (n_in + u, 4 * u)).astype(F32)
    bias = (0.1 * rs.randn(4 * u)).astype(F32)
    return x, h, c, kernel, bias


def lstm_cell(x, h, c, kernel, bias, forget_bias=1.0, dtype=np.float64):
    """One tf.nn.rnn_cell.LSTMCell step (gate order i, j, f, o) -> (h', c')."""
    x, h, c, kernel, bias = (np.asarray(a).astype(dtype) for a in (x, h, c, kernel, bias))
    i, j, f, o = np.split(np.concatenate([x, h], 1) @ kernel + bias, 4, axis=1)
    c2 = c * _sigmoid(f + dtype(forget_bias), dtype) + _sigmoid(i, dtype) * np.tanh(j)
    return np.tanh(c2) * _sigmoid(o, dtype), c2


def dense_inputs(rows, n_in, n_out, seed=0):
    rs = np.random.RandomState(7000 + seed + rows + n_in + n_out)
    x = rs.randn(rows, n_in).astype(F32)
    w = (rs.randn(n_in, n_out) / np.sqrt(n_in)).astype(F32)
    b = (0.5 * rs.randn(n_out)).astype(F32)
    return x, w, b


def dense(x, w, b, act=0, dtype=np.float64):
    z = np.asarray(x).astype(dtype) @ np.asarray(w).astype(dtype) + np.asarray(b).astype(dtype)
    return {0: z, 1: np.maximum(z, dtype(0)), 3: np.tanh(z)}[act]


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def worst(err, bound):
    """max of |err| / bound: what the tests print next to each assertion."""
    return float(np.max(np.abs(np.asarray(err, np.float64)) / np.asarray(bound, np.float64)))
