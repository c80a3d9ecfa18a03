"""Restatements, seeded inputs and error bounds for the batch-norm entries of csrc/pointwise.hip and the channel reductions they share:
kpx_bn_train_{fwd,bwd}_{f32,bf16} (with and without ``tile_stats``), kpx_bn_invstd_f32, kpx_bn_apply_f32, kpx_bn_fold_conv_f32 and
kpx_chan_sum_{f32,bf16}; shared by test_batchnorm_cpu.py and test_batchnorm_gpu.py.

Every restatement is plain numpy and takes ``dtype``: float64 is the reference; float32 evaluates the same formulas with every operation
rounded to fp32 (the multiply-add of the output unfused, two roundings) and every sum taken SEQUENTIALLY.  The per-channel sums over the
pixels (sum x, sum x^2, sum dz, sum dz*xhat, the sums over the items of a ``tile_stats`` slab) are the one exception: the entries are
specified with double accumulators there, so the fp32 evaluation adds them sequentially in float64 and rounds what the entries round (the
mean, the variance, the sums handed on as floats).  ``slip`` plants a mistake; 'sumsq_f32' is the mistake of dropping exactly that exception.
The CPU suite holds the fp32 evaluation to the bounds below and shows that each slip is rejected.

Bounds (fixed before anything ran on a GPU).  u = 2^-24, e = 2u, D = 2^-53, DEN = 2^-149 (one fp32 denormal step, under every absolute
bound), n = terms of a double sum (P pixels, or the items of a slab).  Every sum bound is order-free.  Each stage is judged on the state the
stage before it SAVED (fp32 mean / invstd as the entry wrote them), so no bound absorbs an earlier stage's error.
  mean           u |m| + (n+4) D mean|x| + DEN
  variance       dv = (n+4) D (mean x^2 + m^2) + u v + DEN          (slab: mean|item| for mean x^2)
  invstd         max |f(v +- dv) - f(v)| + 2e f(v),  f(t) = 1/sqrt(max(t,0) + eps): dv carried through f itself, not linearised, because
                 v = 0 (constant channel, P = 1) sits on the clamp
  moving mean    reference: the float64 recurrence mm -= (mm - mean_g)(1 - decay) over the entry's saved means, in group order, decay the
                 fp32 value (1 - decay is exact in fp32); bound sum_g 3u (|mm_g| + |mean_g|) + DEN (three roundings per update; an
                 earlier update's error is carried on with factor decay < 1)
  moving var     the same with unb_g = v_g n/max(n-1,1) from float64: sum_g [3u (|mv_g| + unb_g) + (1-decay)(dv_g n/max(n-1,1) + u unb_g)] + DEN
  y              on saved mean / invstd: 4u (|xhat gamma| + |beta|) + DEN       (xhat two roundings, product, sum)
  sum dz         ds0 = (n+4) D sum|dz| + u |s0| + DEN
  sum dz xhat    ds1 = (e + (n+4) D) sum|dz xhat| + u |s1| + DEN            (e: the fp32 xhat inside every term)
                 slab form: s1 = (sum items)/gamma: ds1 = (n+4) D sum|items| / |gamma| + (u + D)|s1| + DEN; exactly 0 at gamma = 0
  dbeta, dgamma  sum_g ds_g + (t-1) u (|pre| + sum_g |s_g|), t = groups + accumulate terms added in fp32, in order
  dx             |gamma invstd| (10u T + (ds0 + |xhat| ds1)/P) + DEN, T = |dz| + |s0|/P + |xhat s1|/P: the error is relative to T, not to
                 |dx| (dz - mean dz - xhat mean(dz xhat) cancels); 10 >= the eight roundings that reach the largest term
  chan_sum       u |s| + (n+4) D sum|x| + DEN
  bn_invstd      2e / sqrt(var + eps)
  fold           w_out: 8u |w s|, b_out: 8u (|(b - mm) s| + |beta|) + DEN, s = gamma / sqrt(mv + eps)   (s is four roundings)
  bf16 entries   the fp32 bound of the same quantity + 2^-8 |value| for y and dx; mean, invstd, moving statistics, dgamma, dbeta: the fp32 bounds

One term is wider than its plain form, because a correct evaluation cannot meet the plain one:
  2^-8 |value| for a bf16 store, not 2^-9: bf16 keeps 8 significant bits, so round-to-nearest moves a value by up to half a unit in the
    last place = 2^-8 2^floor(log2 |value|), which is 2^-8 |value| just above a power of two and 2^-9 |value| only just below one.  The fp32
    evaluation followed by an exact round-to-nearest-even store misses 2^-9 |value| by a factor of 1.94-1.99 on every bf16 case.

ReLU mask.  An element is UNDECIDED when |y64| <= 2^-10 (|xhat gamma| + |beta|) and gamma != 0 (at gamma = 0 every arithmetic gives
y = beta exactly, so the mask is decided by beta alone, beta = 0 included: closed).  Every case is built so that NO element is undecided:
``make_case`` nudges offending elements away from the zero crossing and re-derives the statistics until none is left, with twice the
threshold plus the reach of an fp32 mean (4u |m| invstd |gamma|) as margin, so that the condition also holds on an entry's saved state.
The tensors of a case are used with act = 0 and act = 1 alike.

Value regimes, per channel and mixed in one tensor (channel c takes REGIMES[c % 8]; group g shifts the means):
  normal N(0.5+g, 2) | offset_a N(1e3, 1e-1) | offset_b N(-1e4, 1) | constant 3.25+g (few mantissa bits: sums and squares exact) |
  tiny N(0, 1e-20) | large N(0, 1e15) | sparse 95 % exact zeros
From C >= 12 on, channel c % 16 == 8 has gamma = beta = 0 and c % 16 == 9 has gamma = 0, beta > 0.  bf16 cases round x (and dy) to bf16
after drawing and use normal | constant | sparse | normal around 8.
"""
import numpy as np

U = 2.0 ** -24
E = 2.0 * U
D = 2.0 ** -53
DEN = 2.0 ** -149
B8 = 2.0 ** -8
F32 = np.float32
F64 = np.float64
EPS = 1e-5
DECAY = 0.99
REGIMES = ('normal', 'offset_a', 'offset_b', 'constant', 'tiny', 'large', 'sparse', 'normal')
REGIMES_BF16 = ('normal', 'constant', 'sparse', 'normal8')
SLIPS = ('sumsq_f32', 'biased_moving', 'eps_outside', 'reverse_groups', 'dgamma_x', 'drop_xhat_term', 'mean_over_all', 'relu_ge',
         'accumulate_ignored')

# name: (groups, P, C, ldx); 'lead': x / y / dx start one float into their buffers; 'dy_lead': only dy does; 'ldo': ld of y / dy / dx
CASES = {
    # vector path (C % 4 == 0, ld % 4 == 0, 16-B bases): G = C/4 channel groups, Gb = min(G,256), PPB = 256/Gb pixel rows per block
    'v_3x4': dict(shape=(1, 3, 4, 4)),                    # G = 1, PPB = 256: 253 idle rows; one block
    'v_37x32': dict(shape=(1, 37, 32, 32)),               # G = 8, PPB = 32: reduction grid 37/(32*8) -> 1, strip grid ceil(37/128) = 1, ragged trip
    'v_5x1028': dict(shape=(1, 5, 1028, 1028)),           # G = 257: blockIdx.y = 1 holds one channel group
    'v_19x64_ld96': dict(shape=(2, 19, 64, 96), ldo=80),  # ld > C on every tensor (a channel slice of a wider buffer), two groups
    'v_1x8': dict(shape=(1, 1, 8, 8)),                    # P = 1: variance 0, unbiased factor 1
    'v_big': dict(shape=(1, 8229, 1024, 1024), big=True),  # G = 256, PPB = 1: reduction grid 8229/8 = 1028 -> capped at 1024, strip grid
                                                          # ceil(8229/4) = 2058 -> capped at 2048: both loops make a second, ragged trip
    # scalar path
    's_7x5': dict(shape=(1, 7, 5, 5)),                    # C % 4 != 0; Gb = 5, PPB = 51, thread 255 idle
    's_3x257': dict(shape=(1, 3, 257, 257)),              # second blockIdx.y slice with one channel
    's_11x32_ld33': dict(shape=(1, 11, 32, 33), ldo=33),  # C % 4 == 0 but ld % 4 != 0
    's_11x32_lead': dict(shape=(1, 11, 32, 32), lead=1),  # base one float into its buffer
    's_11x32_dylead': dict(shape=(1, 11, 32, 32), dy_lead=1),   # only dy misaligned: scalar reduction; the apply pass decides on its own (scalar too)
    's_1x5': dict(shape=(1, 1, 5, 5)),                    # P = 1
    's_big': dict(shape=(1, 8229, 256, 257), ldo=257, big=True),  # Gb = 256, PPB = 1: 1028 -> 1024 blocks; apply grid_for(8229*256) -> 2048
    # groups: the finalize kernels take four groups per trip; 5 and 6 leave a partly idle second trip
    'g4x12': dict(shape=(4, 9, 12, 12)), 'g5x12': dict(shape=(5, 9, 12, 12)), 'g6x12': dict(shape=(6, 9, 12, 12)),
    'g4x6': dict(shape=(4, 9, 6, 6)), 'g5x6': dict(shape=(5, 9, 6, 6)), 'g6x6': dict(shape=(6, 9, 6, 6)),
}
# tile_stats: items per group; P = 2 * items + 3 pixels cut into `items` ragged runs
TILE_ITEMS = (1, 255, 256, 257, 600)
# bf16 entries: (groups, P, C, ldx, ldo)
CASES_BF16 = {
    'b_37x8': dict(shape=(1, 37, 8, 8)),                  # G = 1, PPB = 256
    'b_21x24_ld40': dict(shape=(2, 21, 24, 40), ldo=32),  # ld > C in multiples of 8, two groups
    'b_5x2056': dict(shape=(1, 5, 2056, 2056)),           # G = 257: second blockIdx.y slice
    'b_g5x16': dict(shape=(5, 9, 16, 16)),                # second finalize trip
}


def _f(x, dtype):
    return np.asarray(x).astype(dtype)


def to_bf16(a):
    """Round fp32 values to the nearest bf16 (ties to even); the result is fp32 with 16 low zero bits."""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return r.astype(np.uint32).view(F32).reshape(np.shape(a))


def seqsum(a, axis, dtype=F64, sequential=False):
    """Sum along ``axis`` accumulated in ``dtype``: pairwise (the float64 reference) or strictly left to right."""
    if not sequential:
        return np.sum(a, axis=axis, dtype=dtype)
    return np.take(np.cumsum(a, axis=axis, dtype=dtype), -1, axis=axis)


def worst(err, bound):
    """max |err| / bound; a NaN counts as infinite, 0/0 as 0 (an exact result under an exact bound)."""
    err, bound = np.abs(np.asarray(err, F64)), np.asarray(bound, F64)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0.0, 0.0, err / bound)
    if r.size == 0:
        return 0.0
    return float(np.inf) if np.any(np.isnan(r)) else float(r.max())


# ----------------------------------------------------------------------------------------------- restatements
def stats_from_sums(s, q, n, eps, dtype):
    """(mean, biased variance, invstd) as the entries round them: m, v in double, then fl32(m), fl32(v), 1/sqrt(fl32(v) + eps)."""
    m = s / F64(n)
    v = np.maximum(q / F64(n) - m * m, 0.0)
    if dtype == F64:
        return m, v, 1.0 / np.sqrt(v + F64(F32(eps)))
    mf, vf = m.astype(F32), v.astype(F32)
    return mf, v, (F32(1) / np.sqrt(vf + F32(eps), dtype=F32)).astype(F32)


def bn_stats(x, eps=EPS, dtype=F64, slip=None):
    """x [groups, P, C] -> mean, var (biased, float64 even in the fp32 evaluation: the entry keeps it in double), invstd, each [groups, C]."""
    seq = dtype == F32
    xd = _f(x, F64)
    s = seqsum(xd, 1, F64, seq)
    if slip == 'sumsq_f32':
        q = seqsum(_f(x, F32) * _f(x, F32), 1, F32, True).astype(F64)
    else:
        q = seqsum(xd * xd, 1, F64, seq)
    m, v, inv = stats_from_sums(s, q, x.shape[1], eps, dtype)
    if slip == 'eps_outside':
        inv = (1.0 / (np.sqrt(v) + F64(F32(eps)))).astype(dtype)
    return m, v, inv


def tile_cuts(P, items):
    """A ragged partition of P pixels into ``items`` runs: boundaries [items + 1]."""
    assert P >= items
    rng = np.random.default_rng(P * 1000 + items)
    inner = np.sort(rng.choice(np.arange(1, P), size=items - 1, replace=False)) if items > 1 else np.zeros(0, np.int64)
    return np.concatenate(([0], inner, [P])).astype(np.int64)


def tile_sums(a, b, cuts):
    """Per-item float64 sums of a and b [groups, P, C] over the runs of ``cuts``, rounded to fp32: the slab [groups*items, 2, C]."""
    g, _, c = a.shape
    out = np.zeros((g, len(cuts) - 1, 2, c), F64)
    for k, arr in enumerate((a, b)):
        out[:, :, k] = np.add.reduceat(_f(arr, F64), cuts[:-1], axis=1)
    return out.reshape(g * (len(cuts) - 1), 2, c).astype(F32)


def tile_stats_fwd(x, cuts):
    xd = _f(x, F64)
    return tile_sums(xd, xd * xd, cuts)


def tile_stats_bwd(dz, y_minus_beta, cuts):
    return tile_sums(_f(dz, F64), _f(dz, F64) * _f(y_minus_beta, F64), cuts)


def bn_stats_tiles(ts, groups, P, eps=EPS, dtype=F64):
    """Statistics from a forward slab [groups*items, 2, C] (fp32 per-item sum x, sum x^2), the items added in double."""
    t = _f(ts, F64).reshape(groups, -1, 2, ts.shape[-1])
    seq = dtype == F32
    return stats_from_sums(seqsum(t[:, :, 0], 1, F64, seq), seqsum(t[:, :, 1], 1, F64, seq), P, eps, dtype)


def bn_moving(mm0, mv0, mean, var, n, decay=DECAY, dtype=F64, slip=None):
    """TF fused batch norm: moving -= (moving - batch) (1 - decay), variance Bessel-corrected by n/max(n-1,1); once per group IN ORDER."""
    om = F64(1.0) - F64(F32(decay))                     # exact in fp32 too
    fac = 1.0 if slip == 'biased_moving' else F64(n) / F64(max(n - 1, 1))
    mm, mv = _f(mm0, dtype).copy(), _f(mv0, dtype).copy()
    order = range(mean.shape[0])
    for g in (reversed(order) if slip == 'reverse_groups' else order):
        mb, unb, o = _f(mean[g], dtype), _f(_f(var[g], F64) * fac, dtype), dtype(om)
        mm = mm - (mm - mb) * o
        mv = mv - (mv - unb) * o
    return mm, mv


def bn_xhat(x, mean, invstd, dtype=F64):
    return (_f(x, dtype) - _f(mean, dtype)[:, None, :]) * _f(invstd, dtype)[:, None, :]


def bn_y(x, mean, invstd, gamma, beta, act, dtype=F64):
    """y = xhat gamma + beta (+ ReLU) on given mean / invstd [groups, C]."""
    y = bn_xhat(x, mean, invstd, dtype) * _f(gamma, dtype) + _f(beta, dtype)
    return np.maximum(y, dtype(0)) if act else y


def bn_dz(dy, x, mean, invstd, gamma, beta, act, dtype=F64, slip=None):
    """dz = dy [y > 0] under ReLU (0 at y <= 0), dy otherwise; also xhat."""
    xh = bn_xhat(x, mean, invstd, dtype)
    if not act:
        return _f(dy, dtype), xh
    y = xh * _f(gamma, dtype) + _f(beta, dtype)
    keep = (y >= 0) if slip == 'relu_ge' else (y > 0)
    return np.where(keep, _f(dy, dtype), dtype(0)), xh


def bn_bwd_sums(dz, xh, x=None, dtype=F64, slip=None):
    """s0 = sum dz, s1 = sum dz xhat per group [groups, C] (double accumulators; the fp32 evaluation hands them on as floats)."""
    seq = dtype == F32
    other = _f(x, F64) if slip == 'dgamma_x' else _f(xh, F64)
    s0, s1 = seqsum(_f(dz, F64), 1, F64, seq), seqsum(_f(dz, F64) * other, 1, F64, seq)
    return s0.astype(dtype), s1.astype(dtype)


def bn_bwd_sums_tiles(ts, groups, gamma, dtype=F64):
    """Backward sums from a slab of per-item sum dz, sum dz (y - beta): the second divided by gamma, 0 where gamma = 0."""
    t = _f(ts, F64).reshape(groups, -1, 2, ts.shape[-1])
    seq = dtype == F32
    s0, q = seqsum(t[:, :, 0], 1, F64, seq), seqsum(t[:, :, 1], 1, F64, seq)
    ga = _f(gamma, F64)
    with np.errstate(divide='ignore', invalid='ignore'):
        s1 = np.where(ga != 0.0, q / ga, 0.0)
    return s0.astype(dtype), s1.astype(dtype)


def bn_param_grads(s0, s1, pre_dgamma, pre_dbeta, accumulate, dtype=F64, slip=None):
    """dbeta = sum_g s0, dgamma = sum_g s1 in group order; on top of the pre-filled values when ``accumulate``, in their place otherwise."""
    acc = accumulate and slip != 'accumulate_ignored'
    dg = _f(pre_dgamma, dtype).copy() if acc else np.zeros(s0.shape[1], dtype)
    db = _f(pre_dbeta, dtype).copy() if acc else np.zeros(s0.shape[1], dtype)
    for g in range(s0.shape[0]):
        db = db + _f(s0[g], dtype)
        dg = dg + _f(s1[g], dtype)
    return dg, db


def bn_dx(dz, xh, s0, s1, gamma, invstd, dtype=F64, slip=None):
    """dx = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)) per group; the means are over the group's P pixels."""
    groups, n = dz.shape[0], dz.shape[1]
    inv_count = dtype(F64(1.0) / F64(n * groups if slip == 'mean_over_all' else n))
    m0, m1 = _f(s0, dtype)[:, None, :] * inv_count, _f(s1, dtype)[:, None, :] * inv_count
    gi = (_f(gamma, dtype) * _f(invstd, dtype))[:, None, :]
    if slip == 'drop_xhat_term':
        return gi * (_f(dz, dtype) - m0)
    return gi * (_f(dz, dtype) - m0 - _f(xh, dtype) * m1)


def bn_invstd(var, eps=EPS, dtype=F64):
    return (dtype(1) / np.sqrt(_f(var, dtype) + dtype(F32(eps)))).astype(dtype)


def bn_fold(w, bias, gamma, beta, mm, mv, eps=EPS, dtype=F64):
    """relu(gamma (conv(x,w) + b - mm) rsqrt(mv + eps) + beta) = relu(conv(x, w s) + (b - mm) s + beta): w [rows, C] -> (w s, (b - mm) s + beta)."""
    s = _f(gamma, dtype) * bn_invstd(mv, eps, dtype)
    b = np.zeros(w.shape[1], dtype) if bias is None else _f(bias, dtype)
    return _f(w, dtype) * s, (b - _f(mm, dtype)) * s + _f(beta, dtype)


def chan_sum(x, dtype=F64):
    """x [P, C] -> per-channel sum (double accumulator, fp32 result)."""
    return seqsum(_f(x, F64), 0, F64, dtype == F32).astype(dtype)


# ----------------------------------------------------------------------------------------------- bounds
def _finv(t, eps):
    return 1.0 / np.sqrt(np.maximum(t, 0.0) + F64(F32(eps)))


def stats_bounds(abs1, abs2, m, v, terms, n, eps=EPS):
    """(mean bound, variance bound, invstd bound, unbiased-variance bound) from float64 m, v; abs1 = sum|terms of s|/n, abs2 = sum|terms of q|/n."""
    dm = U * np.abs(m) + (terms + 4) * D * abs1 + DEN
    dv = (terms + 4) * D * (abs2 + m * m) + U * v + DEN
    f = _finv(v, eps)
    dis = np.maximum(np.abs(_finv(v + dv, eps) - f), np.abs(_finv(v - dv, eps) - f)) + 2 * E * f
    fac = n / max(n - 1, 1)
    dunb = (terms + 4) * D * (abs2 + m * m) * fac + U * v * fac + DEN
    return dm, dv, dis, dunb


def stats_bounds_x(x, eps=EPS):
    xd = _f(x, F64)
    n = x.shape[1]
    m, v, _ = bn_stats(x, eps)
    return stats_bounds(np.mean(np.abs(xd), 1), np.mean(xd * xd, 1), m, v, n, n, eps)


def stats_bounds_tiles(ts, groups, P, eps=EPS):
    t = np.abs(_f(ts, F64)).reshape(groups, -1, 2, ts.shape[-1])
    m, v, _ = bn_stats_tiles(ts, groups, P, eps)
    return stats_bounds(t[:, :, 0].sum(1) / P, t[:, :, 1].sum(1) / P, m, v, t.shape[1], P, eps)


def moving_bounds(mm0, mv0, mean, var, dunb, n, decay=DECAY):
    """Bounds of the moving statistics after the in-order updates (mean: the entry's saved means; var, dunb: float64 and its bound)."""
    om = 1.0 - F64(F32(decay))
    fac = n / max(n - 1, 1)
    mm, mv = _f(mm0, F64).copy(), _f(mv0, F64).copy()
    bm, bv = np.full(mm.shape, DEN), np.full(mv.shape, DEN)
    for g in range(mean.shape[0]):
        unb = _f(var[g], F64) * fac
        bm = bm + 3 * U * (np.abs(mm) + np.abs(_f(mean[g], F64)))
        bv = bv + 3 * U * (np.abs(mv) + unb) + om * (dunb[g] + U * unb)
        mm = mm - (mm - _f(mean[g], F64)) * om
        mv = mv - (mv - unb) * om
    return bm, bv


def y_bound(x, mean, invstd, gamma, beta):
    xh = bn_xhat(x, mean, invstd)
    return 4 * U * (np.abs(xh * _f(gamma, F64)) + np.abs(_f(beta, F64))) + DEN


def bwd_sum_bounds(dz, xh):
    """(ds0, ds1) [groups, C] of the reduction pass, from float64 dz, xhat."""
    n = dz.shape[1]
    dz, p = _f(dz, F64), _f(dz, F64) * _f(xh, F64)
    ds0 = (n + 4) * D * np.abs(dz).sum(1) + U * np.abs(dz.sum(1)) + DEN
    ds1 = (E + (n + 4) * D) * np.abs(p).sum(1) + U * np.abs(p.sum(1)) + DEN
    return ds0, ds1


def bwd_sum_bounds_tiles(ts, groups, gamma):
    t = np.abs(_f(ts, F64)).reshape(groups, -1, 2, ts.shape[-1])
    items = t.shape[1]
    s0, s1 = bn_bwd_sums_tiles(ts, groups, gamma)
    ga = np.abs(_f(gamma, F64))
    ds0 = (items + 4) * D * t[:, :, 0].sum(1) + U * np.abs(s0) + DEN
    with np.errstate(divide='ignore', invalid='ignore'):
        ds1 = np.where(ga != 0.0, (items + 4) * D * t[:, :, 1].sum(1) / ga + (U + D) * np.abs(s1) + DEN, 0.0)
    return ds0, ds1


def param_grad_bounds(s0, s1, ds0, ds1, pre_dgamma, pre_dbeta, accumulate):
    t = s0.shape[0] + (1 if accumulate else 0)
    pg = np.abs(_f(pre_dgamma, F64)) if accumulate else 0.0
    pb = np.abs(_f(pre_dbeta, F64)) if accumulate else 0.0
    return (ds1.sum(0) + (t - 1) * U * (pg + np.abs(s1).sum(0)), ds0.sum(0) + (t - 1) * U * (pb + np.abs(s0).sum(0)))


def dx_bound(dz, xh, s0, s1, ds0, ds1, gamma, invstd):
    n = dz.shape[1]
    axh = np.abs(_f(xh, F64))
    T = np.abs(_f(dz, F64)) + (np.abs(s0) / n)[:, None, :] + axh * (np.abs(s1) / n)[:, None, :]
    gi = np.abs(_f(gamma, F64) * _f(invstd, F64))[:, None, :]
    return gi * (10 * U * T + (ds0[:, None, :] + axh * ds1[:, None, :]) / n) + DEN


def chan_sum_bound(x):
    xd = _f(x, F64)
    return U * np.abs(xd.sum(0)) + (x.shape[0] + 4) * D * np.abs(xd).sum(0) + DEN


def invstd_bound(var, eps=EPS):
    return 2 * E * bn_invstd(var, eps)


def fold_bounds(w, bias, gamma, beta, mm, mv, eps=EPS):
    s = _f(gamma, F64) * bn_invstd(mv, eps)
    b = 0.0 if bias is None else _f(bias, F64)
    return 8 * U * np.abs(_f(w, F64) * s), 8 * U * (np.abs((b - _f(mm, F64)) * s) + np.abs(_f(beta, F64))) + DEN


def undecided(x, mean, invstd, gamma, beta, scale=1.0, extra=0.0):
    """Elements whose ReLU mask an fp32 evaluation could take either way: |y64| <= 2^-10 (|xhat gamma| + |beta|) at gamma != 0."""
    xh = bn_xhat(x, mean, invstd)
    ga, be = _f(gamma, F64), _f(beta, F64)
    mag = np.abs(xh * ga) + np.abs(be)
    return (np.abs(xh * ga + be) <= scale * 2.0 ** -10 * mag + extra) & (ga != 0.0)


# ----------------------------------------------------------------------------------------------- seeded inputs
def _draw(rng, regime, shape, g):
    n = rng.standard_normal(shape)
    if regime == 'normal':
        return 0.5 + g + 2.0 * n
    if regime == 'normal8':
        return 8.0 + g + n
    if regime == 'offset_a':
        return 1e3 + 1e-1 * n
    if regime == 'offset_b':
        return -1e4 + n
    if regime == 'constant':
        return np.full(shape, 3.25 + g)
    if regime == 'tiny':
        return 1e-20 * n
    if regime == 'large':
        return 1e15 * n
    if regime == 'sparse':
        return np.where(rng.random(shape) < 0.95, 0.0, n)
    raise ValueError(regime)


def channel_regimes(C, bf16=False):
    table = REGIMES_BF16 if bf16 else REGIMES
    return [table[c % len(table)] for c in range(C)]


def make_case(shape, seed=0, bf16=False, bf16_dy=None, cuts=None):
    """Seeded tensors of one case: x, dy [groups, P, C] fp32 (bf16-exact where asked), gamma, beta, pre-filled dgamma / dbeta, moving statistics.
    No element is undecided (module header): offending elements are moved away from the zero crossing until none is left.  With ``cuts`` the
    statistics that decide are those of the fp32 slab over that partition (on a channel with |mean| >> sigma they are far from the direct ones)."""
    groups, P, C = shape[:3]
    rng = np.random.default_rng(1000003 * seed + 7919 * groups + 31 * P + C)
    regs = channel_regimes(C, bf16)
    x = np.empty((groups, P, C), F64)
    for c, r in enumerate(regs):
        for g in range(groups):
            x[g, :, c] = _draw(rng, r, P, g)
    rnd = to_bf16 if bf16 else (lambda a: a.astype(F32))
    x = rnd(x)
    gamma = (rng.choice([-1.0, 1.0], C) * rng.uniform(0.5, 1.5, C)).astype(F32)
    beta = (rng.choice([-1.0, 1.0], C) * rng.uniform(0.1, 1.0, C)).astype(F32)
    if C >= 12:
        cc = np.arange(C) % 16
        gamma[(cc == 8) | (cc == 9)] = 0
        beta[cc == 8] = 0
        beta[cc == 9] = np.abs(beta[cc == 9])
    dy = rng.standard_normal((groups, P, C))
    dy = to_bf16(dy) if (bf16 if bf16_dy is None else bf16_dy) else dy.astype(F32)
    fixed = np.array([r in ('constant',) for r in regs])
    live = np.arange(C)                                       # channels that still hold an undecided element
    for it in range(200):
        xs, ga, be = x[:, :, live], _f(gamma[live], F64), _f(beta[live], F64)
        m, v, inv = bn_stats(xs) if cuts is None else bn_stats_tiles(tile_stats_fwd(xs, cuts), groups, P)
        bad = undecided(xs, m, inv, ga, be, scale=2.0,
                        extra=np.where(v > 0, 4 * U * np.abs(m) * inv * np.abs(ga), 0.0)[:, None, :])   # (v = 0: the mean is exact)
        hit = bad.any(axis=(0, 1))
        if not hit.any():
            break
        live, xs, bad, ga, be, m, v, inv = live[hit], _f(xs[:, :, hit], F64), bad[:, :, hit], ga[hit], be[hit], m[:, hit], v[:, hit], inv[:, hit]
        xh = bn_xhat(xs, m, inv)
        away = np.where(xh >= -be / ga, 1.0, -1.0)            # (gamma != 0 on every undecided element)
        sd = np.sqrt(v)[:, None, :]
        movable = bad & ~fixed[live][None, None, :] & (xs != 0)
        x[:, :, live] = rnd(np.where(movable, xs + away * (0.03 * (1 + it % 7)) * np.maximum(sd, np.abs(xs) * 2.0 ** -6), xs))
        stuck = (bad & ~movable).any(axis=(0, 1))           # exact zeros of a sparse channel: move beta instead
        beta[live] = np.where(stuck, beta[live] * F32(1.25) + F32(0.0625) * np.sign(beta[live]), beta[live]).astype(F32)
    else:
        raise AssertionError('undecided elements remain in %r' % (shape,))
    return dict(shape=shape, x=x, dy=dy, gamma=gamma, beta=beta,
                pre_dgamma=rng.standard_normal(C).astype(F32), pre_dbeta=rng.standard_normal(C).astype(F32),
                mm0=rng.standard_normal(C).astype(F32), mv0=rng.uniform(0.5, 2.0, C).astype(F32), regimes=regs)


_cache = {}


def case(name, bf16=False, bf16_dy=None):
    """The tensors of a named case, computed once and shared (callers must not modify them)."""
    key = (name, bf16, bf16_dy)
    if key not in _cache:
        spec = (CASES_BF16 if bf16 else CASES)[name]
        c = make_case(spec['shape'], seed=len(name), bf16=bf16, bf16_dy=bf16_dy)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        c.update({k: v for k, v in spec.items() if k != 'shape'})
        _cache[key] = c
    return _cache[key]


def tile_case(items, bf16=False):
    """2 groups x (2 items + 3 pixels) x 16 channels, with its forward slab and the cuts."""
    key = ('tile', items, bf16)
    if key not in _cache:
        cuts = tile_cuts(2 * items + 3, items)
        c = make_case((2, 2 * items + 3, 16, 16), seed=items, bf16=bf16, cuts=cuts)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        c['cuts'] = cuts
        c['ts_fwd'] = tile_stats_fwd(c['x'], c['cuts'])
        _cache[key] = c
    return _cache[key]


# ----------------------------------------------------------------------------------------------- whole-case evaluation
def forward_ratios(c, out, act, ts=None, bf16_y=False, with_moving=True, decay=DECAY):
    """Worst error/bound of a forward result ``out`` (mean, invstd, mm, mv, y as arrays) of case ``c``; y and the moving mean on out's own
    mean / invstd.  Returns {quantity: ratio}."""
    x, groups, n = c['x'], c['shape'][0], c['shape'][1]
    if ts is None:
        m, v, inv = bn_stats(x)
        dm, _, dis, dunb = stats_bounds_x(x)
    else:
        m, v, inv = bn_stats_tiles(ts, groups, n)
        dm, _, dis, dunb = stats_bounds_tiles(ts, groups, n)
    r = {'mean': worst(out['mean'] - m, dm), 'invstd': worst(out['invstd'] - inv, dis)}
    if with_moving:
        mm, mv = bn_moving(c['mm0'], c['mv0'], out['mean'], v, n, decay)
        bm, bv = moving_bounds(c['mm0'], c['mv0'], out['mean'], v, dunb, n, decay)
        r['moving_mean'], r['moving_var'] = worst(out['mm'] - mm, bm), worst(out['mv'] - mv, bv)
    y = bn_y(x, out['mean'], out['invstd'], c['gamma'], c['beta'], act)
    yb = y_bound(x, out['mean'], out['invstd'], c['gamma'], c['beta'])
    r['y'] = worst(out['y'] - y, yb + (B8 * np.abs(y) if bf16_y else 0.0))
    return r


def backward_ratios(c, mean, invstd, out, act, accumulate, ts=None, bf16_dx=False):
    """Worst error/bound of a backward result ``out`` (dx, dgamma, dbeta) on the saved ``mean`` / ``invstd``."""
    groups = c['shape'][0]
    dz, xh = bn_dz(c['dy'], c['x'], mean, invstd, c['gamma'], c['beta'], act)
    if ts is None:
        s0, s1 = bn_bwd_sums(dz, xh)
        ds0, ds1 = bwd_sum_bounds(dz, xh)
    else:
        s0, s1 = bn_bwd_sums_tiles(ts, groups, c['gamma'])
        ds0, ds1 = bwd_sum_bounds_tiles(ts, groups, c['gamma'])
    dg, db = bn_param_grads(s0, s1, c['pre_dgamma'], c['pre_dbeta'], accumulate)
    bg, bb = param_grad_bounds(s0, s1, ds0, ds1, c['pre_dgamma'], c['pre_dbeta'], accumulate)
    dx = bn_dx(dz, xh, s0, s1, c['gamma'], invstd)
    bx = dx_bound(dz, xh, s0, s1, ds0, ds1, c['gamma'], invstd) + (B8 * np.abs(dx) if bf16_dx else 0.0)
    return {'dx': worst(out['dx'] - dx, bx), 'dgamma': worst(out['dgamma'] - dg, bg), 'dbeta': worst(out['dbeta'] - db, bb)}


def evaluate(c, act, accumulate, dtype=F64, slip=None, ts_items=None):
    """The whole chain of one case in ``dtype`` (each stage on the stage before, as the entries run): forward and backward results."""
    x, groups, n = c['x'], c['shape'][0], c['shape'][1]
    if ts_items is None:
        m, v, inv = bn_stats(x, EPS, dtype, slip)
    else:
        m, v, inv = bn_stats_tiles(c['ts_fwd'], groups, n, EPS, dtype)
    mm, mv = bn_moving(c['mm0'], c['mv0'], m, v, n, DECAY, dtype, slip)
    fwd = dict(mean=m, invstd=inv, mm=mm, mv=mv, y=bn_y(x, m, inv, c['gamma'], c['beta'], act, dtype))
    dz, xh = bn_dz(c['dy'], x, m, inv, c['gamma'], c['beta'], act, dtype, slip)
    if ts_items is None:
        s0, s1 = bn_bwd_sums(dz, xh, x, dtype, slip)
        ts_b = None
    else:
        dz64, xh64 = bn_dz(c['dy'], x, m, inv, c['gamma'], c['beta'], act)
        ts_b = tile_stats_bwd(dz64, xh64 * _f(c['gamma'], F64), c['cuts'])
        s0, s1 = bn_bwd_sums_tiles(ts_b, groups, c['gamma'], dtype)
    dg, db = bn_param_grads(s0, s1, c['pre_dgamma'], c['pre_dbeta'], accumulate, dtype, slip)
    bwd = dict(dx=bn_dx(dz, xh, s0, s1, c['gamma'], inv, dtype, slip), dgamma=dg, dbeta=db)
    return fwd, bwd, ts_b
