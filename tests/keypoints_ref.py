"""Restatements, seeded inputs and error bounds for csrc/keypoints.hip: the key-point head (kpx_keypoint_head_{fwd,bwd}_f32), the head
folded over the 1x1 projection (kpx_keypoint_head_proj_{fwd,bwd}_f32) and the Gaussian maps (kpx_gaussian_maps_{fwd,bwd}_f32); shared
by test_keypoints_cpu.py and test_keypoints_gpu.py.

Every restatement is plain numpy and takes ``dtype``: float64 is the reference, float32 evaluates the same formulas with every
operation rounded and every sum taken SEQUENTIALLY in fp32 (the worst order a kernel may use); the CPU suite holds that evaluation
to the bounds below, so a bound no fp32 code could meet cannot sit here unnoticed.  ``form`` picks the fp32 linspace: 'two'
(-1 + fl(step*i), two roundings) or 'fma' (fl(step*i - 1), one): the compiler may emit either.  inv_std**2 is rounded to fp32 first,
as the entries do.  ``slip`` plants a mistake (test_keypoints_cpu.py shows that the bounds reject each).

Bounds (fixed before anything ran on a GPU).  u = 2^-24, e = 2u, n = profile length, other = the axis averaged away.  Every sum
bound is order-free ((terms - 1) u sum|terms| holds for any reduction tree).
  profile mean   delta = max over the profile of (other-1) u mean|x| + u |mean|;
                 folded head: delta = (other + C + 2) u (sum_c mean|x|_c |w_ck| + |b_k|); xs_y / xs_x: (other-1) u sum|x|
  probabilities  |p^ - p| <= p expm1(2 delta + (n+16) e) + PTINY
  key points     |mu^ - mu| <= (expm1(2 delta + (n+16) e) + (n+4) e) sum p|lin| + e sum p (1+lin) + 1e-30
  head backward  on the kernel's own saved mu / py / px: 16e (|dmu_y| p_y (|lin_h|+|mu_y|)/W + |dmu_x| p_x (|lin_w|+|mu_x|)/H)
                 + e (|dmu_y| p_y (1+lin_h)/W + |dmu_x| p_x (1+lin_w)/H) + 1e-30
  folded bwd     on saved state, with M = |dmu| p (|lin| + |mu|)/other (>= |d|) and L = e |dmu| p (1+lin)/other per axis:
                 dx sum_k ((K+16) e M + L)|w| ; dw sum |xs| ((n+2B+16) e M + L), n = max(H,W) ; db other sum ((n+2B+16) e M + L)
  Gaussian map   dy, dx, dist in float64, derr = inv2 (4e(|dy|+|dx|) + 4e(dy^2+dx^2)): |g^ - g| <= g expm1(derr + e dist + 4e) + 1.2e-38
                 (the last term: a flushed denormal result of the hardware exponential)
  Gaussian bwd   (H W + 16) e T + 1e-30 with T = sum_{h,w} |dmaps| g 2 inv2 |x - mu| per component, plus the error of the
                 kernel's own fp32 g and x - mu: sum |dmaps| 2 inv2 (g expm1(derr + e dist + 4e) |x - mu| + 2e g)

Four terms above are wider than the plain n*e forms, each because the fp32 restatement (a correct evaluation) cannot meet the plain one:
  e (1+lin): fp32 linspace is a cancellation, -1 + step*i with step*i in [0,2]; its error is e*step*i + u|lin| = e(1+lin) + u|lin|, NOT
    relative to |lin|.  At the centre of an odd axis lin = 0 in float64 and up to 2^-24 in fp32 (n = 13: step = fl(1/6) > 1/6, the fused
    form gives +2^-25): a one-hot profile there ('spike') has sum p|lin| = 0, and in 'flat' |lin_h| + |mu| ~ 1e-9 at the centre row.
  M in place of |d|: d = dmu p (lin - mu)/other cancels wherever the profile is concentrated (mu = lin at the one place where p > 0:
    'spike', 'wide'), so its rounding error is relative to |dmu| p (|lin| + |mu|)/other, as in the head backward, not to |d|; with |d| the
    fp32 restatement misses the dx bound by 1e5 on 'spike'.
  PTINY = 4 * 2^-149: a probability in the denormal range is rounded to a multiple of 2^-149 three times (the exponential, its
    product with 1/sum <= 1, and the propagated half-spacing), each by at most 2^-150; 'wide' on a 512-long axis reaches that range.
  Gaussian bwd second sum: the kernel recomputes g in fp32; at inv_std = 40 derr alone is ~1e-4 relative (an fp32 grid value carries
    an absolute error e, amplified by 2 inv2 |dy| = 3200 |dy|), which (H W + 16) e cannot cover at H W = 126.
"""
import numpy as np

U = 2.0 ** -24
E = 2.0 * U
TINY = 1e-30
PTINY = 4 * 2.0 ** -149
GTINY = 1.2e-38
F32 = np.float32
F64 = np.float64

HEAD_REGIMES = ('normal', 'wide', 'flat', 'spike', 'huge')
HEAD_SHAPES = ((2, 13, 21, 5), (1, 70, 130, 3), (1, 512, 2, 1), (1, 2, 512, 1), (1, 8, 8, 256), (1, 8, 12, 129), (1, 2, 2, 1),
               (3, 32, 32, 40))
# (B,H,W,C,K), bias
PROJ_SHAPES = (((2, 13, 21, 8, 5), True), ((1, 70, 130, 4, 3), True), ((9, 8, 12, 8, 17), True), ((1, 16, 16, 4, 64), True),
               ((1, 8, 8, 256, 1), True), ((1, 480, 2, 32, 32), True), ((2, 24, 40, 8, 5), False))
MU_REGIMES = ('inside', 'outside', 'nodes')
INV_STDS = (14.3, 40.0, 1.0)
# (B,K,H,W), expected launch path, inv_stds; 'offset' = the output view starts one float into its buffer
GAUSS_CASES = (
    ((2, 15, 32, 32), 'reg_wfix', INV_STDS, 0),          # T = 480, 4m = 128 = 4 rows
    ((2, 4, 6, 6), 'reg_wfix', (14.3,), 0),              # T = 384 > n4 = 36: one ragged slab; 4m = 384 = 64 rows > H (a thread never iterates)
    ((1, 512, 2, 2), 'reg_wfix', (14.3,), 0),            # T = 512, m = 1, 4m = 4 = 2 rows
    ((512, 15, 34, 32), 'reg_wfix', (14.3,), 0),         # T = 480, G = 1, iters = 9, n4 % T = 240
    ((1, 40, 16, 64), 'reg', INV_STDS, 0),               # T = 320 (m = 8), 32 % 64 != 0
    ((1, 16, 8, 33), 'reg', (14.3,), 0),                 # odd W, n4 = 1056, T = 512, ragged
    ((1, 260, 8, 8), 'reg', (14.3,), 0),                 # m = 1, T = 260
    ((2, 3, 16, 20), 'flat', INV_STDS, 0),               # K < 4: LDS tables, multiply-shift division
    ((2, 1, 8, 8), 'flat', (14.3,), 0),
    ((1, 5, 9, 9), 'strided', (14.3,), 0),               # H W K = 405, not a multiple of 4
    ((1, 520, 4, 4), 'strided', (14.3,), 0),             # K > 512
    ((2, 15, 32, 32), 'strided', (14.3,), 1),            # misaligned base
    ((1, 128, 256, 256), 'strided', (14.3,), 0),         # exactly 2^23 elements per image
    ((512, 40, 12, 63), 'reg', (14.3,), 0),              # general register path, T = 320, iters = 6, n4 % T = 200
)
GAUSS_BWD_CASES = tuple((k, 9, 14) for k in (1, 15, 129, 256)) + ((15, 32, 32),)
GAUSS_BWD_INV_STDS = (14.3, 40.0)


def _f(x, dtype):
    return np.asarray(x).astype(dtype)


def seqsum(a, axis, dtype):
    """Sum along ``axis``: float64 pairwise, or fp32 strictly left to right (numpy's cumsum does not reassociate)."""
    if dtype == F64:
        return np.sum(a, axis=axis, dtype=F64)
    return np.take(np.cumsum(a, axis=axis, dtype=F32), -1, axis=axis)


def linspace(n, dtype=F64, form='two', step_slip=False):
    """tf.linspace(-1, 1, n): start + step * i."""
    i = np.arange(n)
    den = n if step_slip else n - 1
    if dtype == F64:
        return -1.0 + (2.0 / den) * i
    step = F32(2) / F32(den)
    if form == 'fma':
        return (F64(step) * i - 1.0).astype(F32)            # step * i - 1 is exact in float64 (24 + 10 bits): one rounding
    return F32(-1) + step * i.astype(F32)


def worst(err, bound):
    """max |err| / bound; a NaN or an error past an infinite bound's reach counts as infinite."""
    err, bound = np.abs(np.asarray(err, F64)), np.asarray(bound, F64)
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(np.isinf(bound) & np.isfinite(err), 0.0, err / bound)
    if r.size == 0:
        return 0.0
    return float(np.inf) if np.any(np.isnan(r)) else float(r.max())


def _mul0(a, b):
    """a * b with inf * 0 = 0 (a: a possibly infinite factor, b: a magnitude)."""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(b == 0, 0.0, a * b)


def _expm1(x):
    with np.errstate(over='ignore'):
        return np.expm1(x)


# ----------------------------------------------------------------------------------------------- inputs
def head_logits(shape, regime, seed=0):
    b, h, w, k = shape
    rng = np.random.RandomState(1000 + seed + 7 * HEAD_REGIMES.index(regime) + h * 31 + w * 17 + k)
    x = rng.standard_normal(shape)
    if regime == 'wide':
        x = x * 30.0
    elif regime == 'flat':
        x = np.full(shape, 7.5)
    elif regime == 'spike':
        x[:, h // 2, :, :] += 1000.0                      # the centre row (an odd H: lin = 0 there) and the centre column
        x[:, :, w // 2, :] += 1000.0
    elif regime == 'huge':
        x = x * 1e30
    return x.astype(F32)


def head_dmu(shape, seed=0):
    b, h, w, k = shape
    return np.random.RandomState(2000 + seed + h + w + k).standard_normal((b, k, 2)).astype(F32)


def proj_inputs(shape, bias, regime='normal', seed=0):
    b, h, w, c, k = shape
    rng = np.random.RandomState(3000 + seed + h * 31 + w * 17 + c * 5 + k)
    x = head_logits((b, h, w, c), regime, seed=seed + 1)
    wk = (rng.standard_normal((c, k)) / np.sqrt(c)).astype(F32)
    bk = rng.standard_normal(k).astype(F32) if bias else None
    return x, wk, bk


def gauss_mu(b, k, h, w, regime, seed=0):
    rng = np.random.RandomState(4000 + seed + 3 * MU_REGIMES.index(regime) + k * 13 + h + w)
    if regime == 'inside':
        return rng.uniform(-0.9, 0.9, (b, k, 2)).astype(F32)
    if regime == 'outside':
        return rng.uniform(-1.3, 1.3, (b, k, 2)).astype(F32)
    mu = np.empty((b, k, 2), F32)                          # the fp32 grid values themselves ('two' form)
    mu[..., 0] = linspace(w, F32)[rng.randint(0, w, (b, k))]
    mu[..., 1] = linspace(h, F32)[rng.randint(0, h, (b, k))]
    return mu


def gauss_dmaps(b, h, w, k, seed=0):
    return np.random.RandomState(5000 + seed + k + h).standard_normal((b, h, w, k)).astype(F32)


# ----------------------------------------------------------------------------------------------- head
def _softmax_expect(m, dtype, form, slip):
    """m [B,n,K] profile means -> (mu [B,K], p [B,n,K])."""
    n = m.shape[1]
    mx = np.zeros_like(m[:, :1]) if slip == 'nomax' else m.max(axis=1, keepdims=True)
    with np.errstate(over='ignore', invalid='ignore'):
        ex = np.exp(m - mx)
        inv = dtype(1) / seqsum(ex, 1, dtype)
        p = ex * inv[:, None, :]
        lin = linspace(n, dtype, form, step_slip=(slip == 'step'))
        mu = seqsum(p * lin[None, :, None], 1, dtype)
    return mu, p


def head(x, dtype=F64, form='two', slip=None):
    """logits [B,H,W,K] -> mu [B,K,2] (x,y), prob_y [B,H,K], prob_x [B,W,K]."""
    x = _f(x, dtype)
    b, h, w, k = x.shape
    dy, dx = (h, w) if slip == 'axis' else (w, h)
    my = seqsum(x, 2, dtype) / dtype(dy)
    mx = seqsum(x, 1, dtype) / dtype(dx)
    mu_y, py = _softmax_expect(my, dtype, form, slip)
    mu_x, px = _softmax_expect(mx, dtype, form, slip)
    return np.stack([mu_x, mu_y], axis=-1), py, px


def _profile_bounds(p, delta, n):
    """(bound p [B,n,K], bound mu [B,K]) for a profile with float64 probabilities p and mean error delta [B,K]."""
    lin = linspace(n)[None, :, None]
    fac = _expm1(2 * delta + (n + 16) * E)                                     # [B,K]
    bp = _mul0(fac[:, None, :], p) + PTINY
    s = np.sum(p * np.abs(lin), axis=1)
    bmu = _mul0(fac + (n + 4) * E, s) + E * np.sum(p * (1 + lin), axis=1) + TINY
    return bp, bmu


def _head_mean_deltas(x):
    """(delta_y, delta_x) [B,K]: what an fp32 profile mean can be off by, at its worst place in the profile."""
    b, h, w, k = x.shape
    ax = np.abs(x)
    with np.errstate(over='ignore'):
        dy = ((w - 1) * U * ax.mean(axis=2) + U * np.abs(x.mean(axis=2))).max(axis=1)
        dx = ((h - 1) * U * ax.mean(axis=1) + U * np.abs(x.mean(axis=1))).max(axis=1)
    return dy, dx


def head_bounds(x):
    """(bound mu [B,K,2], bound prob_y, bound prob_x) around head(x) in float64."""
    x = _f(x, F64)
    b, h, w, k = x.shape
    _, py, px = head(x)
    dy, dx = _head_mean_deltas(x)
    bpy, bmy = _profile_bounds(py, dy, h)
    bpx, bmx = _profile_bounds(px, dx, w)
    return np.stack([bmx, bmy], axis=-1), bpy, bpx


def head_one_hot_margin(x):
    """The smallest gap between the two largest float64 means of a profile, less twice the error an fp32 mean can carry and the rounding
    of their difference.  Above 104 (exp(-104) < 2^-150 rounds to +0 in fp32) every fp32 evaluation, in any summation order, gives an
    exactly one-hot profile: p = 1 at the maximum (the sum of exponentials is 1 + 0 + ..), +0 elsewhere, and mu is the fp32 grid value."""
    x = _f(x, F64)
    out = np.inf
    for m, d in zip((x.mean(axis=2), x.mean(axis=1)), _head_mean_deltas(x)):
        top = np.sort(m, axis=1)
        gap = top[:, -1] - top[:, -2]
        out = min(out, float(np.min(gap * (1 - U) - 2 * d)))
    return out


def head_one_hot_ok(x, mu, py, px):
    """True if fp32 outputs are the exactly one-hot profiles of head(x) with mu the fp32 grid value of either linspace form."""
    x = _f(x, F64)
    b, h, w, k = x.shape
    ok = True
    for axis, p, m, n in ((1, py, x.mean(axis=2), h), (0, px, x.mean(axis=1), w)):
        arg = m.argmax(axis=1)                                                    # [B,K]
        hot = (np.arange(n)[None, :, None] == arg[:, None, :]).astype(np.float32)
        ok = ok and np.array_equal(np.asarray(p, np.float32).view(np.uint32), hot.view(np.uint32))
        grids = [linspace(n, F32, form)[arg] for form in ('two', 'fma')]
        got = np.asarray(mu, np.float32)[..., axis]
        ok = ok and bool(np.all((got == grids[0]) | (got == grids[1])))
    return bool(ok)


def _d_terms(dmu, mu, py, px, h, w, dtype, form='two'):
    """d_row [B,H,K] = dmu_y p_y (lin_h - mu_y) / W and d_col [B,W,K] likewise (the reciprocal is formed first, as the kernels do)."""
    dmu, mu, py, px = (_f(a, dtype) for a in (dmu, mu, py, px))
    lh, lw = linspace(h, dtype, form)[None, :, None], linspace(w, dtype, form)[None, :, None]
    iw, ih = dtype(1) / dtype(w), dtype(1) / dtype(h)
    drow = dmu[:, None, :, 1] * py * (lh - mu[:, None, :, 1]) * iw
    dcol = dmu[:, None, :, 0] * px * (lw - mu[:, None, :, 0]) * ih
    return drow, dcol


def _d_mags(dmu, mu, py, px, h, w):
    """(M_row, L_row, M_col, L_col) in float64: M = |dmu| p (|lin| + |mu|) / other, the magnitude d is rounded at, and
    L = e |dmu| p (1 + lin) / other, what the error of an fp32 linspace adds to d."""
    dmu, mu, py, px = (_f(a, F64) for a in (dmu, mu, py, px))
    lh, lw = linspace(h)[None, :, None], linspace(w)[None, :, None]
    ay, ax = np.abs(dmu[:, None, :, 1]) * py / w, np.abs(dmu[:, None, :, 0]) * px / h
    return (ay * (np.abs(lh) + np.abs(mu[:, None, :, 1])), ay * E * (1 + lh),
            ax * (np.abs(lw) + np.abs(mu[:, None, :, 0])), ax * E * (1 + lw))


def head_bwd(dmu, mu, py, px, h, w, dtype=F64, form='two'):
    """dlogits [B,H,W,K] = d_row[b,h,k] + d_col[b,w,k]: pointwise on the saved state."""
    drow, dcol = _d_terms(dmu, mu, py, px, h, w, dtype, form)
    return drow[:, :, None, :] + dcol[:, None, :, :]


def head_bwd_bound(dmu, mu, py, px, h, w):
    my, ly, mx, lx = _d_mags(dmu, mu, py, px, h, w)
    return (16 * E * my + ly)[:, :, None, :] + (16 * E * mx + lx)[:, None, :, :] + TINY


def head_bwd_forward_part(dmu, x):
    """What the forward's error adds to dlogits when the float64 gradient of the float64 forward is the reference (first order in the
    forward bounds, second-order term kept): |dmu| (bp |lin - mu| + (p + bp) bmu) / other per axis."""
    x = _f(x, F64)
    b, h, w, k = x.shape
    mu, py, px = head(x)
    bmu, bpy, bpx = head_bounds(x)
    dmu = _f(dmu, F64)
    lh, lw = linspace(h)[None, :, None], linspace(w)[None, :, None]
    ty = np.abs(dmu[:, None, :, 1]) * (bpy * np.abs(lh - mu[:, None, :, 1]) + (py + bpy) * bmu[:, None, :, 1]) / w
    tx = np.abs(dmu[:, None, :, 0]) * (bpx * np.abs(lw - mu[:, None, :, 0]) + (px + bpx) * bmu[:, None, :, 0]) / h
    return ty[:, :, None, :] + tx[:, None, :, :]


# ----------------------------------------------------------------------------------------------- folded head
def head_proj(x, wk, bk, dtype=F64, form='two', slip=None):
    """x [B,H,W,C], w [C,K], b [K] or None -> mu, prob_y, prob_x, xs_y [B,H,C], xs_x [B,W,C]."""
    x, wk = _f(x, dtype), _f(wk, dtype)
    b, h, w, c = x.shape
    xs_y, xs_x = seqsum(x, 2, dtype), seqsum(x, 1, dtype)
    bias = dtype(0) if bk is None else _f(bk, dtype)
    my = seqsum(xs_y[..., None] * wk[None, None], 2, dtype) / dtype(w) + bias
    mx = seqsum(xs_x[..., None] * wk[None, None], 2, dtype) / dtype(h) + bias
    mu_y, py = _softmax_expect(my, dtype, form, slip)
    mu_x, px = _softmax_expect(mx, dtype, form, slip)
    return np.stack([mu_x, mu_y], axis=-1), py, px, xs_y, xs_x


def head_proj_bounds(x, wk, bk):
    """(bound mu, bound prob_y, bound prob_x, bound xs_y, bound xs_x) around conv-then-head in float64."""
    x, wk = _f(x, F64), _f(wk, F64)
    b, h, w, c = x.shape
    ab = 0.0 if bk is None else np.abs(_f(bk, F64))
    _, py, px, _, _ = head_proj(x, wk, bk)
    ax, aw = np.abs(x), np.abs(wk)
    dy = ((w + c + 2) * U * (ax.mean(axis=2) @ aw + ab)).max(axis=1)
    dx = ((h + c + 2) * U * (ax.mean(axis=1) @ aw + ab)).max(axis=1)
    bpy, bmy = _profile_bounds(py, dy, h)
    bpx, bmx = _profile_bounds(px, dx, w)
    return np.stack([bmx, bmy], axis=-1), bpy, bpx, (w - 1) * U * ax.sum(axis=2) + 1e-45, (h - 1) * U * ax.sum(axis=1) + 1e-45


def head_proj_bwd(dmu, mu, py, px, xs_y, xs_x, wk, h, w, dtype=F64, form='two', slip=None):
    """-> dx [B,H,W,C], dw [C,K], db [K] on the saved state; one partial row per (image, axis), summed in that order."""
    drow, dcol = _d_terms(dmu, mu, py, px, h, w, dtype, form)
    wk, xs_y, xs_x = _f(wk, dtype), _f(xs_y, dtype), _f(xs_x, dtype)
    r = seqsum(drow[:, :, None, :] * wk[None, None], 3, dtype)                  # [B,H,C]
    cc = seqsum(dcol[:, :, None, :] * wk[None, None], 3, dtype)                 # [B,W,C]
    dx = r[:, :, None, :] + cc[:, None, :, :]
    pw_y = seqsum(xs_y[..., None] * drow[:, :, None, :], 1, dtype)              # [B,C,K]
    pw_x = seqsum(xs_x[..., None] * dcol[:, :, None, :], 1, dtype)
    pb_y = seqsum(drow, 1, dtype) * dtype(w)                                    # [B,K]
    pb_x = seqsum(dcol, 1, dtype) * dtype(h)
    if slip == 'dw_row':
        pw_y = pw_y.copy()
        pw_y[-1] = 0
    dw = seqsum(np.stack([pw_x, pw_y], axis=1).reshape((-1,) + pw_y.shape[1:]), 0, dtype)
    db = seqsum(np.stack([pb_x, pb_y], axis=1).reshape(-1, pb_y.shape[-1]), 0, dtype)
    return dx, dw, db


def head_proj_bwd_bounds(dmu, mu, py, px, xs_y, xs_x, wk, h, w):
    b, c, k = np.shape(xs_y)[0], np.shape(wk)[0], np.shape(wk)[1]
    my, ly, mx, lx = _d_mags(dmu, mu, py, px, h, w)
    aw, ay, ax = np.abs(_f(wk, F64)), np.abs(_f(xs_y, F64)), np.abs(_f(xs_x, F64))
    n = max(h, w)
    fx, fw = (k + 16) * E, (n + 2 * b + 16) * E
    bdx = ((fx * my + ly) @ aw.T)[:, :, None, :] + ((fx * mx + lx) @ aw.T)[:, None, :, :] + TINY
    bdw = np.einsum('bic,bik->ck', ay, fw * my + ly) + np.einsum('bic,bik->ck', ax, fw * mx + lx) + TINY
    bdb = w * (fw * my + ly).sum(axis=(0, 1)) + h * (fw * mx + lx).sum(axis=(0, 1)) + TINY
    return bdx, bdw, bdb


def proj_eligible(b, h, w, c, k):
    """kp_proj_dims_ok restated."""
    n = max(h, w)
    return (b > 0 and 2 <= h <= 512 and 2 <= w <= 512 and 0 < c <= 256 and 0 < k <= 64 and c % 4 == 0
            and (n * c + c * k) * 4 <= 65536 and (n * k + c * k) * 4 <= 65536)


# ----------------------------------------------------------------------------------------------- Gaussian maps
def inv2_of(inv_std, dtype=F64):
    return dtype(F32(float(inv_std) * float(inv_std)))


def _gauss_el(yv, xv, my, mx, inv2, dtype):
    dy, dx = yv - my, xv - mx
    dist = (dy * dy + dx * dx) * inv2
    with np.errstate(under='ignore'):
        return np.exp(-dist), dy, dx, dist


def gauss(mu, h, w, inv_std, dtype=F64, form='two', slip=None):
    """mu [B,K,2] (x,y) -> maps [B,H,W,K]."""
    mu = _f(mu, dtype)
    inv2 = dtype(F32(inv_std)) if slip == 'inv' else inv2_of(inv_std, dtype)
    ys, xs = linspace(h, dtype, form)[None, :, None, None], linspace(w, dtype, form)[None, None, :, None]
    return _gauss_el(ys, xs, mu[:, None, None, :, 1], mu[:, None, None, :, 0], inv2, dtype)[0]


def gauss_at(mu, h, w, inv_std, b, hh, ww, k):
    """float64 (value, bound) at the listed positions."""
    mu = _f(mu, F64)
    g, dy, dx, dist = _gauss_el(linspace(h)[hh], linspace(w)[ww], mu[b, k, 1], mu[b, k, 0], inv2_of(inv_std), F64)
    return g, _gauss_bound(g, dy, dx, dist, inv2_of(inv_std))


def _gauss_rel(dy, dx, dist, inv2):
    derr = inv2 * (4 * E * (np.abs(dy) + np.abs(dx)) + 4 * E * (dy * dy + dx * dx))
    return _expm1(derr + E * dist + 4 * E)


def _gauss_bound(g, dy, dx, dist, inv2):
    return _mul0(_gauss_rel(dy, dx, dist, inv2), g) + GTINY


def gauss_with_bound(mu, h, w, inv_std):
    mu = _f(mu, F64)
    inv2 = inv2_of(inv_std)
    ys, xs = linspace(h)[None, :, None, None], linspace(w)[None, None, :, None]
    g, dy, dx, dist = _gauss_el(ys, xs, mu[:, None, None, :, 1], mu[:, None, None, :, 0], inv2, F64)
    return g, _gauss_bound(g, dy, dx, dist, inv2)


def gauss_bwd(dmaps, mu, h, w, inv_std, dtype=F64, form='two'):
    """dmaps [B,H,W,K] -> dmu [B,K,2]: sum_{h,w} dmaps g 2 inv2 (x - mu_x), y likewise (pixels in row-major order)."""
    mu, dmaps = _f(mu, dtype), _f(dmaps, dtype)
    inv2 = inv2_of(inv_std, dtype)
    ys, xs = linspace(h, dtype, form)[None, :, None, None], linspace(w, dtype, form)[None, None, :, None]
    g, dy, dx, _ = _gauss_el(ys, xs, mu[:, None, None, :, 1], mu[:, None, None, :, 0], inv2, dtype)
    d = dmaps * g * (dtype(2) * inv2)
    b, k = mu.shape[:2]
    sx = seqsum((d * dx).reshape(b, h * w, k), 1, dtype)
    sy = seqsum((d * dy).reshape(b, h * w, k), 1, dtype)
    return np.stack([sx, sy], axis=-1)


def gauss_bwd_bound(dmaps, mu, h, w, inv_std):
    mu, dmaps = _f(mu, F64), np.abs(_f(dmaps, F64))
    inv2 = inv2_of(inv_std)
    ys, xs = linspace(h)[None, :, None, None], linspace(w)[None, None, :, None]
    g, dy, dx, dist = _gauss_el(ys, xs, mu[:, None, None, :, 1], mu[:, None, None, :, 0], inv2, F64)
    rel = np.minimum(_gauss_rel(dy, dx, dist, inv2), 1e300)
    a = dmaps * 2 * inv2
    out = []
    for dd in (dx, dy):
        t = (a * g * np.abs(dd)).sum(axis=(1, 2))
        own = (a * (g * rel * np.abs(dd) + 2 * E * g)).sum(axis=(1, 2))
        out.append((h * w + 16) * E * t + own + TINY)
    return np.stack(out, axis=-1)


def gauss_path(b, k, h, w, ldy=None, aligned=True):
    """The launch selection of kpx_gaussian_maps_fwd_f32 restated -> (path, T, iters, n4 % T); T = iters = 0 off the register paths."""
    ldy = k if ldy is None else ldy
    hwk = h * w * k
    flat = ldy == k and aligned and hwk % 4 == 0 and hwk < (1 << 23)
    if flat and 4 <= k <= 512:
        m, best, wfix = 1, 0, False
        mm = 1
        while k * mm <= 512:
            t = k * mm
            wf = (4 * mm) % w == 0
            fill = t * 1000 // (((t + 63) // 64) * 64) + (1000 if t >= 192 else 0) + (500 if wf else 0)
            if fill >= best:
                best, m, wfix = fill, mm, wf
            mm += 1
        t, n4 = k * m, hwk >> 2
        per = t * (11 if wfix else 6)
        g = (n4 + per - 1) // per
        if g * b < 512:
            g = (512 + b - 1) // b
        iters = max(1, (n4 + t * g - 1) // (t * g))
        return ('reg_wfix' if wfix else 'reg'), t, iters, n4 % t
    if flat and k <= 256 and w <= 512 and h <= 512:
        return 'flat', 0, 0, 0
    return 'strided', 0, 0, 0
