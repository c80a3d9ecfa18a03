"""The restatement of csrc/prdc.hip and kpx_amd.prdc for the tests: numpy, longdouble distances (direct differences), ``lexsort`` on (d2, index),
the scores as ratios of integers; and the generator of planted sets the tests run on.

The planted sets: a 2-d latent of unit Gaussians at the centres (0,0), (6,0), (0,6), (6,6), pushed through a random 2 x D map, plus 0.01 noise,
rounded through float32.  Real rows draw from the centres {0, 1, 2}, generated rows from {0, 1, 3}: two shared modes, one missed, one invented,
so that all four scores lie well inside (0, 1).  (i.i.d. high-dimensional Gaussians give precision 1 and recall 0 and test nothing.)
"""
import numpy as np

LD = np.longdouble
CENTRES = np.array([[0.0, 0.0], [6.0, 0.0], [0.0, 6.0], [6.0, 6.0]])
SCORES = ('precision', 'recall', 'density', 'coverage')


def planted(seed, n, m, d):
    """-> (real float64 [n, d], fake float64 [m, d], real_centre int32 [n], fake_centre int32 [m]); every value is a float32 value"""
    rs = np.random.RandomState(seed)
    proj = rs.randn(2, d) / np.sqrt(2.0)

    def draw(count, centres):
        c = np.array(centres)[rs.randint(0, len(centres), size=count)]
        z = CENTRES[c] + rs.randn(count, 2)
        return (z @ proj + 0.01 * rs.randn(count, d)).astype(np.float32).astype(np.float64), c.astype(np.int32)

    real, rc = draw(n, (0, 1, 2))
    fake, fc = draw(m, (0, 1, 3))
    return real, fake, rc, fc


def d2_matrix(q, r):
    """longdouble [M, N]: sum_d (q - r)^2, direct differences; NaN / inf where a row holds one"""
    q, r = np.asarray(q, LD), np.asarray(r, LD)
    out = np.empty((q.shape[0], r.shape[0]), LD)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(q.shape[0]):
            e = q[j][None, :] - r
            out[j] = (e * e).sum(axis=1)
    return out


def neighbours(q, r, k, q_group=None, r_group=None, q_skip=None, r_radius2=None, d2=None):
    """-> (nn_d2 longdouble [M, k], nn_idx int32 [M, k], inside int32 [M] or None, d2 longdouble [M, N], eligible bool [M, N]): the k
    lexicographically lowest (d2, index) of the eligible pairs, +inf / -1 in the empty places; inside = the eligible references with a
    finite radius and d2 <= radius."""
    d2 = d2_matrix(q, r) if d2 is None else d2
    m, n = d2.shape
    ok = np.isfinite(d2)
    if q_skip is not None:
        ok &= np.arange(n)[None, :] != np.asarray(q_skip)[:, None]
    if q_group is not None:
        ok &= np.asarray(q_group)[:, None] == np.asarray(r_group)[None, :]
    nn_d2, nn_idx = np.full((m, k), np.inf, LD), np.full((m, k), -1, np.int32)
    for j in range(m):
        idx = np.flatnonzero(ok[j])
        order = idx[np.lexsort((idx, d2[j, idx]))][:k]              # d2 first, the index breaks ties
        nn_d2[j, :len(order)], nn_idx[j, :len(order)] = d2[j, order], order
    inside = None
    if r_radius2 is not None:
        rad = np.asarray(r_radius2, LD)
        with np.errstate(invalid='ignore'):
            inside = (ok & np.isfinite(rad)[None, :] & (d2 <= rad[None, :])).sum(axis=1).astype(np.int32)
    return nn_d2, nn_idx, inside, d2, ok


def prdc(real, fake, k, real_group=None, fake_group=None):
    """The four scores and the per-row arrays of kpx_amd.prdc.prdc, restated; ``margin`` = the smallest relative distance between a d2 and
    the radius it is compared with (the comparisons that decide the integer counts).  Scores: floats (NaN = null), or with groups
    {'groups': [...], score: [per group]}."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    n, m = len(real), len(fake)
    rg, fg = real_group, fake_group
    rr = neighbours(real, real, k, rg, rg, np.arange(n))[0][:, k - 1] if n else np.zeros(0, LD)
    fr = neighbours(fake, fake, k, fg, fg, np.arange(m))[0][:, k - 1] if m else np.zeros(0, LD)
    out = {'real_radius2': rr, 'fake_radius2': fr}
    margin = np.inf
    if n and m:
        _, _, fake_inside, d_fx, ok_fx = neighbours(fake, real, 1, fg, rg, None, rr)
        nn_d2, nn_idx, real_inside, d_xf, ok_xf = neighbours(real, fake, 1, rg, fg, None, fr)
        for d2, ok, rad in ((d_fx, ok_fx, rr), (d_xf, ok_xf, fr)):
            use = ok & np.isfinite(rad)[None, :]
            if use.any():
                with np.errstate(invalid='ignore'):
                    rel = np.abs(d2 - rad[None, :]) / np.maximum(rad[None, :], np.finfo(np.float64).tiny)
                margin = min(margin, float(rel[use].min()))
        fin = np.isfinite(rr) & (nn_idx[:, 0] >= 0)
        if fin.any():
            margin = min(margin, float((np.abs(nn_d2[fin, 0] - rr[fin]) / np.maximum(rr[fin], np.finfo(np.float64).tiny)).min()))
        nn_d2, nn_idx = nn_d2[:, 0], nn_idx[:, 0]
    else:
        fake_inside, real_inside = np.zeros(m, np.int32), np.zeros(n, np.int32)
        nn_d2, nn_idx = np.full(n, np.inf, LD), np.full(n, -1, np.int32)
    out.update(fake_inside=fake_inside, real_inside=real_inside, real_nn_d2=nn_d2, real_nn_idx=nn_idx, margin=margin, n_real=n, n_fake=m)
    covered = (nn_d2 <= rr) & np.isfinite(rr)

    def scores(r_rows, f_rows):
        nr, nf = int(r_rows.sum()), int(f_rows.sum())
        if nr < k + 1 or nf < k + 1:
            return dict.fromkeys(SCORES, np.nan)
        return {'precision': float((fake_inside[f_rows] > 0).sum()) / nf, 'recall': float((real_inside[r_rows] > 0).sum()) / nr,
                'density': float(fake_inside[f_rows].astype(np.int64).sum()) / (k * nf), 'coverage': float(covered[r_rows].sum()) / nr}

    if rg is None:
        out.update(scores(np.ones(n, bool), np.ones(m, bool)))
    else:
        rg, fg = np.asarray(rg), np.asarray(fg)
        groups = np.unique(np.concatenate([rg, fg]))
        per = [scores(rg == g, fg == g) for g in groups]
        out['groups'] = groups.astype(np.int32)
        out['group_n_real'] = np.array([(rg == g).sum() for g in groups], np.int64)
        out['group_n_fake'] = np.array([(fg == g).sum() for g in groups], np.int64)
        for sc in SCORES:
            out[sc] = np.array([p[sc] for p in per], np.float64)
    return out


def d2_bound(d):
    """The relative bound of a kernel d2 against longdouble for rows of width d: lane l adds ceil(d / 64) terms, each with the rounding of
    e = q - r (counted twice: it is squared) and the one of its fma, then six butterfly adds; all terms are >= 0, so the relative errors add
    at most linearly: (ceil(d / 64) + 10) * 2^-53."""
    return ((d + 63) // 64 + 10) * 2.0 ** -53


def equal_or_nan(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
