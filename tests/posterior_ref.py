"""Restatements for the posterior kernels (csrc/posterior.hip, include/kpx.h), numpy only: the statistics as sequential float64 / int64 loops
(the kernel's order) and in longdouble (the arbiter of the kl fields), the sampler in float64, the path in longdouble."""
import numpy as np

LD = np.longdouble
EPS32 = np.float32(1e-8)


def stats_inputs(b, v, g, seed, integer=False):
    """logit [B, 2V] (mu >= 0, sigma >= 0 as the ReLU head leaves them, some exactly 0) and groups [B] that leave some groups empty"""
    rs = np.random.RandomState(seed)
    if integer:
        logit = (rs.randint(0, 9, (b, 2 * v)) * 0.5).astype(np.float32)
    else:
        logit = np.maximum(rs.randn(b, 2 * v), 0).astype(np.float32) + (rs.rand(b, 2 * v) < 0.5) * rs.rand(b, 2 * v).astype(np.float32)
        logit = logit.astype(np.float32)
    used = [i for i in range(g) if i % 3 != 1] or [0]                  # groups 1, 4, 7 stay empty
    group = np.asarray(used, np.int32)[rs.randint(0, len(used), b)]
    return logit, group


def kl_parts(mu, sd, dtype):
    """the four parts of a kl term, each already times 0.5, in ``dtype`` from the fp32 values"""
    m, s = np.asarray(mu, np.float32).astype(dtype), np.asarray(sd, np.float32).astype(dtype)
    with np.errstate(all='ignore'):
        return 0.5 * m * m, 0.5 * s * s, -0.5 * np.log(EPS32.astype(dtype) + s * s), np.full(m.shape, -0.5, dtype)


def stats_sequential(logit, group, groups, state=None, counts=None):
    """kpx_latent_stats_add_f64 as a sequential float64 / int64 loop over b -> (state, counts, kept [B] bool); field 4 is summed from
    numpy's float64 log (the kernel's agrees with it to the rounding of log) and is judged against ``stats_longdouble`` instead"""
    b, v = logit.shape[0], logit.shape[1] // 2
    state = np.zeros((groups, v, 8), np.float64) if state is None else state.copy()
    counts = np.zeros((groups, 3), np.int64) if counts is None else counts.copy()
    kept = np.zeros(b, bool)
    for i in range(b):
        g = 0 if group is None else int(group[i])
        if not 0 <= g < groups:
            counts[0, 2] += 1
            continue
        if not np.isfinite(logit[i]).all():
            counts[g, 1] += 1
            continue
        mu, sd = logit[i, :v], logit[i, v:]
        m, s = mu.astype(np.float64), sd.astype(np.float64)
        kl = 0.5 * ((((m * m) + s * s) - np.log(np.float64(EPS32) + s * s)) - 1.0)
        for f, term in enumerate((m, m * m, s, s * s, kl, (mu == 0) * 1.0, (sd == 0) * 1.0, np.ones(v))):
            state[g, :, f] += term
        counts[g, 0] += 1
        kept[i] = True
    return state, counts, kept


def stats_longdouble(logit, group, groups):
    """-> (sum kl [G, V], sum |parts| [G, V], kl_rows [B], sum |parts| per row [B]) in longdouble over the rows that count"""
    b, v = logit.shape[0], logit.shape[1] // 2
    skl, sabs = np.zeros((groups, v), LD), np.zeros((groups, v), LD)
    rows, rows_abs = np.full(b, np.nan, LD), np.full(b, np.nan, LD)
    for i in range(b):
        g = 0 if group is None else int(group[i])
        if not 0 <= g < groups or not np.isfinite(logit[i]).all():
            continue
        parts = kl_parts(logit[i, :v], logit[i, v:], LD)
        kl, mag = sum(parts), sum(np.abs(p) for p in parts)
        skl[g] += kl
        sabs[g] += mag
        rows[i], rows_abs[i] = kl.sum(), mag.sum()
    return skl, sabs, rows, rows_abs


def sample_f64(logit, eps, tau):
    """z in float64: mu + fl32(tau sigma) eps, the product and the sum exact to float64's rounding"""
    v = logit.shape[1] // 2
    ts = (np.float32(tau) * logit[:, v:]).astype(np.float32)
    return logit[:, :v].astype(np.float64) + ts.astype(np.float64) * eps.astype(np.float64)


def ulp32(x):
    """the spacing of float32 at |x| (of the binade |x| lies in), as float64"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def path_longdouble(za, zb, steps, mode):
    """-> (out [S, B, V] longdouble, lerp_rows [B] bool: the rows that fall back); ends are za and zb"""
    a, c = za.astype(LD), zb.astype(LD)
    b, v = a.shape
    out = np.zeros((steps, b, v), LD)
    fallback = np.zeros(b, bool)
    for i in range(b):
        aa, cc, ac = (a[i] * a[i]).sum(), (c[i] * c[i]).sum(), (a[i] * c[i]).sum()
        omega = sin_omega = None
        if mode == 'slerp' and aa > 0 and cc > 0:
            omega = np.arccos(np.clip(ac / (np.sqrt(aa) * np.sqrt(cc)), LD(-1), LD(1)))
            sin_omega = np.sin(omega)
        slerp = sin_omega is not None and sin_omega >= 1e-6
        fallback[i] = mode == 'slerp' and not slerp
        for s in range(steps):
            t = LD(s) / LD(steps - 1)
            if slerp:
                out[s, i] = np.sin((1 - t) * omega) / sin_omega * a[i] + np.sin(t * omega) / sin_omega * c[i]
            else:
                out[s, i] = (1 - t) * a[i] + t * c[i]
    out[0], out[steps - 1] = a, c
    return out, fallback
