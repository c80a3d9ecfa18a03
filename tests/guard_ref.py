"""Float64 restatements and planted inputs for the step guard (csrc/guard.hip: kpx_grad_health_f32, kpx_adam_tf_flat_guarded_f32,
kpx_guard_restore_f32); shared by test_guard_cpu.py and test_guard_gpu.py.

Health: every fp32 value squares exactly in float64, so a fixed-order float64 sum of the n squares differs from the exact sum by at most
(n-1) roundings of a partial sum that never exceeds the total (every term is non-negative): (n-1) * 2^-53 relative.  ``health`` takes the
accumulator's dtype: float64 is the restatement, longdouble the value the bound is measured against.  The count of non-finite values and
the largest finite magnitude are exact in any order.
"""
import numpy as np

import loss_optim_ref as L

F32 = np.float32
HEALTH_SLAB = 16384                                    # elements per workgroup slab of the health pass (csrc/guard.hip)
SIZES = (1, 3, 4, 5, 255, 256, 257, 4100, L.ADAM_GRID_ELEMS + 1027)
OFFSETS = (0, 1)                                       # floats past a 16-byte boundary: the 16-byte and the 4-byte load path
BAD_VALUES = (np.nan, np.inf, -np.inf)
PLANT_KINDS = ('nowhere', 'first', 'last', 'slab')
RESTORE_SIZES = (1, 5, 4100)


def plant_positions(n, kind):
    """Element indices that receive a non-finite value: none; element 0; element n-1; both sides of every slab boundary inside [0, n)
    that the first and the last slab touch."""
    if kind == 'nowhere':
        return []
    if kind == 'first':
        return [0]
    if kind == 'last':
        return [n - 1]
    edges = sorted({HEALTH_SLAB, (n - 1) // HEALTH_SLAB * HEALTH_SLAB} - {0})
    return [i for e in edges for i in (e - 1, e) if 0 < e < n]


HEALTH_CASES = [(n, kind) for n in SIZES for kind in PLANT_KINDS if kind == 'nowhere' or plant_positions(n, kind)]


def health_clean(n, seed=0):
    """n finite fp32 values whose magnitudes run from 1e-30 to 1e30: their squares span 1e-60 .. 1e60, far outside fp32 and well inside
    float64, so a sum of squares kept in fp32 anywhere would flush or overflow."""
    rs = np.random.RandomState(9000 + seed + n % 1009)
    mag = 10.0 ** rs.uniform(-30.0, 30.0, size=n)
    g = (rs.choice([-1.0, 1.0], size=n) * mag * rs.uniform(1.0, 2.0, size=n)).astype(F32)
    if n >= 4:
        g[1], g[2] = F32(1e-30), F32(-1e30)
    assert np.all(np.isfinite(g))
    return g


def health_planted(n, kind, value, seed=0):
    g = health_clean(n, seed)
    for i in plant_positions(n, kind):
        g[i] = F32(value)
    return g


def health(g, dtype=np.float64):
    """-> (nonfinite, sumsq, maxabs) of an fp32 vector; sumsq accumulated in ``dtype``, non-finite values counted and left out."""
    g = np.ascontiguousarray(g, dtype=F32).ravel()
    ok = np.isfinite(g)
    fin = g[ok].astype(dtype)
    sumsq = (fin * fin).sum(dtype=dtype) if fin.size else dtype(0)
    maxabs = F32(np.abs(g[ok]).max()) if fin.size else F32(0)
    return int(g.size - int(ok.sum())), sumsq, maxabs


def sumsq_bound(n, ref):
    """|fixed-order float64 sum - exact| <= (n-1) 2^-53 * exact; the longdouble reference adds its own (n-1) 2^-64 at the most."""
    return (max(n - 1, 0) * (2.0 ** -53 + 2.0 ** -64)) * float(ref)


def new_counters():
    return dict(skipped_total=0, skipped_run=0, updates=0)


def guarded_adam(p, g, m, v, alpha, nonfinite, counters, gscale=1.0, dtype=np.float64):
    """kpx_adam_tf_flat_guarded_f32 on top of loss_optim_ref.adam_step -> ((p', m', v'), counters')."""
    c = dict(counters, updates=counters['updates'] + 1)
    if nonfinite:
        c['skipped_total'] += 1
        c['skipped_run'] += 1
        return tuple(np.asarray(x).astype(dtype) for x in (p, m, v)), c
    c['skipped_run'] = 0
    return L.adam_step(p, g, m, v, alpha, gscale=gscale, dtype=dtype), c


def restore(dst, src, nonfinite):
    """kpx_guard_restore_f32: src's bits when the record counts a non-finite value, dst's own otherwise."""
    return np.array(src if nonfinite else dst, dtype=F32, copy=True)
