"""Float64 restatement of the clipped Adam update (csrc/guard.hip: kpx_adam_tf_flat_clipped_f32) = tf.clip_by_global_norm over one bucket in
front of ApplyAdam; shared by test_clip_cpu.py and test_clip_gpu.py.  Imports nothing from the package under test.

N = gscale * sqrt(sum g^2); N <= clip: the guarded update with gs = gscale and scale = 1; otherwise gs = gscale * clip / N and
scale = clip / N.  A non-finite count skips as guard_ref.guarded_adam does and leaves the clip state alone.

Bound on the reported scale (fixed before measuring): the kernel takes N from a fixed-order float64 sum, which guard_ref.sumsq_bound allows
(n-1)(2^-53 + 2^-64) relative, and rounds clip / N to fp32 once: one fp32 ulp of the scale plus that relative slack.
"""
import numpy as np

import guard_ref as G
import loss_optim_ref as L

F32 = np.float32


def sumsq(g, dtype=np.float64):
    d = np.asarray(g, dtype=F32).ravel().astype(dtype)
    return (d * d).sum(dtype=dtype)


def clip_scale(sumsq_, clip_norm, gscale=1.0):
    """-> (N, scale, gs) in float64; clip_norm and gscale cross the C ABI as fp32."""
    gs0, c = np.float64(F32(gscale)), np.float64(F32(clip_norm))
    norm = gs0 * np.sqrt(np.float64(sumsq_))
    if norm <= c:
        return norm, np.float64(1.0), gs0
    return norm, c / norm, gs0 * (c / norm)


def scale_bound(n, scale):
    return float(np.spacing(F32(scale))) + G.sumsq_bound(n, 1.0) * float(scale)


def new_state():
    return dict(norm=0.0, scale=0.0, clipped_total=0)


def clipped_adam(p, g, m, v, alpha, nonfinite, clip_norm, counters, state, gscale=1.0, dtype=np.float64):
    """-> ((p', m', v'), counters', state').  ``g`` holds the finite values the sum runs over (the callers plant nothing when nonfinite == 0)."""
    if nonfinite:
        out, c = G.guarded_adam(p, g, m, v, alpha, nonfinite, counters, dtype=dtype)
        return out, c, dict(state)
    norm, scale, gs = clip_scale(sumsq(g), clip_norm, gscale)
    out, c = G.guarded_adam(p, g, m, v, alpha, 0, counters, gscale=gs, dtype=dtype)
    return out, c, dict(norm=float(norm), scale=float(scale), clipped_total=state['clipped_total'] + int(scale < 1.0))
