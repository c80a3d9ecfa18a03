"""Fréchet distance between sets of frames (and of rollouts) in the feature space of this project's VGG19 (evaluate.py --frechet,
DESIGN.md section 2).  Not FID and not FVD: those are defined on Inception / I3D features, which this project does not have; the figures
here are comparable with one another only.

Device side (``FrechetAccumulator``): per feature layer the pooled features of a frame (``ops.feature_pool``: the mean over positions, fp64)
are one row of the *frame* level; a rollout of T frames gives one row of the *video* level, concat(mean_t p_t, mean_t |p_{t+1} - p_t|).  The
rows go into fp64 first and second moments in HBM (``ops.moments_add``), in place across batches and draws.  Host side (numpy float64, no
scipy): ``stats`` -> mean and covariance, ``frechet_distance``, and ``python -m kpx_amd.frechet a.npz b.npz`` to compare the ``frechet.npz``
of two runs without a GPU.
"""
import sys

import numpy as np

LEVELS = ('frame', 'video')


def frechet_distance(m1, c1, m2, c2):
    """|m1 - m2|^2 + tr c1 + tr c2 - 2 sum_i sqrt(max(l_i, 0)), l = eigvalsh(S c2 S), S = c1^(1/2) by eigh with negative eigenvalues clamped
    to 0 (the l_i are the eigenvalues of c1 c2, taken from a symmetric matrix).  float64; NaN where a covariance is None (fewer than two
    rows).  The result is not clamped at 0: for equal statistics it is the rounding error of the computation, of either sign."""
    if c1 is None or c2 is None:
        return float('nan')
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    w, q = np.linalg.eigh(c1)
    s = (q * np.sqrt(np.maximum(w, 0.0))) @ q.T
    lam = np.linalg.eigvalsh(s @ c2 @ s)
    d = m1 - m2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def stats_from_moments(n, total, outer):
    """{n, mean, cov} of n rows from their sum [D] and their sum of outer products [D,D]: cov = (outer - n mu mu^T) / (n - 1), None for
    n < 2; mean None for n < 1.  float64."""
    n = int(round(float(n)))
    total, outer = np.asarray(total, np.float64), np.asarray(outer, np.float64)
    if n < 1:
        return {'n': n, 'mean': None, 'cov': None}
    mean = total / n
    cov = (outer - n * np.outer(mean, mean)) / (n - 1) if n >= 2 else None
    return {'n': n, 'mean': mean, 'cov': cov}


def video_descriptor(pooled, frames_per_video):
    """pooled fp64 [B * T, C] (torch) -> [B, 2 C]: per rollout of T frames concat(mean_t p_t, mean_{t < T - 1} |p_{t+1} - p_t|); the second
    half is 0 for a frozen pose (and for T = 1).  A few KB of torch glue in fp64."""
    import torch
    t = int(frames_per_video)
    p = pooled.view(-1, t, pooled.shape[1])
    motion = (p[:, 1:] - p[:, :-1]).abs().mean(dim=1) if t > 1 else torch.zeros_like(p[:, 0])
    return torch.cat([p.mean(dim=1), motion], dim=1).contiguous()


def pool_features(feats):
    """one layer list of fp32 [N,H,W,C] features -> the list of their pooled fp64 [N,C] rows (ops.feature_pool)"""
    from . import ops
    return [ops.feature_pool(f) for f in feats]


class FrechetAccumulator:
    """First and second moments of pooled features, per layer (``dims``: the channel counts C) and level: device fp64 ``n`` (a scalar), ``sum``
    [D] and ``outer`` [D,D] with D = C (frame) and 2 C (video).  ``add(feats, frames_per_video)`` pools one layer list of fp32 NHWC features
    of B * frames_per_video frames and adds both levels; moments are additive, so ``merge`` is an element-wise add."""

    def __init__(self, dims, device):
        import torch
        self.dims = [int(c) for c in dims]
        self.device = torch.device(device)
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=self.device)
        self.moments = {level: [{'n': z(), 'sum': z(d), 'outer': z(d, d)} for d in self.level_dims(level)] for level in LEVELS}

    def level_dims(self, level):
        return [c if level == 'frame' else 2 * c for c in self.dims]

    def add(self, feats, frames_per_video=None):
        self.add_pooled(pool_features(feats), frames_per_video)

    def add_pooled(self, pooled, frames_per_video=None):
        """pooled: per layer fp64 [N,C] rows on the accumulator's device, N a multiple of frames_per_video (None: one video of N frames)"""
        from . import _lib, ops
        if len(pooled) != len(self.dims) or any(p.dim() != 2 or p.shape[1] != c or p.shape[0] != pooled[0].shape[0]
                                                for p, c in zip(pooled, self.dims)):
            raise _lib.KpxError('FrechetAccumulator: needs one [N,C] tensor per layer with C = %s (got %s)'
                                % (self.dims, [tuple(p.shape) for p in pooled]))
        n = pooled[0].shape[0]
        t = n if frames_per_video is None else int(frames_per_video)
        if n < 1 or t < 1 or n % t:
            raise _lib.KpxError('FrechetAccumulator: %d frames do not split into videos of %d frames' % (n, t))
        for layer, p in enumerate(pooled):
            for level, rows in (('frame', p), ('video', video_descriptor(p, t))):
                m = self.moments[level][layer]
                ops.moments_add(rows, m['sum'], m['outer'])
                m['n'] += rows.shape[0]

    def add_moments(self, level, layer, n, total, outer):
        """moments computed elsewhere (another accumulator's, or a host's) into this one: an element-wise add"""
        import torch
        m = self.moments[level][layer]
        as_t = lambda v: torch.as_tensor(np.asarray(v, np.float64) if not torch.is_tensor(v) else v, dtype=torch.float64).to(self.device)
        m['n'] += as_t(n)
        m['sum'] += as_t(total)
        m['outer'] += as_t(outer)

    def merge(self, other):
        if other.dims != self.dims:
            raise ValueError('FrechetAccumulator.merge: layer widths differ (%s, %s)' % (self.dims, other.dims))
        for level in LEVELS:
            for layer, m in enumerate(other.moments[level]):
                self.add_moments(level, layer, m['n'], m['sum'], m['outer'])
        return self

    def stats(self):
        """-> {level: [per layer {n, mean, cov}]} as host float64 (one copy per tensor); cov None for n < 2"""
        return {level: [stats_from_moments(m['n'].item(), m['sum'].cpu().numpy(), m['outer'].cpu().numpy()) for m in self.moments[level]]
                for level in LEVELS}


class FrechetSplit:
    """Routes the videos of a batch to several accumulators in turn: video v of the batch (global index ``first_video`` + v) goes to
    ``accumulators[(first_video + v) % len(accumulators)]``.  evaluate.py --frechet splits the real samples into even and odd ones this way:
    the distance between the two halves is the finite-sample noise floor."""

    def __init__(self, accumulators, first_video=0):
        self.accumulators, self.first_video = list(accumulators), int(first_video)

    def add(self, feats, frames_per_video=None):
        self.add_pooled(pool_features(feats), frames_per_video)

    def add_pooled(self, pooled, frames_per_video=None):
        n = pooled[0].shape[0]
        t = n if frames_per_video is None else int(frames_per_video)
        k = len(self.accumulators)
        for i, acc in enumerate(self.accumulators):
            start = (i - self.first_video) % k                         # the first video of this batch that belongs to accumulator i
            part = [p.view(-1, t, p.shape[1])[start::k].reshape(-1, p.shape[1]).contiguous() for p in pooled]
            if part[0].shape[0]:
                acc.add_pooled(part, t)


def layer_distances(a, b, level):
    """stats() of two accumulators -> float64 [layers]: the Fréchet distance per layer at ``level``, NaN where either side has n < 2"""
    return np.array([frechet_distance(x['mean'], x['cov'], y['mean'], y['cov']) for x, y in zip(a[level], b[level])], np.float64)


def stats_arrays(prefix, stats, layers):
    """the entries of frechet.npz for one set: <prefix>_<level>_<layer>_{n, mean, cov}; an absent mean / cov is stored as an empty array"""
    out = {}
    for level in LEVELS:
        for name, s in zip(layers, stats[level]):
            key = '%s_%s_%s_' % (prefix, level, name)
            out[key + 'n'] = np.int64(s['n'])
            out[key + 'mean'] = s['mean'] if s['mean'] is not None else np.zeros((0,), np.float64)
            out[key + 'cov'] = s['cov'] if s['cov'] is not None else np.zeros((0, 0), np.float64)
    return out


def stats_from_arrays(npz, prefix, layers):
    """the inverse of stats_arrays on a loaded frechet.npz"""
    out = {}
    for level in LEVELS:
        out[level] = []
        for name in layers:
            key = '%s_%s_%s_' % (prefix, level, name)
            mean, cov = np.asarray(npz[key + 'mean']), np.asarray(npz[key + 'cov'])
            out[level].append({'n': int(npz[key + 'n']), 'mean': mean if mean.size else None, 'cov': cov if cov.size else None})
    return out


def main(argv=None):
    """python -m kpx_amd.frechet a.npz b.npz [set_a [set_b]]: the distances between two runs' stored statistics (sets: real, pred; default
    pred against pred), per layer and level.  This project's VGG19 quantity: not FID, not FVD."""
    argv = sys.argv[1:] if argv is None else list(argv)
    if not 2 <= len(argv) <= 4:
        print('usage: python -m kpx_amd.frechet a.npz b.npz [real|pred [real|pred]]', file=sys.stderr)
        return 2
    set_a = argv[2] if len(argv) > 2 else 'pred'
    set_b = argv[3] if len(argv) > 3 else set_a
    a, b = np.load(argv[0]), np.load(argv[1])
    layers = [str(v) for v in a['layers']]
    if layers != [str(v) for v in b['layers']]:
        print('the two files hold different layers', file=sys.stderr)
        return 2
    sa, sb = stats_from_arrays(a, set_a, layers), stats_from_arrays(b, set_b, layers)
    print('Frechet distance in VGG19 feature space (this project\'s quantity; not FID/FVD): %s[%s] against %s[%s]' % (argv[0], set_a, argv[1], set_b))
    for level in LEVELS:
        d = layer_distances(sa, sb, level)
        for name, v, x, y in zip(layers, d, sa[level], sb[level]):
            print('%-5s %-8s n = %d / %d  D = %-4d  %s' % (level, name, x['n'], y['n'], 0 if x['mean'] is None else x['mean'].size, repr(float(v))))
    return 0


if __name__ == '__main__':
    sys.exit(main())
