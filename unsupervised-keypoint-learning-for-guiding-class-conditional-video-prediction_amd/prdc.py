"""Precision / recall (Kynkaanniemi et al., NeurIPS 2019) and density / coverage (Naeem et al., ICML 2020) between a real and a generated
set of rows (csrc/prdc.hip, include/kpx.h): evaluate.py --prdc.

Both pairs of scores are k-nearest-neighbour manifold estimates and need only pairwise distances.  ``set_neighbours`` is the exact fp64
all-pairs search (the general form of ``novelty.seq_nearest``: the k lowest, one skipped reference per query, per-row groups, the count of
reference balls that hold the query); ``prdc`` is four launches of it.  ``neighbours_numpy`` / ``prdc_numpy`` restate both on the CPU in
float64 with the same tie rules, and ``python -m kpx_amd.prdc prdc.npz`` re-scores the rows a run stored.  The rows are this project's own
key-point-space and recogniser-space quantities: nothing here is comparable with published figures.
"""
import json
import sys

import numpy as np

# mirrors of include/kpx.h (tests/test_prdc_cpu.py holds them equal to the header)
SET_MAX_K, SET_MAX_DIM, SET_MAX_QUERIES, SET_MAX_REFS, SET_BLOCK = 8, 16384, 4096, 1 << 20, 64
SCORES = ('precision', 'recall', 'density', 'coverage')
ROW_ARRAYS = ('real_radius2', 'fake_radius2', 'real_inside', 'fake_inside', 'real_nn_d2', 'real_nn_idx')

DEFINITION = (
    'prdc: precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) between a set X of n real rows and a '
    'set Y of m generated rows, from exact fp64 squared Euclidean distances d2 = sum (a - b)^2 (the direct form, no |a|^2 + |b|^2 - 2ab). '
    'r_k(row) = the k-th smallest d2 to the OTHER rows of its own set, +inf when fewer than k others exist; ties go to the lowest index; a '
    'row with a non-finite value is never a neighbour and lies in no ball. inside_X(y) = the number of x with d2(y, x) <= r_k(x). '
    'precision = the share of y with inside_X(y) > 0; recall = the share of x with inside_Y(x) > 0; density = sum_y inside_X(y) / (k m); '
    'coverage = the share of x whose nearest y lies within r_k(x). A set or group with fewer than k + 1 rows gives null. Spaces: kp = the '
    '32 K 2 future key points of a sequence in label coordinates (real: the pseudo labels of the real future frames, that is, the output '
    'of this project\'s own detector; fake: the motion generator\'s rollout); cls (with --action-accuracy) = the features of this '
    'project\'s own key-point recogniser (its top LSTM layer at the last step). Comparisons: draw0 = the rollouts of draw 0 against the real '
    'rows, sets of equal size (the headline); all_draws = the rollouts of every draw against the same real rows: precision and recall are '
    'unstable for unequal set sizes, read density and coverage there; ceiling = the even-numbered real samples as generated rows against '
    'the odd-numbered ones, what a perfect generator would reach at this sample size; per_class = the same with neighbours, balls and '
    'scores restricted to the rows of one action class; commanded (with --actions) = per listed class the draw-0 rollouts under that class '
    'against the real rows of that class. These are this project\'s own key-point-space and recogniser-space quantities, measured on '
    'pseudo labels and on a recogniser trained on them: they are not comparable with published precision / recall or density / coverage '
    'figures, which use image or video network embeddings, and no published figure for this dataset is quoted.')


def _error(msg):
    from ._lib import KpxError
    return KpxError(msg)


def set_neighbours(q, r, k, q_group=None, r_group=None, q_skip=None, r_radius2=None):
    """kpx_set_neighbours_f64 (include/kpx.h): q contiguous fp64 [M, D], r contiguous fp64 [N, D] on one device, 1 <= k <= 8, 1 <= D <= 16384,
    1 <= N <= 2^20; q_group int32 [M] and r_group int32 [N], both or neither: only pairs of equal group are eligible; q_skip int32 [M]: the
    reference each query leaves out (-1: none); r_radius2 fp64 [N]: the squared radius of each reference's ball -> (nn_d2 fp64 [M, k], nn_idx
    int32 [M, k], inside int32 [M] or None without radii): per query the k lexicographically lowest (d2, index) of its eligible pairs in
    ascending order (+inf / -1 in the places that stay empty) and the number of eligible references with a finite radius and d2 <= radius.
    More than 4096 queries go in several calls; a query's result does not depend on its place.  Two launches per call on the current
    stream, no atomics; every d2's bits depend on the two rows and on D alone."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= SET_MAX_K:
        raise _error('set_neighbours: k must be an integer in [1, %d] (got %r)' % (SET_MAX_K, k))
    if (q_group is None) != (r_group is None):
        raise _error('set_neighbours: q_group and r_group go together: both or neither')
    import torch
    from ._args import OPTIONAL, _ptr, _stream, check_tensors, scratch
    from ._lib import lib, check
    f64, i32 = torch.float64, torch.int32
    dev = check_tensors('set_neighbours', [('q', q, f64, (None, None), 8)])
    m, d = q.shape
    check_tensors('set_neighbours', [('r', r, f64, (None, d), 8)], dev)
    n = r.shape[0]
    if m < 1 or not 1 <= n <= SET_MAX_REFS or not 1 <= d <= SET_MAX_DIM:
        raise _error('set_neighbours: needs M >= 1 queries and 1 <= N <= %d references of 1 <= D <= %d values (got q %s, r %s)'
                     % (SET_MAX_REFS, SET_MAX_DIM, tuple(q.shape), tuple(r.shape)))
    check_tensors('set_neighbours', [('q_group', q_group, i32, (m,), *OPTIONAL), ('r_group', r_group, i32, (n,), *OPTIONAL),
                                     ('q_skip', q_skip, i32, (m,), *OPTIONAL), ('r_radius2', r_radius2, f64, (n,), 8, True)], dev)
    nn_d2 = torch.empty((m, k), dtype=f64, device=dev)
    nn_idx = torch.empty((m, k), dtype=i32, device=dev)
    inside = torch.empty((m,), dtype=i32, device=dev) if r_radius2 is not None else None
    with torch.cuda.device(dev):
        for lo in range(0, m, SET_MAX_QUERIES):
            hi = min(m, lo + SET_MAX_QUERIES)
            nbytes = lib.kpx_set_neighbours_workspace_bytes(hi - lo, n, k)
            work = scratch.get('set_neighbours', nbytes, dev)
            part = lambda t: None if t is None else t[lo:hi]     # a slice of whole rows: contiguous, and 8-byte aligned where the tensor is
            check(lib.kpx_set_neighbours_f64(q[lo:hi].data_ptr(), hi - lo, r.data_ptr(), n, d, _ptr(part(q_group)), _ptr(r_group), _ptr(part(q_skip)),
                                             _ptr(r_radius2), k, work.data_ptr(), nbytes, nn_d2[lo:hi].data_ptr(), nn_idx[lo:hi].data_ptr(),
                                             _ptr(part(inside)), _stream()), 'kpx_set_neighbours_f64')
    return nn_d2, nn_idx, inside


def neighbours_numpy(q, r, k, q_group=None, r_group=None, q_skip=None, r_radius2=None, chunk_bytes=1 << 26):
    """``set_neighbours`` on the CPU: numpy, float64, direct differences, chunked over the queries; the same eligibility and tie rules (a stable
    sort: equal d2 keep ascending index).  The distances are summed in numpy's order, not the kernel's, so they agree with it to rounding."""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    m, n = q.shape[0], r.shape[0]
    if not 1 <= k <= SET_MAX_K or (q_group is None) != (r_group is None) or q.ndim != 2 or r.ndim != 2 or q.shape[1] != r.shape[1]:
        raise ValueError('neighbours_numpy: q [M, D], r [N, D], 1 <= k <= %d, groups for both sides or neither' % SET_MAX_K)
    nn_d2, nn_idx = np.full((m, k), np.inf), np.full((m, k), -1, np.int32)
    inside = np.zeros((m,), np.int32) if r_radius2 is not None else None
    if not n:
        return nn_d2, nn_idx, inside
    rad = None if r_radius2 is None else np.asarray(r_radius2, np.float64)
    step = max(1, int(chunk_bytes // max(1, 8 * n * q.shape[1])))
    for lo in range(0, m, step):
        hi = min(m, lo + step)
        with np.errstate(invalid='ignore', over='ignore'):
            e = q[lo:hi, None, :] - r[None, :, :]
            d2 = np.einsum('mnd,mnd->mn', e, e)
        ok = np.isfinite(d2)
        if q_skip is not None:
            ok &= np.arange(n)[None, :] != np.asarray(q_skip)[lo:hi, None]
        if q_group is not None:
            ok &= np.asarray(q_group)[lo:hi, None] == np.asarray(r_group)[None, :]
        if rad is not None:
            with np.errstate(invalid='ignore'):
                inside[lo:hi] = (ok & np.isfinite(rad)[None, :] & (d2 <= rad[None, :])).sum(axis=1)
        d2 = np.where(ok, d2, np.inf)
        order = np.argsort(d2, axis=1, kind='stable')[:, :k]
        low = np.take_along_axis(d2, order, axis=1)
        kk = order.shape[1]
        nn_d2[lo:hi, :kk] = low
        nn_idx[lo:hi, :kk] = np.where(np.isfinite(low), order, -1)
    return nn_d2, nn_idx, inside


class _Torch(object):
    """the array operations ``_prdc`` needs, on device tensors"""

    def __init__(self, like):
        import torch
        self.t, self.dev = torch, like.device

    def rows(self, x):
        if x.dtype != self.t.float64 or x.dim() != 2:
            raise _error('prdc: the rows must be fp64 [n, D] tensors (got %s %s)' % (x.dtype, tuple(x.shape)))
        return x.contiguous()

    def ints(self, x):
        return x.to(self.t.int32).contiguous()

    neighbours = staticmethod(set_neighbours)

    def arange(self, n):
        return self.t.arange(n, dtype=self.t.int32, device=self.dev)

    def full(self, shape, value, kind):
        return self.t.full(shape, value, dtype=self.t.float64 if kind == 'f' else self.t.int32, device=self.dev)

    def unique_inverse(self, a, b):
        u, inv = self.t.unique(self.t.cat([a, b]), return_inverse=True)
        return u.to(self.t.int32), inv[:a.shape[0]], inv[a.shape[0]:]

    def bincount(self, idx, weights, size):
        out = self.t.zeros(size, dtype=self.t.int64, device=self.dev)
        return out.index_add_(0, idx.to(self.t.int64), weights.to(self.t.int64))

    def ratio(self, num, den, valid):
        nan = self.t.full_like(num, float('nan'), dtype=self.t.float64)
        return self.t.where(valid, num.to(self.t.float64) / den.to(self.t.float64).clamp(min=1), nan)

    def column(self, t, i):
        return t[:, i].contiguous()


class _Numpy(object):
    """the same on numpy arrays"""
    rows = staticmethod(lambda x: np.ascontiguousarray(x, np.float64))
    ints = staticmethod(lambda x: np.ascontiguousarray(x, np.int32))
    neighbours = staticmethod(neighbours_numpy)
    arange = staticmethod(lambda n: np.arange(n, dtype=np.int32))
    full = staticmethod(lambda shape, value, kind: np.full(shape, value, np.float64 if kind == 'f' else np.int32))
    column = staticmethod(lambda t, i: np.ascontiguousarray(t[:, i]))

    @staticmethod
    def unique_inverse(a, b):
        u, inv = np.unique(np.concatenate([a, b]), return_inverse=True)
        inv = inv.reshape(-1)
        return u.astype(np.int32), inv[:a.shape[0]], inv[a.shape[0]:]

    @staticmethod
    def bincount(idx, weights, size):
        out = np.zeros(size, np.int64)
        np.add.at(out, idx, np.asarray(weights, np.int64))
        return out

    @staticmethod
    def ratio(num, den, valid):
        return np.where(valid, np.asarray(num, np.float64) / np.maximum(np.asarray(den, np.float64), 1.0), np.nan)


def _prdc(x, real, fake, k, real_group, fake_group):
    real, fake = x.rows(real), x.rows(fake)
    n, m = int(real.shape[0]), int(fake.shape[0])
    if (real_group is None) != (fake_group is None):
        raise _error('prdc: real_group and fake_group go together: both or neither')
    rg, fg = (None, None) if real_group is None else (x.ints(real_group), x.ints(fake_group))
    out = {'k': k, 'n_real': n, 'n_fake': m}

    def radii(rows, count, group):
        if not count:
            return x.full((0,), np.inf, 'f')
        return x.column(x.neighbours(rows, rows, k, group, group, x.arange(count))[0], k - 1)

    out['real_radius2'], out['fake_radius2'] = radii(real, n, rg), radii(fake, m, fg)
    if n and m:
        _, _, out['fake_inside'] = x.neighbours(fake, real, 1, fg, rg, None, out['real_radius2'])
        nn_d2, nn_idx, out['real_inside'] = x.neighbours(real, fake, 1, rg, fg, None, out['fake_radius2'])
        out['real_nn_d2'], out['real_nn_idx'] = x.column(nn_d2, 0), x.column(nn_idx, 0)
    else:
        out.update(fake_inside=x.full((m,), 0, 'i'), real_inside=x.full((n,), 0, 'i'), real_nn_d2=x.full((n,), np.inf, 'f'),
                   real_nn_idx=x.full((n,), -1, 'i'))
    covered = (out['real_nn_d2'] <= out['real_radius2']) & (out['real_radius2'] < np.inf)       # a ball without a finite radius holds nothing
    hit_f, hit_r = out['fake_inside'] > 0, out['real_inside'] > 0
    if rg is None:
        ones_r, ones_f = x.full((n,), 0, 'i'), x.full((m,), 0, 'i')
        size = 1
    else:
        out['groups'], ones_r, ones_f = x.unique_inverse(rg, fg)
        size = int(out['groups'].shape[0])
    cnt_r, cnt_f = x.bincount(ones_r, ones_r * 0 + 1, size), x.bincount(ones_f, ones_f * 0 + 1, size)
    valid = (cnt_r >= k + 1) & (cnt_f >= k + 1)
    out['precision'] = x.ratio(x.bincount(ones_f, hit_f, size), cnt_f, valid)
    out['recall'] = x.ratio(x.bincount(ones_r, hit_r, size), cnt_r, valid)
    out['density'] = x.ratio(x.bincount(ones_f, out['fake_inside'], size), cnt_f * k, valid)
    out['coverage'] = x.ratio(x.bincount(ones_r, covered, size), cnt_r, valid)
    if rg is None:
        for name in SCORES:
            out[name] = out[name][0]
    else:
        out['group_n_real'], out['group_n_fake'] = cnt_r, cnt_f
    return out


def prdc(real, fake, k, real_group=None, fake_group=None):
    """Precision, recall, density and coverage (DEFINITION) of the generated rows ``fake`` fp64 [m, D] against the real rows ``real`` fp64
    [n, D], both on one device: four launches of ``set_neighbours``.  -> a dict of device tensors: the four scores (fp64, NaN = null: a set
    with fewer than k + 1 rows) and the per-row arrays real_radius2 [n], fake_radius2 [m] (r_k, +inf without k others), fake_inside [m] =
    inside_X(y), real_inside [n] = inside_Y(x), real_nn_d2 / real_nn_idx [n] = each real row's nearest generated row; k, n_real, n_fake as
    ints.  With ``real_group`` int [n] and ``fake_group`` int [m] neighbours and balls stay inside a group and the same four launches give
    the scores per group: groups int32 [G] (ascending), every score [G], group_n_real / group_n_fake [G]."""
    return _prdc(_Torch(real), real, fake, k, real_group, fake_group)


def prdc_numpy(real, fake, k, real_group=None, fake_group=None):
    """``prdc`` on the CPU through ``neighbours_numpy``: the same dict, of numpy arrays."""
    return _prdc(_Numpy, real, fake, k, real_group, fake_group)


# ------------------------------------------------------------------------------------------------ the rows of a run and their comparisons
def comparisons(store):
    """The comparisons of a store of rows, ``(name, space, real rows, fake rows, real group, fake group)`` each, as indices into the store:
    ``store`` maps '<space>_real' [S, D], '<space>_fake' [draws, S, D], 'own' [S] (the samples' classes), 'parity' [S] (0 even, 1 odd: the
    sample's number in the run mod 2) and optionally 'actions' [C] with '<space>_commanded' [C, S, D].  Works on numpy arrays and on device
    tensors alike (only indexing and reshaping)."""
    spaces = [key[:-5] for key in store if key.endswith('_real')]
    own, parity = store['own'], store['parity']
    for sp in sorted(spaces):
        real, fake = store[sp + '_real'], store[sp + '_fake']
        d, s = fake.shape[0], fake.shape[1]
        flat = fake.reshape(d * s, -1)
        own_all = own.repeat(d) if hasattr(own, 'dim') else np.tile(own, d)
        even, odd = parity == 0, parity == 1
        yield sp + '_draw0', real, fake[0], None, None
        yield sp + '_all_draws', real, flat, None, None
        yield sp + '_ceiling', real[odd], real[even], None, None
        yield sp + '_draw0_per_class', real, fake[0], own, own
        yield sp + '_all_draws_per_class', real, flat, own, own_all
        yield sp + '_ceiling_per_class', real[odd], real[even], own[odd], own[even]
        if sp + '_commanded' in store:
            for c, a in enumerate(np.asarray(store['actions'].cpu() if hasattr(store['actions'], 'cpu') else store['actions']).tolist()):
                yield '%s_commanded_%d' % (sp, a), real[own == a], store[sp + '_commanded'][c], None, None


def score_store(store, k, score=prdc_numpy):
    """Every comparison of ``comparisons(store)`` scored once with ``score`` (``prdc`` on device tensors, ``prdc_numpy`` on arrays) -> the
    ``prdc_*`` arrays of metrics.npz as numpy arrays: prdc_k, and per comparison prdc_<name>_<score>, _n_real, _n_fake, the per-row arrays
    (ROW_ARRAYS) and with groups _groups, _group_n_real, _group_n_fake."""
    host = lambda v: v.cpu().numpy() if hasattr(v, 'cpu') else np.asarray(v)
    out = {'prdc_k': np.int32(k)}
    for name, real, fake, rg, fg in comparisons(store):
        res = score(real, fake, k, rg, fg)
        for key, v in res.items():
            if key != 'k':
                out['prdc_%s_%s' % (name, key)] = host(v) if not isinstance(v, int) else np.int64(v)
    return out


def summarise(arrays):
    """The ``prdc`` block of metrics.json (DEFINITION) from the ``prdc_*`` arrays of metrics.npz; numpy only.  Scores are floats or null;
    a per_class entry lists the classes present and one value per class."""
    num = lambda v: None if not np.isfinite(v) else float(v)
    names = sorted(key[5:-len('_n_real')] for key in arrays if key.startswith('prdc_') and key.endswith('_n_real') and not key.endswith('_group_n_real'))
    out = {'definition': DEFINITION, 'k': int(arrays['prdc_k']), 'spaces': sorted({name.split('_')[0] for name in names})}
    for name in names:
        get = lambda key: np.asarray(arrays['prdc_%s_%s' % (name, key)])
        blk = {'n_real': int(get('n_real')), 'n_fake': int(get('n_fake'))}
        if 'prdc_%s_groups' % name in arrays:
            blk['classes'] = [int(v) for v in get('groups')]
            blk['class_n_real'] = [int(v) for v in get('group_n_real')]
            blk['class_n_fake'] = [int(v) for v in get('group_n_fake')]
            for sc in SCORES:
                blk[sc] = [num(v) for v in get(sc)]
        else:
            for sc in SCORES:
                blk[sc] = num(get(sc))
        space, comparison = name.split('_', 1)
        out.setdefault(space, {})[comparison] = blk
    return out


def load_store(path):
    """prdc.npz -> the store ``comparisons`` reads: the float32 rows as float64 (exact), the rest as stored"""
    with np.load(path) as f:
        return {key: (f[key].astype(np.float64) if f[key].dtype == np.float32 else f[key]) for key in f.files if key != 'k'}, \
            (int(f['k']) if 'k' in f.files else None)


def main(argv=None):
    """python -m kpx_amd.prdc prdc.npz [--k K]: the ``prdc`` block of the rows a run of evaluate.py --prdc stored, re-scored on the CPU (numpy,
    float64, the kernel's tie rules) and printed as JSON.  This project's own quantities: not comparable with published figures."""
    argv = sys.argv[1:] if argv is None else list(argv)
    k = None
    if '--k' in argv:
        at = argv.index('--k')
        try:
            k = int(argv[at + 1])
        except (IndexError, ValueError):
            argv = []
        else:
            del argv[at:at + 2]
    if len(argv) != 1 or (k is not None and not 1 <= k <= SET_MAX_K):
        print('usage: python -m kpx_amd.prdc prdc.npz [--k 1..%d]' % SET_MAX_K, file=sys.stderr)
        return 2
    store, stored_k = load_store(argv[0])
    k = k if k is not None else stored_k if stored_k is not None else 5
    print(json.dumps(summarise(score_store(store, k, prdc_numpy)), indent=1, allow_nan=False))
    return 0


if __name__ == '__main__':
    sys.exit(main())
