"""GPU: the posterior kernels (csrc/posterior.hip) against the restatements of tests/posterior_ref.py -- the statistics bit for bit where
fp64 sums of fp32 values allow it and within a derived bound for the kl fields, in pieces, with dead units, bad rows, odd bases, guards and
graph replay; the sampler against the training kernel's z; the path against longdouble and in its fall-backs -- then FinalModel.encode
against the oracle in float64, evaluate.py --posterior and animate.py --interpolate / --motion-from end to end."""
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref
import motion_metrics_ref as M
import posterior_ref as P
import sheet_ref
from oracle import restatement as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U = 2.0 ** -53
STATS_SHAPES = [(1, 1, 1), (3, 5, 1), (64, 64, 9), (65, 100, 9), (257, 64, 3)]
SAMPLE_SHAPES = [(1, 1), (3, 5), (64, 64), (65, 100)]
PATH_SHAPES = [(1, 1), (3, 5), (2, 64), (1, 1000)]
ids = lambda shapes: ['x'.join(map(str, s)) for s in shapes]


def _ops():
    from kpx_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _stats(logit, group, g, pieces=None, rows=True):
    """ops.latent_stats_add over the rows in ``pieces`` (row counts, default one call) -> (state, counts, kl_rows) on the host"""
    from kpx_amd import posterior
    ops = _ops()
    b, v = logit.shape[0], logit.shape[1] // 2
    state, counts = posterior.new_state(g, v, DEV)
    out, lo = [], 0
    for n in pieces or [b]:
        if n:
            out.append(ops.latent_stats_add(_dev(logit[lo:lo + n]), state, counts, None if group is None else _dev(group[lo:lo + n])))
        lo += n
    assert lo == b
    return state.cpu().numpy(), counts.cpu().numpy(), torch.cat(out).cpu().numpy()


# ------------------------------------------------------------------------------------------------ kpx_latent_stats_add_f64
@pytest.mark.parametrize('shape', STATS_SHAPES, ids=ids(STATS_SHAPES))
def test_stats_match_the_sequential_restatement(shape):
    """integer-valued inputs: the seven polynomial and count fields and counts bit for bit; normal inputs: the four polynomial sums (and the
    counters) bit for bit; sum kl and kl_rows within (n + 8) 2^-53 sum |parts| of longdouble, n the rows of the column: n additions of the
    fixed-order sum, and per term the roundings of mu^2 + sigma^2, of 1e-8 + sigma^2 (an absolute error of one unit in the log), of the
    fp64 log itself, and of the two subtractions -- derived, not measured.  kl_rows: the same bound with the n of the row's columns (its
    V terms are added as a tree of depth 6 plus one addition per further wavefront, two at these sizes)."""
    b, v, g = shape
    for integer in (True, False):
        logit, group = P.stats_inputs(b, v, g, seed=b * 7 + v, integer=integer)
        grp = None if g == 1 else group
        state, counts, kl_rows = _stats(logit, grp, g)
        want, want_counts, kept = P.stats_sequential(logit, grp, g)
        assert np.array_equal(counts, want_counts) and counts[:, 0].sum() == b and kept.all()
        if g > 1:
            assert (counts[1::3, 0] == 0).all() and (state[1::3] == 0).all()          # the groups left empty
        for f in (0, 1, 2, 3, 5, 6, 7):
            assert _same_bits(state[:, :, f], want[:, :, f]), (shape, integer, f)
        assert (state[:, :, 5] > 0).any() or b * v < 64                                # exact zeros do occur
        skl, sabs, rows, rows_abs = P.stats_longdouble(logit, grp, g)
        n = state[:, :, 7]
        err = np.abs(state[:, :, 4].astype(P.LD) - skl).astype(np.float64)
        bound = ((n + 8) * U * sabs).astype(np.float64)
        print('%s integer=%s: sum kl error / bound max %.3f' % (shape, integer, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), (shape, integer)
        n_row = counts[:, 0][0 if grp is None else grp]
        err = np.abs(kl_rows.astype(P.LD) - rows).astype(np.float64)
        bound = ((n_row + 8) * U * rows_abs).astype(np.float64)
        print('%s integer=%s: kl_rows error / bound max %.3f' % (shape, integer, float((err / bound).max())))
        assert np.isfinite(kl_rows).all() and (err <= bound).all(), (shape, integer)


@pytest.mark.parametrize('shape', STATS_SHAPES, ids=ids(STATS_SHAPES))
def test_stats_in_pieces_leave_the_bits_of_one_call(shape):
    b, v, g = shape
    logit, group = P.stats_inputs(b, v, g, seed=b + 3 * v)
    if b > 2:
        logit[1, v - 1] = np.inf                                       # a row left out rides along
        group[b - 1] = g
    grp = None if g == 1 else group
    whole = _stats(logit, grp, g)
    for pieces in ([1, b - 1], [b // 2, b - b // 2]):
        got = _stats(logit, grp, g, pieces)
        for a, w, name in zip(got, whole, ('state', 'counts', 'kl_rows')):
            assert _same_bits(a, w), (shape, pieces, name)


def test_stats_of_dead_units_stay_finite_and_are_counted():
    v = 5
    logit = np.array([[0.5, 0, 1, 2, 0] + [0, 0, 1, 0.25, 0],          # sigma = 0 at 0, 1, 4; mu = sigma = 0 at 1 and 4
                      [0, 0, 3, 0, -0.0] + [0, 1, 0, 0, -0.0]], np.float32)
    state, counts, kl_rows = _stats(logit, None, 1)
    assert np.isfinite(state).all() and np.isfinite(kl_rows).all() and counts.tolist() == [[2, 0, 0]]
    assert state[0, :, 5].tolist() == [1, 2, 0, 1, 2] and state[0, :, 6].tolist() == [2, 1, 1, 1, 2] and (state[0, :, 7] == 2).all()
    dead = 0.5 * (-np.log(np.float64(np.float32(1e-8))) - 1.0)
    assert abs(state[0, 4, 4] - 2 * dead) <= 4 * U * 40 and abs(state[0, 0, 4] - (2 * dead + 0.125)) <= 4 * U * 40
    want = P.stats_sequential(logit, None, 1)[0]
    for f in (0, 1, 2, 3, 5, 6, 7):
        assert _same_bits(state[:, :, f], want[:, :, f]), f


def test_bad_rows_leave_no_trace_but_their_counter():
    b, v, g = 9, 6, 3
    logit, group = P.stats_inputs(b, v, g, seed=5)
    group[:] = [0, 2, 0, 2, 2, 0, 0, 2, 0]
    clean_rows = [0, 2, 5, 8]
    bad = logit.copy()
    bad[1, 2] = np.nan
    bad[3, v + 1] = np.inf
    bad[4, 0] = -np.inf
    bad_group = group.copy()
    bad_group[6], bad_group[7] = -1, g
    bad[7, 3] = np.nan                                                 # a bad group is met first: the values are not looked at
    state, counts, kl_rows = _stats(bad, bad_group, g)
    want = _stats(logit[clean_rows], group[clean_rows], g)
    assert _same_bits(state, want[0])
    assert counts.tolist() == [[4, 0, 2], [0, 0, 0], [0, 3, 0]]
    assert np.array_equal(np.isnan(kl_rows), ~np.isin(np.arange(b), clean_rows)) and _same_bits(kl_rows[clean_rows], want[2])


def test_stats_with_odd_bases_and_guards():
    """logit based 4 bytes past a 16-byte boundary; guard words around state, counts and kl_rows"""
    ops = _ops()
    b, v, g = 7, 9, 2
    logit, group = P.stats_inputs(b, v, g, seed=8)
    group[:] = [0, 1, 1, 0, 1, 0, 0]
    buf = torch.empty(b * 2 * v + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    lg = buf[1:1 + b * 2 * v].view(b, 2 * v)
    lg.copy_(_dev(logit))
    assert lg.data_ptr() % 16 == 4
    gs = torch.full((g * v * 8 + 16,), -7.0, dtype=torch.float64, device=DEV)
    gc = torch.full((g * 3 + 16,), -7, dtype=torch.int64, device=DEV)
    gk = torch.full((b + 16,), -7.0, dtype=torch.float64, device=DEV)
    state, counts, rows = gs[8:8 + g * v * 8].view(g, v, 8), gc[8:8 + g * 3].view(g, 3), gk[8:8 + b]
    state.zero_()
    counts.zero_()
    assert ops.latent_stats_add(lg, state, counts, _dev(group), kl_rows=rows) is rows
    want = _stats(logit, group, g)
    assert _same_bits(state.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1]) and _same_bits(rows.cpu().numpy(), want[2])
    for guard, n in ((gs, g * v * 8), (gc, g * 3), (gk, b)):
        h = guard.cpu().numpy()
        assert (h[:8] == -7).all() and (h[8 + n:] == -7).all()


def test_latent_launches_replay_from_a_graph_bit_for_bit():
    ops = _ops()
    b, v, g, s = 6, 70, 3, 5
    logit, group = P.stats_inputs(b, v, g, seed=12)
    lg, gr = _dev(logit), _dev(group)
    eps = _dev(np.random.RandomState(2).randn(b, v).astype(np.float32))
    from kpx_amd import posterior
    state, counts = posterior.new_state(g, v, DEV)
    rows, z, path = torch.empty(b, dtype=torch.float64, device=DEV), torch.empty((b, v), device=DEV), torch.empty((s, b, v), device=DEV)

    def enqueue():
        ops.latent_stats_add(lg, state, counts, gr, kl_rows=rows)
        ops.latent_sample(lg, eps, 0.5, out=z)
        ops.latent_path(z, eps, s, 'slerp', out=path)

    enqueue()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (state, counts, rows, z, path)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    state.zero_()
    counts.zero_()
    for t in (rows, z, path):
        t.fill_(77.0)
    graph.replay()
    torch.cuda.synchronize()
    for t, e in zip((state, counts, rows, z, path), eager):
        assert _same_bits(t.cpu().numpy(), e.cpu().numpy())


def test_bad_arguments_raise_kpx_error_and_launch_nothing():
    from kpx_amd import _lib, posterior
    from kpx_amd._lib import KpxError
    ops = _ops()
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=DEV)
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    logit, group = z(f32, 3, 10), z(i32, 3)
    state, counts = posterior.new_state(2, 5, DEV)
    state.fill_(5.0)
    za, out = z(f32, 3, 5), torch.full((4, 3, 5), 5.0, device=DEV)
    bad = [lambda: ops.latent_stats_add(z(f32, 3, 0), z(f64, 2, 0, 8), counts, group),                    # V = 0
           lambda: ops.latent_stats_add(z(f32, 3, 2050), z(f64, 2, 1025, 8), counts, group),              # V = 1025
           lambda: ops.latent_stats_add(logit, z(f64, 0, 5, 8), z(i64, 0, 3), group),                     # G = 0
           lambda: ops.latent_stats_add(logit, state, counts),                                            # G = 2 without groups
           lambda: ops.latent_stats_add(logit.double(), state, counts, group),                            # dtypes
           lambda: ops.latent_stats_add(logit, state.float(), counts, group),
           lambda: ops.latent_stats_add(logit, state, counts.int(), group),
           lambda: ops.latent_stats_add(logit, state, counts, group.long()),
           lambda: ops.latent_stats_add(logit, state, counts, group, kl_rows=z(f32, 3)),
           lambda: ops.latent_stats_add(logit, z(f64, 2, 4, 8), counts, group),                           # shapes
           lambda: ops.latent_stats_add(logit, z(f64, 2, 5, 7), counts, group),
           lambda: ops.latent_stats_add(logit, state, z(i64, 2, 2), group),
           lambda: ops.latent_stats_add(logit, state, counts, z(i32, 4)),
           lambda: ops.latent_stats_add(logit, state, counts, group, kl_rows=z(f64, 4)),
           lambda: ops.latent_stats_add(z(f32, 3, 20)[:, ::2], state, counts, group),                     # contiguity
           lambda: ops.latent_stats_add(logit.cpu(), state, counts, group),                               # CPU tensors
           lambda: ops.latent_stats_add(logit, state.cpu(), counts, group),
           lambda: ops.latent_stats_add(logit, state, counts, group.cpu()),
           lambda: ops.latent_sample(logit, z(f32, 3, 4)),
           lambda: ops.latent_sample(logit, z(f64, 3, 5)),
           lambda: ops.latent_sample(logit, za.cpu()),
           lambda: ops.latent_sample(logit, None, float('inf')),
           lambda: ops.latent_sample(logit, None, 0.0, out=z(f32, 3, 4)),
           lambda: ops.latent_sample(z(f32, 3, 2050), None),
           lambda: ops.latent_path(za, z(f32, 2, 5), 4, out=out),
           lambda: ops.latent_path(za, za.double(), 4, out=out),
           lambda: ops.latent_path(za, za, 5, out=out),
           lambda: ops.latent_path(za, za, 1), lambda: ops.latent_path(za, za, 65), lambda: ops.latent_path(za, za, 4, 'linear', out=out),
           lambda: ops.latent_path(za.cpu(), za, 4, out=out), lambda: ops.latent_path(z(f32, 1, 1025), z(f32, 1, 1025), 2)]
    launched = _lib.abi_calls[0]
    for i, fn in enumerate(bad):
        with pytest.raises(KpxError):
            fn()
            pytest.fail('case %d raised nothing' % i)
    assert _lib.abi_calls[0] == launched
    assert bool((state == 5.0).all()) and bool((counts == 0).all()) and bool((out == 5.0).all())


@pytest.mark.parametrize('shape', SAMPLE_SHAPES, ids=ids(SAMPLE_SHAPES))
def test_stats_agree_with_the_training_kernels_kl(shape):
    """the fp32 scalar of kpx_vae_sample_kl_fwd_f32 against sum_v sum kl / n on the same logits, within 2^-21 sum(mu^2 + sigma^2 + |log(1e-8 +
    sigma^2)| + 1) / (2 B): four fp32 roundings and a one-to-two-ulp logf per term"""
    from kpx_amd._lib import lib
    ops = _ops()
    b, v = shape
    logit, _ = P.stats_inputs(b, v, 1, seed=3 * b + v)
    lg, eps = _dev(logit), torch.zeros((b, v), device=DEV)
    zt, kl = torch.empty((b, v), device=DEV), torch.empty(1, device=DEV)
    assert lib.kpx_vae_sample_kl_fwd_f32(lg.data_ptr(), eps.data_ptr(), zt.data_ptr(), kl.data_ptr(), b, v, ops._stream()) == 0
    state, counts, _ = _stats(logit, None, 1)
    mine = state[0, :, 4].sum() / counts[0, 0]
    m, s = logit[:, :v].astype(np.float64), logit[:, v:].astype(np.float64)
    bound = 2.0 ** -21 * (m * m + s * s + np.abs(np.log(np.float64(np.float32(1e-8)) + s * s)) + 1).sum() / (2 * b)
    print('%s: |training - stats| = %.3e, bound %.3e' % (shape, abs(float(kl.cpu()[0]) - mine), bound))
    assert abs(float(kl.cpu()[0]) - mine) <= bound


# ------------------------------------------------------------------------------------------------ kpx_latent_sample_f32
@pytest.mark.parametrize('shape', SAMPLE_SHAPES, ids=ids(SAMPLE_SHAPES))
def test_sample(shape):
    from kpx_amd._lib import lib
    ops = _ops()
    b, v = shape
    rs = np.random.RandomState(b + v)
    logit, _ = P.stats_inputs(b, v, 1, seed=b * 5 + v)
    logit[:, :v] -= 0.5                                                 # the sampler does not need mu >= 0
    eps = rs.randn(b, v).astype(np.float32)
    mu = logit[:, :v].copy()
    # tau = 0 and eps = None: mu's bits, with NaNs planted in sigma and eps
    poisoned, eps_nan = logit.copy(), eps.copy()
    poisoned[:, v:][::2] = np.nan
    eps_nan[b // 2] = np.nan
    for args in ((_dev(eps_nan), 0.0), (_dev(eps_nan), -0.0), (None, 1.0), (None, 0.0)):
        assert _same_bits(ops.latent_sample(_dev(poisoned), *args).cpu().numpy(), mu), args
    # tau = 1: the training kernel's z
    lg, ep = _dev(logit), _dev(eps)
    zt, kl = torch.empty((b, v), device=DEV), torch.empty(1, device=DEV)
    assert lib.kpx_vae_sample_kl_fwd_f32(lg.data_ptr(), ep.data_ptr(), zt.data_ptr(), kl.data_ptr(), b, v, ops._stream()) == 0
    assert _same_bits(ops.latent_sample(lg, ep, 1.0).cpu().numpy(), zt.cpu().numpy())
    assert _same_bits(ops.latent_sample(lg, ep).cpu().numpy(), zt.cpu().numpy())
    for tau in (0.5, 2.0):
        got = ops.latent_sample(lg, ep, tau).cpu().numpy()
        assert M.within_one_ulp(got, P.sample_f64(logit, eps, tau)), (shape, tau)
    # a NaN in mu reaches only its own element
    bad = logit.copy()
    bad[b - 1, v // 2] = np.nan
    got = ops.latent_sample(_dev(bad), ep, 1.0).cpu().numpy()
    hit = np.zeros((b, v), bool)
    hit[b - 1, v // 2] = True
    assert np.array_equal(np.isnan(got), hit) and np.array_equal(got[~hit], zt.cpu().numpy()[~hit])


# ------------------------------------------------------------------------------------------------ kpx_latent_path_f32
def _path(za, zb, steps, mode):
    return _ops().latent_path(_dev(za), _dev(zb), steps, mode).cpu().numpy()


@pytest.mark.parametrize('steps', [2, 3, 64])
@pytest.mark.parametrize('shape', PATH_SHAPES, ids=ids(PATH_SHAPES))
def test_path_against_longdouble(shape, steps):
    """ends bit for bit; every other value within 1 fp32 ulp of longdouble plus 2^-48 (|a_i| + |b_i|), the cancellation of a component near
    zero under coefficients that carry fp64's rounding (the rows here are random: the angle is far from 0 and pi, asserted below)"""
    b, v = shape
    rs = np.random.RandomState(b * 31 + v + steps)
    za, zb = rs.randn(b, v).astype(np.float32), rs.randn(b, v).astype(np.float32)
    for mode in ('lerp', 'slerp'):
        got = _path(za, zb, steps, mode)
        want, fallback = P.path_longdouble(za, zb, steps, mode)
        assert got.shape == (steps, b, v) and got.dtype == np.float32
        assert _same_bits(got[0], za) and _same_bits(got[-1], zb), (shape, steps, mode)
        assert fallback.all() if (v == 1 and mode == 'slerp') else not fallback.any()
        if mode == 'slerp' and v > 1:
            cos = (za.astype(np.float64) * zb).sum(1) / np.sqrt((za.astype(np.float64) ** 2).sum(1) * (zb.astype(np.float64) ** 2).sum(1))
            assert (np.sqrt(1 - cos * cos) > 0.05).all()
        w64 = want.astype(np.float64)
        tol = P.ulp32(w64) + 2.0 ** -48 * (np.abs(za) + np.abs(zb)).astype(np.float64)[None]
        assert (np.abs(got.astype(np.float64) - w64) <= tol).all(), (shape, steps, mode)


def test_path_exact_cases_and_fallbacks():
    # S = 3 lerp on even integers is exact
    rs = np.random.RandomState(4)
    za, zb = (2 * rs.randint(-50, 50, (3, 5))).astype(np.float32), (2 * rs.randint(-50, 50, (3, 5))).astype(np.float32)
    assert np.array_equal(_path(za, zb, 3, 'lerp')[1], (za + zb) / 2)
    # e1 -> e2 on the great circle
    e1, e2 = np.array([[1, 0]], np.float32), np.array([[0, 1]], np.float32)
    mid = _path(e1, e2, 3, 'slerp')[1, 0]
    assert M.within_one_ulp(mid, np.array([np.sqrt(0.5), np.sqrt(0.5)]))
    assert M.within_one_ulp(_path(3 * e1, 3 * e2, 3, 'slerp')[1, 0], np.array([3 * np.sqrt(0.5)] * 2))
    # the fall-backs give lerp's bits: a = b, a = -b (through 0), a zero row, V = 1
    a = rs.randn(4, 7).astype(np.float32)
    b = rs.randn(4, 7).astype(np.float32)
    b[0], b[1], b[2] = a[0], -a[1], 0
    for steps in (3, 8):
        sl, le = _path(a, b, steps, 'slerp'), _path(a, b, steps, 'lerp')
        assert _same_bits(sl[:, :3], le[:, :3]) and not np.array_equal(sl[:, 3], le[:, 3])
        assert _same_bits(_path(b, a, steps, 'slerp')[:, 2], _path(b, a, steps, 'lerp')[:, 2])      # the zero row on the other side
    assert (_path(a, b, 3, 'slerp')[1, 1] == 0).all()                   # a = -b passes through 0
    one_a, one_b = np.array([[2.0], [-1.5], [0.5]], np.float32), np.array([[3.0], [4.0], [-0.5]], np.float32)
    assert _same_bits(_path(one_a, one_b, 5, 'slerp'), _path(one_a, one_b, 5, 'lerp'))


# ------------------------------------------------------------------------------------------------ FinalModel.encode
A = 9


def _encoder_arrays(k, cells, vae, seed):
    """vae_encoder/* from the oracle's registry, the biases randomised"""
    rs = np.random.RandomState(seed + 1)
    out = {n: a for n, a in R.init_motion_generator(k, A, cells, vae, (4, 4), seed=seed).items() if n.startswith('vae_encoder/')}
    for n in out:
        if n.endswith('/bias') or n.endswith('/biases'):
            out[n] = (rs.randn(*out[n].shape) * 0.05).astype(np.float32)
    return out


def _toy(seed=77, posterior=True):
    import kpx_amd
    import test_drive_gpu as T
    arrays = T._toy_arrays(seed)
    cfg = {'model': {'n_pts': T.K, 'cell_info': list(T.CELLS), 'vae_dim': T.VDIM, 'n_action': A}, 'paths': {'log_dir': '/tmp/kpx_final'}}
    fm = kpx_amd.FinalModel(cfg, device=DEV, image_size=T.RES, frames_per_launch=32, **({'posterior': True} if posterior else {}))
    fm.build()
    if posterior:
        arrays = dict(arrays, **_encoder_arrays(T.K, T.CELLS, T.VDIM, seed))
    fm.store.load_numpy(arrays, strict=True)
    return fm, arrays


def _motion(b, k, seed):
    rs = np.random.RandomState(seed)
    return ((rs.rand(b, k, 2) * 1.6 - 0.8).astype(np.float32), (rs.rand(b, 32, k, 2) * 1.6 - 0.8).astype(np.float32),
            np.eye(A, dtype=np.float32)[rs.randint(0, A, size=b)])


def _oracle_logit(arrays, kp, seq, ac, k, cells, vae, dtype):
    p = {n: torch.from_numpy(a).to(dtype) for n, a in arrays.items() if n.startswith('vae_encoder/')}
    b = kp.shape[0]
    mu, sd = R.vae_encoder(p, torch.from_numpy(seq).to(dtype).reshape(b, 32, 2 * k), torch.from_numpy(kp).to(dtype).reshape(b, 2 * k),
                           torch.from_numpy(ac).to(dtype), cells, vae)
    return torch.cat([mu, sd], 1).numpy()


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def _check_encode(fm, arrays, b, k, cells, vae, seed):
    kp, seq, ac = _motion(b, k, seed)
    state = torch.cuda.get_rng_state(DEV)
    got = [fm.encode(_dev(kp), _dev(seq), _dev(ac)).cpu().numpy().copy() for _ in range(3)]          # eager, capture + replay, replay
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    assert got[0].shape == (b, 2 * vae) and got[0].dtype == np.float32 and (got[0] >= 0).all()
    assert _same_bits(got[0], got[1]) and _same_bits(got[0], got[2])
    assert ('encode', b, 0) in fm._graphs and not fm._graph_failed
    w64, w32 = (_oracle_logit(arrays, kp, seq, ac, k, cells, vae, dt) for dt in (torch.float64, torch.float32))
    e_gpu, e_cpu = _rel_l2(got[0], w64), _rel_l2(w32, w64)
    print('encode B=%d K=%d cells=%s: rel-L2 vs float64 %.2e (CPU fp32 %.2e)' % (b, k, cells, e_gpu, e_cpu))
    assert e_gpu <= 4 * e_cpu + 2e-6
    assert np.array_equal(got[0] > 0, w64 > 0) or np.abs(w64[(got[0] > 0) != (w64 > 0)]).max() < 1e-5
    return got[0]


def test_encode_matches_the_oracle_in_float64_and_replays_bit_for_bit():
    import test_drive_gpu as T
    fm, arrays = _toy()
    _check_encode(fm, arrays, T.B, T.K, T.CELLS, T.VDIM, seed=3)
    _check_encode(fm, arrays, 5, T.K, T.CELLS, T.VDIM, seed=4)


def test_encode_at_the_reference_sizes():
    """configs/penn.yaml's cells and vae_dim at B = 2, K = 15 (30-wide rows)"""
    import kpx_amd
    k, cells, vae = 15, (1024, 1024), 64
    cfg = {'model': {'n_pts': k, 'cell_info': list(cells), 'vae_dim': vae, 'n_action': A}, 'paths': {'log_dir': '/tmp/kpx_final'}}
    fm = kpx_amd.FinalModel(cfg, device=DEV, image_size=32, posterior=True)
    fm.build()
    arrays = _encoder_arrays(k, cells, vae, seed=5)
    fm.store.load_numpy(arrays, strict=False)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    _check_encode(fm, arrays, 2, k, cells, vae, seed=6)


def test_encode_after_a_reload_and_the_rollout_beside_it():
    """a second checkpoint drops the encoder's graph and gives a fresh model's bits; run(z = mu) on a posterior=True model is the run of a
    posterior=False model bit for bit; posterior=False refuses encode by the argument's name"""
    import test_drive_gpu as T
    from kpx_amd._lib import KpxError
    ops = _ops()
    kp, seq, ac = (_dev(a) for a in _motion(T.B, T.K, 9))
    want = {seed: _toy(seed)[0].encode(kp, seq, ac).cpu().numpy().copy() for seed in (77, 177)}
    assert not np.array_equal(want[77], want[177])
    fm, _ = _toy(77)
    for _ in range(3):
        got = fm.encode(kp, seq, ac).cpu().numpy().copy()
    assert _same_bits(got, want[77]) and ('encode', T.B, 0) in fm._graphs
    fm.store.load_numpy(_toy(177)[1], strict=True)
    torch.empty(1 << 22, device=DEV).fill_(float('nan'))               # recycle freed blocks with poison: a stale graph would read it
    for call in range(3):
        assert _same_bits(fm.encode(kp, seq, ac).cpu().numpy().copy(), want[177]), call
    assert not fm._graph_failed
    # the rollout at z = mu, beside a model without the encoder
    feed, _, _ = T._toy_feed()
    mu = ops.latent_sample(fm.encode(kp, seq, ac), None, 0.0)
    assert _same_bits(mu.cpu().numpy(), want[177][:, :T.VDIM])
    plain, _ = _toy(177, posterior=False)
    assert not any(n.startswith('vae_encoder/') for n in plain.store.vars) and any(n.startswith('vae_encoder/') for n in fm.store.vars)
    state = torch.cuda.get_rng_state(DEV)
    for _ in range(3):
        a, b = T._snap(fm.run(None, feed, z=mu)), T._snap(plain.run(None, feed, z=mu))
        assert T._equal(a, b)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)
    with pytest.raises(KpxError, match='posterior=True'):
        plain.encode(kp, seq, ac)
    for bad in ((kp[:1], seq, ac), (kp, seq[:, :31], ac), (kp, seq, ac[:, :8]), (kp.double(), seq, ac), (kp, seq.cpu(), ac)):
        with pytest.raises(KpxError, match='FinalModel.encode'):
            fm.encode(*bad)


def test_a_checkpoint_without_the_encoder_is_refused_by_name(tmp_path):
    import test_drive_gpu as T
    from kpx_amd._lib import KpxError
    fm, arrays = _toy()
    full, bare = str(tmp_path / 'full.npz'), str(tmp_path / 'bare.npz')
    np.savez(full, **{n.replace('/', '|'): a for n, a in arrays.items()})
    np.savez(bare, **{n.replace('/', '|'): a for n, a in arrays.items() if not n.startswith('vae_encoder/')})
    fm.restore(None, full)
    with pytest.raises(KpxError, match='vae_encoder/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel is missing'):
        fm.restore(None, bare)
    _toy(posterior=False)[0].restore(None, bare)                       # without the argument the checkpoint is what it always was
    stage1 = str(tmp_path / 'stage1.npz')
    np.savez(stage1, **{n.replace('/', '|'): a for n, a in arrays.items() if not n.startswith('vae_')})
    fm.restore(None, stage1)                                           # a stage-1 checkpoint holds no motion generator: nothing to ask of it


# ------------------------------------------------------------------------------------------------ evaluate.py --posterior
def _png(path, mode=None):
    from PIL import Image
    im = Image.open(path)
    assert mode is None or im.mode == mode
    return np.asarray(im, np.uint8)


def _read_seq(d):
    assert sorted(os.listdir(d)) == ['%06d.png' % i for i in range(32)]
    return np.stack([_png(os.path.join(d, '%06d.png' % i), 'RGB') for i in range(32)])


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def test_evaluate_posterior_end_to_end_on_the_fixture_videos(tmp_path, monkeypatch, capsys):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    from kpx_amd import posterior
    from test_data_gpu import _fixture_dataset
    from test_drive_gpu import _check_metrics
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k, n_action, vae = int(golden['n_points']), int(golden['n_action']), 8
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': vae}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV, posterior=True)
    fm.build(None)
    rs = np.random.RandomState(2)                                      # biases off zero: the ReLU head leaves live and dead units
    fm.store.assign('vae_encoder/fully_connected/biases', rs.uniform(-0.2, 0.6, 2 * vae).astype(np.float32))
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt])

    states = []
    end_batch = evaluate._Posterior.end_batch

    def watched(self, *a, **kw):
        before = torch.cuda.get_rng_state(DEV)
        out = end_batch(self, *a, **kw)
        states.append(torch.equal(before, torch.cuda.get_rng_state(DEV)))
        return out

    monkeypatch.setattr(evaluate._Posterior, 'end_batch', watched)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics',
            '--motion-metrics', '--drive', 'labels,hold']
    for name, extra in (('post', ['--posterior', '--posterior-transfer']), ('plain', [])):
        torch.manual_seed(11)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    printed = capsys.readouterr().out
    assert 'posterior (own quantity, not comparable with published figures): 3 rows' in printed
    assert states == [True, True]                                      # a whole --posterior batch draws nothing
    ev, plain = tmp_path / 'post', tmp_path / 'plain'

    # ---- the run without the flags: every file it writes is there byte for byte, every array and key it scores bit for bit
    had, has = _files(str(plain)), _files(str(ev))
    for name, data_ in had.items():
        if name not in ('metrics.npz', 'metrics.json'):
            assert has[name] == data_, name
    npz0, npz = np.load(str(plain / 'metrics.npz')), np.load(str(ev / 'metrics.npz'))
    for key in npz0.files:
        assert _same_bits(npz0[key], npz[key]), key
    assert sorted(set(npz.files) - set(npz0.files)) == ['post_kp_l2', 'post_mse', 'post_psnr', 'post_ssim']
    js0, js = json.loads((plain / 'metrics.json').read_text()), json.loads((ev / 'metrics.json').read_text())
    assert set(js) - set(js0) == {'posterior'} and {key: js[key] for key in js0} == js0
    new = sorted(set(has) - set(had))
    samples = ['0000', '0001', '0002']
    want_new = ['posterior.npz'] + sorted('%s/%s' % (s, f) for s in samples for f in
                                          ['posterior.png'] + ['%s/%06d.png' % (d, i) for d in ('post_seq', 'post_points', 'post_transfer') for i in range(32)])
    assert new == sorted(want_new)

    # ---- posterior.npz, the block and the module
    store = np.load(str(ev / 'posterior.npz'))
    logit, classes = store['logit'], store['classes']
    assert logit.shape == (3, 2 * vae) and logit.dtype == np.float32 and classes.shape == (3,) and classes.dtype == np.int32
    assert store['state'].shape == (n_action, vae, 8) and store['counts'].shape == (n_action, 3) and store['kl_rows'].shape == (3,)
    assert (logit >= 0).all() and (logit > 0).any() and (logit == 0).any()
    loader = kpx_amd.data.SequenceDataLoader(str(data), 'test', n_points=k, n_action=n_action, random_order=False, randomness=False,
                                             with_image_seq=True)
    batches = [{key: b[key] for key in ('image', 'real_im_seq', 'real_seq', 'keypoints', 'action_code')}
               for b in loader.batches(2, DEV, repeat=False, num_preprocess_threads=2)]
    assert np.array_equal(classes, np.concatenate([b['action_code'].argmax(1).cpu().numpy() for b in batches]))
    state, counts, kl_rows = posterior.state_numpy(logit, classes, n_action)
    assert np.array_equal(counts, store['counts']) and counts[:, 0].sum() == 3
    for f in (0, 1, 2, 3, 5, 6, 7):
        assert _same_bits(state[:, :, f], store['state'][:, :, f]), f
    assert np.allclose(state[:, :, 4], store['state'][:, :, 4], rtol=1e-14, atol=0) and np.allclose(kl_rows, store['kl_rows'], rtol=1e-14, atol=0)
    block = js['posterior']
    want = json.loads(json.dumps(posterior.summarise_posterior(state, counts, 0.01), allow_nan=False))

    def close(a, b, path=''):
        if isinstance(b, dict):
            assert set(b) <= set(a), path
            for key in b:
                close(a[key], b[key], path + '/' + key)
        elif isinstance(b, list):
            assert len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                close(x, y, '%s[%d]' % (path, i))
        elif isinstance(b, float) and 'kl' in path and 'agg' not in path:
            assert abs(a - b) <= 1e-13 * abs(b), path                  # the kl fields: the device's log against numpy's
        else:
            assert a == b, path

    close(block, want)
    assert block['n'] == 3 and block['vae_dim'] == vae and block['counts'] == {'rows': 3, 'non_finite': 0, 'bad_group': 0}
    assert set(block['recon']) == {'ssim', 'psnr', 'mse', 'kp_l2'} and set(block['z_skill']) == {'ssim', 'psnr', 'mse'}
    capsys.readouterr()                                                # (the loader announced its subset)
    assert posterior.main([str(ev / 'posterior.npz')]) == 0
    again = json.loads(capsys.readouterr().out)
    assert again == {key: block[key] for key in again}                 # the module reproduces the block from the stored state
    recon = evaluate.summarise_recon({key[5:]: npz[key] for key in ('post_ssim', 'post_psnr', 'post_mse', 'post_kp_l2')},
                                     {key: npz[key] for key in ('ssim', 'psnr', 'mse')},
                                     {key: npz['drive_hold_' + key] for key in ('ssim', 'psnr', 'mse')})
    assert {key: block[key] for key in ('recon', 'z_skill')} == json.loads(json.dumps(recon, allow_nan=False))

    # ---- the rollouts: at z = mu of the stored rows, and of the next sample of the batch; the scores on the PNGs written
    model = kpx_amd.FinalModel(cfg, device=DEV, point_maps=True, posterior=True)
    model.build(None)
    model.restore(None, ckpt)
    res, cols, s = 128, 9, 0
    frames = [3, 7, 11, 15, 19, 23, 27, 31]
    scores, kp_l2 = [], []
    for batch in batches:
        bsz = batch['image'].shape[0]
        lg = model.encode(batch['keypoints'].contiguous(), batch['real_seq'].contiguous(), batch['action_code'].contiguous()).cpu().numpy()
        assert _same_bits(lg, logit[s:s + bsz])
        mu = _dev(logit[s:s + bsz, :vae])
        feed = {'image': batch['image'], 'action_code': batch['action_code']}
        rec = {key: v.cpu().numpy().copy() for key, v in model.run(None, feed, z=mu).items() if key in ('pred_im_seq', 'future_points', 'fut_pt_raw')}
        tr = model.run(None, feed, z=torch.roll(mu, -(1 % bsz), 0).contiguous())['pred_im_seq'].cpu().numpy().copy()
        image, real = batch['image'].cpu().numpy(), batch['real_im_seq'].cpu().numpy()
        driver = (np.arange(bsz) + 1 % bsz) % bsz
        for i in range(bsz):
            d = ev / samples[s + i]
            assert np.array_equal(_read_seq(str(d / 'post_seq')), metrics_ref.png8(rec['pred_im_seq'][i]))
            assert np.array_equal(_read_seq(str(d / 'post_points')), sheet_ref.raw8(rec['future_points'][i]))
            assert np.array_equal(_read_seq(str(d / 'post_transfer')), metrics_ref.png8(tr[i]))
            sheet = _png(str(d / 'posterior.png'), 'RGB')
            assert sheet.shape == (5 * res, cols * res, 3)
            cell = lambda row, col: sheet[row * res:(row + 1) * res, col * res:(col + 1) * res]
            for row, folder, src in ((0, 'real_seq', i), (1, 'post_seq', i), (2, 'pred_seq', i), (3, 'real_seq', driver[i]), (4, 'post_transfer', i)):
                own = ev / samples[s + (src if row == 3 else i)]
                assert np.array_equal(cell(row, 0), _png(str(own / 'input_im.png'))), (samples[s + i], row)
                for j, fr in enumerate(frames):
                    assert np.array_equal(cell(row, 1 + j), _png(str(own / folder / ('%06d.png' % fr)))), (samples[s + i], folder, fr)
        real8 = metrics_ref.png8(real).reshape(bsz * 32, res, res, 3) / 255.0
        post8 = np.stack([_read_seq(str(ev / samples[s + i] / 'post_seq')) for i in range(bsz)]).reshape(bsz * 32, res, res, 3) / 255.0
        scores.append(metrics_ref.frame_metrics(post8, real8))
        kp_l2.append(M.keypoint_draw_metrics(rec['fut_pt_raw'][None], batch['real_seq'].cpu().numpy())[0][0])
        s += bsz
    got = np.stack([npz['post_' + n] for n in ('ssim', 'mse', 'psnr')], axis=-1)
    assert got.shape == (3, 32, 3) and got.dtype == np.float32
    _check_metrics(got.reshape(-1, 3), np.concatenate(scores), 'post')
    assert npz['post_kp_l2'].shape == (3, 32) and M.within_one_ulp(npz['post_kp_l2'], np.concatenate(kp_l2))


# ------------------------------------------------------------------------------------------------ animate.py --interpolate / --motion-from
def test_animate_interpolate_and_motion_from(tmp_path):
    from PIL import Image
    import kpx_amd
    import animate
    from kpx_amd import stills
    from kpx_amd.data import _to_device_unit
    from test_animate_gpu import _picture, _tiny_config
    res, vae, n_action = 128, 8, 3
    cfg, cfg_path = _tiny_config(tmp_path, 5, n_action)
    fm = kpx_amd.FinalModel(cfg, device=DEV, posterior=True)
    fm.build(None)
    fm.store.assign('vae_encoder/fully_connected/biases', np.random.RandomState(2).uniform(-0.2, 0.6, 2 * vae).astype(np.float32))
    # to_coord is initialised at stddev 0.02, under which two draws of z move the key points by less than an 8-bit frame shows: widen it
    fm.store.assign('vae_decoder/fully_connected/W', np.random.RandomState(3).randn(32, 10).astype(np.float32))
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    pics = [str(tmp_path / 'a.png'), str(tmp_path / 'b.png')]
    Image.fromarray(_picture(140, 128, 4)).save(pics[0])
    Image.fromarray(_picture(128, 131, 5)).save(pics[1])
    video = tmp_path / 'video'
    video.mkdir()
    for i in range(33):
        Image.fromarray(_picture(64, 48, 100 + i)).save(str(video / ('%03d.png' % i)))
    out_dir, actions, seed, steps = str(tmp_path / 'out'), [0, 2], 7, 3
    animate.main(['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--images'] + pics +
                 ['--actions', '0,2', '--samples', '2', '--seed', str(seed), '--png', '--interpolate', str(steps), '--motion-from', str(video),
                  '--motion-class', '1', '--save_dir', out_dir])
    meta = json.loads(open(os.path.join(out_dir, 'animate.json')).read())
    assert meta['interpolate'] == {'steps': steps, 'mode': 'slerp', 'draws': [0, 1], 'grid': [steps, 2]}
    assert meta['motion_from']['class'] == 1 and meta['motion_from']['frames'] == list(range(33)) and meta['motion_from']['grid'] == [1, 2]
    assert set(meta['palette_sizes']) == {'classes', 'interp', 'latent'}
    # what the test computes itself: the path between the seeded draws, and mu of the 33 frames
    model = kpx_amd.FinalModel(cfg, device=DEV, point_maps=True, posterior=True)
    model.build(None)
    model.restore(None, ckpt)
    zs = np.random.RandomState(seed).randn(2, vae).astype(np.float32)
    path, fallback = P.path_longdouble(zs[:1], zs[1:], steps, 'slerp')
    assert not fallback.any()
    frames = _to_device_unit(np.stack([stills.fit(str(video / ('%03d.png' % i)))[0] for i in range(33)]), DEV)
    pts = model.detect(frames)
    code = _dev(np.eye(n_action, dtype=np.float32)[1:2])
    mu = _ops().latent_sample(model.encode(pts[:1].contiguous(), pts[1:].unsqueeze(0).contiguous(), code), None, 0.0)
    assert float(mu.abs().max()) > 0
    image = _to_device_unit(np.stack([stills.fit(p)[0] for p in pics]), DEV)
    mid = _ops().latent_path(_dev(zs[:1]), _dev(zs[1:]), steps, 'slerp')[1]
    assert (np.abs(mid.cpu().numpy().astype(np.float64) - path[1].astype(np.float64)) <= P.ulp32(path[1].astype(np.float64)) + 2.0 ** -48 * 8).all()
    for b in range(len(pics)):
        d = os.path.join(out_dir, '%04d' % b)
        assert {'interp.gif', 'interp.png', 'latent.gif', 'latent.png', 'classes.gif', 'classes.png'} <= set(os.listdir(d))
        interp, latent, classes = (_png(os.path.join(d, n), 'RGB') for n in ('interp.png', 'latent.png', 'classes.png'))
        assert interp.shape == (steps * res, 2 * res, 3) and latent.shape == (res, 2 * res, 3)
        cell = lambda im, r, c: im[r * res:(r + 1) * res, c * res:(c + 1) * res]
        for a, cls in enumerate(actions):
            # the first and last rows are draws 0 and 1: the last predicted frame, as classes.png (draw 0) and the PNG folders show it
            assert np.array_equal(cell(interp, 0, a), cell(classes, a, 8))
            for row, draw in ((0, 0), (steps - 1, 1)):
                assert np.array_equal(cell(interp, row, a), _png(os.path.join(d, 'draw_%02d' % draw, 'class_%02d' % cls, 'pred_seq', '000031.png'), 'RGB'))
            feed = {'image': image, 'action_code': _dev(np.repeat(np.eye(n_action, dtype=np.float32)[cls][None], len(pics), 0))}
            out = model.run(None, feed, z=mu.expand(len(pics), -1).contiguous())['pred_im_seq'][b, 31].cpu().numpy()
            assert np.array_equal(cell(latent, 0, a), metrics_ref.png8(out)), (b, cls)
            out = model.run(None, feed, z=mid.expand(len(pics), -1).contiguous())['pred_im_seq'][b, 31].cpu().numpy()
            assert np.array_equal(cell(interp, 1, a), metrics_ref.png8(out)), (b, cls)
        assert not np.array_equal(interp[:res], interp[(steps - 1) * res:])                     # the two draws differ, so the path has somewhere to go
