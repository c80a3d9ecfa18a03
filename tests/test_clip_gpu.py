"""GPU: gradient norms on the device -- the clipped Adam update (csrc/guard.hip: kpx_adam_tf_flat_clipped_f32), the per-variable statistics
(csrc/grad_stats.hip) and clip_norm= / grad_stats= of the training models.  Restatements: tests/clip_ref.py, tests/grad_stats_ref.py.

Clipped Adam:  with N <= clip (N < clip, N == clip exactly, an all-zero gradient, clip = +Inf) bit-equal to adam_tf_flat_guarded_; a planted NaN
               skips bit for bit and leaves the clip record alone; with N > clip the reported scale within one fp32 ulp of the restatement's
               plus the relative slack guard_ref.sumsq_bound grants the sum, and p, m, v within loss_optim_ref.adam_bounds evaluated at the
               kernel's own gs = gscale * scale.
Statistics:    counts and maxima exact, sums within sumsq_bound of float64 in longdouble, the records bit-equal from run to run and across the
               table moved by 0..3 floats, NaN in the padding never counted, and the per-variable sums added up agree with kpx_grad_health_f32.
Models:        a bound far above the norm leaves the guarded model's bits; a bound below it gives the restatement's step at the reported scale,
               the same bits through the captured graph and eagerly.  In stage 1 the generator's gradient depends on the discriminator update
               of the same step, so a clipped run is held to the restatement on the gradient IT left in the bucket; the discriminator's is
               also held bit-equal to the unclipped run's.
"""
import numpy as np
import pytest
import torch

import clip_ref as C
import grad_stats_ref as S
import guard_ref as G
import loss_optim_ref as L
from test_guard_gpu import DEV, SENTINEL, bits, placed, intact, raw, _snapshot, _same, _pair, _seq_feed

pytestmark = pytest.mark.gpu
ADAM_SIZES = (1, 5, 1003, L.ADAM_GRID_ELEMS + 1027)
HYPER = (L.BETA1, L.BETA2, L.ADAM_EPS)


@pytest.fixture(scope='module')
def ops():
    from kpx_amd import ops
    return ops


def _state(n):
    return [torch.from_numpy(x).to(DEV) for x in L.adam_state(n)]


def _alpha(step=1):
    return torch.tensor([L.adam_alpha(step)], dtype=torch.float32, device=DEV)


def _both(ops, n, g, clip_norm, gscale=1.0):
    """One clipped and one guarded update from the same state on the gradient ``g`` -> (clipped p m v, guarded p m v, records)."""
    clipped, guarded = _state(n), _state(n)
    gd = torch.from_numpy(g).to(DEV)
    hc, hg, clip = ops.new_guard_health(DEV), ops.new_guard_health(DEV), ops.new_clip_state(DEV)
    ops.grad_health(gd, hc)
    ops.grad_health(gd, hg)
    ops.adam_tf_flat_clipped_(clipped[0], gd, clipped[1], clipped[2], _alpha(), *HYPER, hc, clip, clip_norm, gscale=gscale)
    ops.adam_tf_flat_guarded_(guarded[0], gd, guarded[1], guarded[2], _alpha(), *HYPER, hg, gscale=gscale)
    return clipped, guarded, ops.read_guard_health(hc), ops.read_guard_health(hg), ops.read_clip_state(clip)


# ----------------------------------------------------------------------------------------------- clipped Adam
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_clipped_adam_below_the_bound_is_the_guarded_update_bit_for_bit(ops, n):
    g = L.adam_grad(n, 1)
    exact = np.zeros(n, np.float32)                               # N == clip exactly: one element 3 (and 4 where there is room), N = 3 or 5
    exact[0] = 3.0
    if n > 1:
        exact[n - 1] = 4.0
    exact_norm = 3.0 if n == 1 else 5.0
    loose = float(np.sqrt(C.sumsq(g))) * 1.5
    for name, grad, clip_norm, gscale in (('N < clip', g, loose, 1.0), ('N < clip, gscale 1/3', g, loose, 1.0 / 3.0), ('N == clip', exact, exact_norm, 1.0),
                                          ('N == clip, gscale 0.5', exact, 0.5 * exact_norm, 0.5), ('zero', np.zeros(n, np.float32), 1e-30, 1.0),
                                          ('clip = inf', g * np.float32(1e6), np.inf, 1.0)):
        clipped, guarded, hc, hg, state = _both(ops, n, grad, clip_norm, gscale)
        for which, a, b in zip('pmv', clipped, guarded):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), (name, which)
        assert hc == hg and hc['updates'] == 1 and hc['skipped_total'] == 0, name
        want = C.clip_scale(C.sumsq(grad), clip_norm, gscale)[0]
        assert state['scale'] == 1.0 and state['clipped_total'] == 0 and state['norm'] == pytest.approx(float(want), rel=1e-6), (name, state)


@pytest.mark.parametrize('n', ADAM_SIZES)
def test_clipped_adam_skips_on_a_planted_nan_and_leaves_the_clip_record_alone(ops, n):
    g = L.adam_grad(n, 1) * np.float32(100.0)
    gd = torch.from_numpy(g).to(DEV)
    pairs = [placed(x) for x in L.adam_state(n)]
    P, M, V = (view for _, view in pairs)
    h, clip = ops.new_guard_health(DEV), ops.new_clip_state(DEV)
    clip_norm = float(np.sqrt(C.sumsq(g))) / 8
    ops.grad_health(gd, h)
    ops.adam_tf_flat_clipped_(P, gd, M, V, _alpha(), *HYPER, h, clip, clip_norm)                 # a clipped update first: the record holds values
    kept, before = clip.cpu().numpy().tobytes(), [bits(t.cpu().numpy()).copy() for t in (P, M, V)]
    assert ops.read_clip_state(clip)['clipped_total'] == 1
    g[n // 2] = np.nan
    gd = torch.from_numpy(g).to(DEV)
    ops.grad_health(gd, h)
    ops.adam_tf_flat_clipped_(P, gd, M, V, _alpha(), *HYPER, h, clip, clip_norm)
    assert all(np.array_equal(a, bits(t.cpu().numpy())) for a, t in zip(before, (P, M, V))), 'a skipped update wrote p, m or v'
    assert clip.cpu().numpy().tobytes() == kept, 'a skipped update wrote the clip record'
    rec = ops.read_guard_health(h)
    assert (rec['updates'], rec['skipped_total'], rec['skipped_run'], rec['nonfinite']) == (2, 1, 1, 1)
    assert all(intact(buf, view) for buf, view in pairs)


@pytest.mark.parametrize('gscale', (1.0, 0.5))
@pytest.mark.parametrize('n', ADAM_SIZES)
def test_clipped_adam_above_the_bound_against_the_restatement(ops, n, gscale):
    p, m, v = L.adam_state(n)
    pairs = [placed(x) for x in (p, m, v)]
    P, M, V = (view for _, view in pairs)
    h, clip = ops.new_guard_health(DEV), ops.new_clip_state(DEV)
    counters, state = G.new_counters(), C.new_state()
    alpha = L.adam_alpha(1)
    norm1 = gscale * float(np.sqrt(C.sumsq(L.adam_grad(n, 1))))
    clip_norm = float(np.float32(2.0 * norm1))                  # step 1 stays below it; steps 2 and 4 carry 8x the gradient and exceed it
    worst = 0.0
    for step, (factor, poison) in enumerate(((1.0, None), (8.0, None), (8.0, np.inf), (8.0, None)), 1):
        g = L.adam_grad(n, 1) * np.float32(factor)             # (one direction at two lengths: which steps clip does not hang on a draw)
        clean = g.copy()
        if poison is not None:
            g[n - 1] = poison
        gd = torch.from_numpy(g).to(DEV)
        ops.grad_health(gd, h)
        ops.adam_tf_flat_clipped_(P, gd, M, V, _alpha(), *HYPER, h, clip, clip_norm, gscale=gscale)
        got_state, rec = ops.read_clip_state(clip), ops.read_guard_health(h)
        (p64, m64, v64), counters, state = C.clipped_adam(p, clean, m, v, alpha, int(poison is not None), clip_norm, counters, state, gscale=gscale)
        assert {k: rec[k] for k in counters} == counters and got_state['clipped_total'] == state['clipped_total'], (step, rec, got_state)
        err = abs(got_state['scale'] - state['scale'])
        print('clipped adam n=%d gscale=%g step %d: scale %.9g restatement %.9g error/bound %.3g'
              % (n, gscale, step, got_state['scale'], state['scale'], err / C.scale_bound(n, state['scale'])))
        assert err <= C.scale_bound(n, state['scale'])
        assert got_state['norm'] == pytest.approx(state['norm'], rel=1e-6)
        got = [t.cpu().numpy() for t in (P, M, V)]
        if poison is None:
            assert (got_state['scale'] < 1.0) == (factor > 1.0)
            gs = gscale * got_state['scale']                    # the kernel's own operand (gscale is a power of two: the product is exact)
            ref = L.adam_step(p, g, m, v, alpha, gscale=gs)
            for which, a, r, b in zip('pmv', got, ref, L.adam_bounds(p, g, m, v, alpha, gscale=gs)):
                ratio = float(np.max(np.abs(a.astype(np.float64) - r) / b))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (which, step, ratio)
        else:
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, (p, m, v))), 'a skipped update wrote p, m or v'
        p, m, v = got
        assert all(intact(buf, view) for buf, view in pairs)
    assert state['clipped_total'] == 2 and counters == dict(skipped_total=1, skipped_run=0, updates=4)
    print('ratio kpx_adam_tf_flat_clipped_f32 n=%d gscale=%g %.4f' % (n, gscale, worst))


def test_clip_ops_refuse_wrong_dtypes_misaligned_pointers_and_bad_bounds(ops):
    from kpx_amd._lib import KpxError, lib
    f = torch.zeros(8, device=DEV)
    h, clip, a = ops.new_guard_health(DEV), ops.new_clip_state(DEV), torch.zeros(1, device=DEV)
    hyper = (0.5, 0.999, 1e-8)
    for call in (lambda: ops.adam_tf_flat_clipped_(f, f[:4], f, f, a, *hyper, h, clip, 1.0), lambda: ops.adam_tf_flat_clipped_(f, f, f.half(), f, a, *hyper, h, clip, 1.0),
                 lambda: ops.adam_tf_flat_clipped_(f, f, f, f, torch.zeros(2, device=DEV), *hyper, h, clip, 1.0),
                 lambda: ops.adam_tf_flat_clipped_(f, f, f, f, a, *hyper, torch.zeros(4, dtype=torch.int32, device=DEV), clip, 1.0),
                 lambda: ops.adam_tf_flat_clipped_(f, f, f, f, a, *hyper, h, torch.zeros(4, dtype=torch.int64, device=DEV), 1.0),
                 lambda: ops.adam_tf_flat_clipped_(f, f, f, f, a, *hyper, h, clip.cpu(), 1.0), lambda: ops.adam_tf_flat_clipped_(f, f, f, f, a, *hyper, h, clip, 0.0),
                 lambda: ops.adam_tf_flat_clipped_(f, f, f, f, a, *hyper, h, clip, -1.0), lambda: ops.adam_tf_flat_clipped_(f, f, f, f, a, *hyper, h, clip, float('nan')),
                 lambda: ops.adam_tf_flat_clipped_(f[1:5], f[1:5], f[1:5], f[1:5], a, *hyper, h, clip, 1.0)):      # 4-byte aligned views: the entry refuses
        with pytest.raises(KpxError):
            call()
    assert lib.kpx_adam_tf_flat_clipped_f32(f.data_ptr(), f.data_ptr() + 4, f.data_ptr(), f.data_ptr(), 4, a.data_ptr(), 0.5, 0.999, 1e-8, 1.0, 1.0,
                                            h.data_ptr(), clip.data_ptr(), None) == -1
    assert not f.any() and ops.read_guard_health(h)['updates'] == 0
    table = ops.grad_segment_table(S.FlatBucket((8,)), DEV)
    work, out = ops.grad_segment_workspace(table, DEV)
    for call in (lambda: ops.grad_segment_stats(f.double(), None, table), lambda: ops.grad_segment_stats(f, f[:4], table), lambda: ops.grad_segment_stats(f[:4], None, table),
                 lambda: ops.grad_segment_stats(f, None, ops.grad_segment_table(S.FlatBucket((8,)), 'cpu')), lambda: ops.grad_segment_stats(f, None, None),
                 lambda: ops.grad_segment_stats(f, None, table, work=torch.zeros(1, device=DEV)), lambda: ops.grad_segment_stats(f, None, table, out=out.int()),
                 lambda: ops.grad_segment_stats(f, None, table, out=torch.zeros((2, 4), dtype=torch.int64, device=DEV))):
        with pytest.raises(KpxError):
            call()


# ----------------------------------------------------------------------------------------------- per-variable statistics
_seg = {}


def seg_case(kind):
    """The per-variable vectors of one case and their float64 / longdouble statistics at shift 0; computed once and shared."""
    if kind not in _seg:
        b = S.synthetic_bucket(0)
        g, p = S.values(b, 1), S.values(b, 2)
        if kind != 'clean':
            g = S.planted(g, range(len(S.SEG_LENGTHS) + 2), {'nan': np.nan, 'inf': np.inf, 'ninf': -np.inf}[kind])      # every length, two of the ones
        f64, fld = (S.segment_stats(b, S.flat(b, g), S.flat(b, p), dtype=t) for t in (np.float64, np.longdouble))
        _seg[kind] = (g, p, f64, fld)
    return _seg[kind]


def _run_stats(ops, shift, g, p, with_p=True, gap=np.nan):
    b = S.synthetic_bucket(shift)
    gbuf, gview = placed(S.flat(b, g, gap=gap))
    pbuf, pview = placed(S.flat(b, p, gap=gap))
    assert gview.data_ptr() % 16 == 0 and all((off % 4 == 0) == (shift == 0) for off, _ in list(b.entries.values())[:8])
    table = ops.grad_segment_table(b, DEV)
    out = ops.grad_segment_stats(gview, pview if with_p else None, table)
    assert intact(gbuf, gview) and intact(pbuf, pview)
    return out.cpu().numpy().tobytes(), ops.read_segment_stats(out), gview


@pytest.mark.parametrize('kind', ('clean', 'nan', 'inf', 'ninf'))
def test_segment_stats_against_the_restatement_at_every_shift(ops, kind):
    g, p, f64, fld = seg_case(kind)
    numel = f64['numel']
    assert (kind == 'clean') == (f64['nonfinite_g'].sum() == 0)
    if kind != 'clean':
        assert f64['nonfinite_g'][:10].tolist() == [1, 2, 2, 2, 2, 2, 3, 6, 1, 1] and not f64['nonfinite_g'][10:].any()
    records, worst = [], 0.0
    for shift in S.SHIFTS:
        record, got, _ = _run_stats(ops, shift, g, p)               # the padding, the shift and the tail hold NaN: none may be counted
        assert np.array_equal(got['nonfinite_g'], f64['nonfinite_g']), 'shift %d' % shift
        assert np.array_equal(bits(got['maxabs_g']), bits(f64['maxabs_g'])), 'shift %d' % shift
        for key in ('sumsq_g', 'sumsq_p'):
            err = np.abs(got[key].astype(np.longdouble) - fld[key])
            bound = np.array([G.sumsq_bound(int(n), float(r)) for n, r in zip(numel, fld[key])])
            assert np.all(err <= bound), (key, shift, np.flatnonzero(err > bound)[:5])
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        records.append(record)
    assert all(r == records[0] for r in records[1:]), 'the records differ between shifts'
    assert _run_stats(ops, 0, g, p)[0] == records[0], 'the records differ from run to run'
    print('ratio kpx_grad_segment_stats_f32 %s %.4f' % (kind, worst))


def test_segment_stats_without_parameters_and_against_the_health_pass(ops):
    g, p, f64, fld = seg_case('clean')
    record, got, _ = _run_stats(ops, 1, g, p, with_p=False)
    assert not got['sumsq_p'].any() and np.array_equal(got['sumsq_g'], _run_stats(ops, 0, g, p)[1]['sumsq_g'])
    # the same buffer with zeros in the gaps through the health pass: the two fixed-order sums agree within the bound of either
    _, got, gview = _run_stats(ops, 0, g, p, gap=0.0)
    h = ops.new_guard_health(DEV)
    ops.grad_health(gview, h)
    rec = ops.read_guard_health(h)
    total, ref = got['sumsq_g'].sum(dtype=np.float64), fld['sumsq_g'].sum(dtype=np.longdouble)
    bound = G.sumsq_bound(gview.numel(), ref)
    print('segment sums %.17g health %.17g difference/bound %.3g' % (total, rec['sumsq'], abs(total - rec['sumsq']) / bound))
    assert abs(total - rec['sumsq']) <= bound and abs(np.longdouble(rec['sumsq']) - ref) <= bound
    assert rec['nonfinite'] == 0 and np.float32(rec['maxabs']) == got['maxabs_g'].max()


# ----------------------------------------------------------------------------------------------- the models
def _dt_model(**kw):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
           'model': {'n_pts': 3}, 'paths': {'log_dir': '/tmp/kpx_test', 'vggnet': None}}
    vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(seed=19, width_div=8), device=DEV)
    m = kpx_amd.DetectorTranslatorModel(cfg, device=DEV, vgg=vgg, image_size=32, **kw)
    m.build()
    return m


_run_a = {}


def run_a():
    """Run A: the guarded model (with grad_stats) over three steps; after the first, the gradients, their norms and the per-variable report."""
    if not _run_a:
        m = _dt_model(guard=True, grad_stats=True)
        m.train_step(None, _pair(0), 0, 2)
        rep = m.guard_report()
        _run_a.update(norms={w: r['grad_norm'] for w, r in rep.items()}, sizes={w: m.store.buckets[w].size for w in 'DG'}, grads={w: m.store.buckets[w].grads.cpu().numpy().copy() for w in 'DG'},
                      stats=m.grad_stats())
        # a NaN planted into one variable's gradient (what grad_stats() reads is the bucket as the step left it)
        bucket = m.store.buckets['D']
        victim = list(bucket.entries)[len(bucket.entries) // 2]
        view = bucket.view(bucket.grads, victim).view(-1)
        kept = view[-1:].clone()
        view[-1] = float('nan')
        _run_a['victim'], _run_a['dirty'] = victim, m.grad_stats()
        view[-1:] = kept
        for step in (1, 2):
            m.train_step(None, _pair(step), step, 2)
        _run_a['after3'] = _snapshot(m)
    return _run_a


def test_grad_stats_names_the_variable_with_a_planted_nan_and_only_that_one():
    a = run_a()
    assert set(a['stats']) == {'D', 'G'}
    for which, per_var in a['stats'].items():
        assert all(r['nonfinite'] == 0 and 0 <= r['max_abs'] <= r['grad_norm'] * (1 + 1e-6) and r['param_norm'] >= 0 for r in per_var.values())
        total = np.sqrt(sum(r['grad_norm'] ** 2 for r in per_var.values()))
        # the per-variable norms add up to the guard's norm of the bucket: two fixed-order float64 sums of the same n squares
        assert total == pytest.approx(a['norms'][which], rel=a['sizes'][which] * 2.0 ** -52)
        assert any(r['param_norm'] > 0 for r in per_var.values())
    named = [(w, n) for w, per_var in a['dirty'].items() for n, r in per_var.items() if r['nonfinite']]
    assert named == [('D', a['victim'])] and a['dirty']['D'][a['victim']]['nonfinite'] == 1


@pytest.mark.parametrize('graph', (True, False), ids=('graph', 'eager'))
def test_detector_translator_with_a_loose_bound_is_the_guarded_model_bit_for_bit(monkeypatch, graph):
    import kpx_amd.detector_translator_model as dtm
    monkeypatch.setattr(dtm, 'GRAPH', graph)
    a = run_a()
    b = _dt_model(clip_norm=4 * max(a['norms'].values()))
    assert b.guard and set(b._clip_state) == {'D', 'G'}
    for step in range(3):
        b.train_step(None, _pair(step), step, 2)
    assert (len(b._graphs) == 1) == graph and not b._graph_failed
    assert _same(a['after3'], _snapshot(b)) == []
    for r in b.clip_report().values():
        assert r['scale'] == 1.0 and r['clipped_total'] == 0 and 0 < r['norm'] < 4 * max(a['norms'].values())


_run_c = {}


@pytest.mark.parametrize('graph', (True, False), ids=('graph', 'eager'))
def test_detector_translator_with_a_tight_bound_takes_the_restatements_step(monkeypatch, graph):
    import kpx_amd.detector_translator_model as dtm
    monkeypatch.setattr(dtm, 'GRAPH', graph)
    a = run_a()
    clip_norm = float(np.float32(min(a['norms'].values()) / 4))
    c = _dt_model(clip_norm=clip_norm)
    start = {w: c.store.buckets[w].params.cpu().numpy().copy() for w in 'DG'}
    c.train_step(None, _pair(0), 0, 2)
    report = c.clip_report()
    tightest = min(a['norms'], key=a['norms'].get)
    assert report[tightest]['scale'] == pytest.approx(0.25, rel=1e-6)
    for which in 'DG':
        bucket = c.store.buckets[which]
        g = bucket.grads.cpu().numpy()
        if which == 'D':                                        # D's gradient does not depend on any update of this step: it is run A's
            assert np.array_equal(bits(g), bits(a['grads']['D']))
        n = g.size
        _, scale, _ = C.clip_scale(C.sumsq(g), clip_norm)
        r = report[which]
        assert r['clipped_total'] == 1 and abs(r['scale'] - scale) <= C.scale_bound(n, scale), (which, r, scale)
        zeros = np.zeros(n, np.float32)
        alpha = L.adam_alpha(1)
        ref = L.adam_step(start[which], g, zeros, zeros, alpha, gscale=r['scale'])
        bounds = L.adam_bounds(start[which], g, zeros, zeros, alpha, gscale=r['scale'])
        for name, got, want, bound in zip('pmv', (bucket.params, bucket.m, bucket.v), ref, bounds):
            ratio = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want) / bound))
            print('ratio clipped step %s %s %.4f' % (which, name, ratio))
            assert ratio <= 1.0, (which, name, ratio)
    for step in (1, 2):                                          # two more steps: replays of the captured step in the graph form
        c.train_step(None, _pair(step), step, 2)
    assert (len(c._graphs) == 1) == graph and not c._graph_failed
    assert all(1 <= r['clipped_total'] <= 3 for r in c.clip_report().values())
    _run_c[graph] = _snapshot(c)
    if len(_run_c) == 2:
        assert _same(_run_c[True], _run_c[False]) == [], 'the captured and the eager clipped steps differ'


def test_detector_translator_clipping_in_the_data_parallel_segments():
    """The segment form of the step (_train_step_dp) has its own Adam calls.  Driven at one rank without a process group, as the guard's test
    of the segments is: three clipped steps through the segments (eager, then captured) end in the bits of three clipped ordinary steps."""
    clip_norm = float(np.float32(min(run_a()['norms'].values()) / 4))
    segments, plain = _dt_model(clip_norm=clip_norm), _dt_model(clip_norm=clip_norm)
    for step in range(3):
        segments._train_step_dp(_pair(step))
        plain.train_step(None, _pair(step), step, 2)
    assert any(k[0] == 'dp' for k in segments._graphs) and not segments._graph_failed
    assert _same(_snapshot(segments), _snapshot(plain)) == []
    assert segments.clip_report() == plain.clip_report() and all(r['clipped_total'] >= 1 for r in segments.clip_report().values())


@pytest.mark.parametrize('kind', ('motion_generator', 'action_classifier'))
def test_sequence_models_take_a_clipped_step(kind):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
           'model': {'n_pts': 5, 'n_action': 4, 'cell_info': [32, 32], 'vae_dim': 8, 'classifier_cells': [32, 16]}, 'paths': {'log_dir': '/tmp/kpx_test'}}
    make = (lambda **kw: kpx_amd.MotionGeneratorModel(cfg, device=DEV, discr_cells=(32, 32), **kw)) if kind == 'motion_generator' \
        else (lambda **kw: kpx_amd.ActionClassifierModel(cfg, device=DEV, **kw))
    clip_norm = 1e-4                                             # far below the norm of either model's first gradient (asserted through scale < 1)
    m = make(clip_norm=clip_norm, grad_stats=True)
    m.build()
    before = _snapshot(m)
    m.train_step(None, _seq_feed(5, 4, 2, 0), 0, 2)
    after = _snapshot(m)
    assert all(np.isfinite(v.view(np.float32)).all() for v in after.values()) and _same(before, after)
    report, guard, stats = m.clip_report(), m.guard_report(), m.grad_stats()
    assert set(report) == set(guard) == set(stats) == {'motion_generator': {'D', 'G'}, 'action_classifier': {'G'}}[kind]
    for which, r in report.items():
        assert r['clipped_total'] == 1 and guard[which]['skipped_total'] == 0 and r['norm'] == pytest.approx(guard[which]['grad_norm'], rel=1e-6)
        assert 0 < r['scale'] < 1 and r['scale'] == pytest.approx(clip_norm / guard[which]['grad_norm'], rel=1e-6)
        total = np.sqrt(sum(v['grad_norm'] ** 2 for v in stats[which].values()))
        assert total == pytest.approx(guard[which]['grad_norm'], rel=m.store.buckets[which].size * 2.0 ** -52) and set(stats[which]) == set(m.store.buckets[which].entries)
