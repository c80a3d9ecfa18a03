"""GPU: the step guard (csrc/guard.hip, BaseModel._guard_*).  Restatements, sizes and planted inputs live in tests/guard_ref.py.

Kernels:  the health record against the restatement -- the non-finite count exact, the largest finite magnitude bit-equal, the sum of squares
          within (n-1) 2^-53 relative of the restatement in longdouble (the derived bound of a fixed-order float64 sum of exact non-negative
          terms), the 16-byte and the 4-byte load path bit-equal, a second call overwriting the first; the guarded Adam bit-equal to
          adam_tf_flat_dev_alpha_ on a clean record and leaving p, m, v alone on a dirty one, with the counters of the restatement; the
          restore copying on a dirty record only.
Models:   a guarded and an unguarded DetectorTranslatorModel stay bit-equal over clean steps in both launch forms; a step fed a non-finite
          NUMBER (one +Inf pixel, one NaN coordinate: ordinary values in ordinary tensors) leaves every parameter, slot and moving statistic
          of the guarded model bit-equal to before; the next clean step trains again.
"""
import numpy as np
import pytest
import torch

import guard_ref as G
import loss_optim_ref as L

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 0x7fa5c3e1                   # a NaN bit pattern no kernel here produces
PAD = 8


@pytest.fixture(scope='module')
def ops():
    from kpx_amd import ops
    return ops


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def placed(data, offset=0):
    """(buffer, fp32 view of ``data`` starting ``offset`` floats past a 16-byte boundary) with sentinels around the view."""
    data = np.ascontiguousarray(data, dtype=np.float32).ravel()
    lead = 4 + offset
    buf = torch.full((lead + data.size + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    view = buf[lead:lead + data.size].view(torch.float32)
    view.copy_(torch.from_numpy(data))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * offset
    return buf, view


def intact(buf, view):
    lead = (view.data_ptr() - buf.data_ptr()) // 4
    b = buf.cpu().numpy()
    return bool(np.all(b[:lead] == SENTINEL) and np.all(b[lead + view.numel():] == SENTINEL))


def dirty_health(ops, nonfinite):
    """A record with ``nonfinite`` planted through the health pass itself (one Inf per count) and zeroed counters."""
    h = ops.new_guard_health(DEV)
    g = np.ones(max(nonfinite, 1), np.float32)
    g[:nonfinite] = np.inf
    ops.grad_health(torch.from_numpy(g).to(DEV), h)
    assert ops.read_guard_health(h)['nonfinite'] == nonfinite
    return h


# ----------------------------------------------------------------------------------------------- health
_health_refs = {}


def health_ref(n, kind, value):
    """(count, float64 sum, longdouble sum, max) of one planted vector; computed once and shared by the cases that need it."""
    key = (n, kind, 'clean' if kind == 'nowhere' else repr(value))
    if key not in _health_refs:
        g = G.health_planted(n, kind, value)
        bad, s64, mx = G.health(g)
        _health_refs[key] = (bad, s64, G.health(g, np.longdouble)[1], mx)
    return _health_refs[key]


@pytest.mark.parametrize('n,kind', G.HEALTH_CASES)
def test_health_against_the_restatement_on_both_load_paths(ops, n, kind):
    work = ops.grad_health_workspace(n, DEV)
    worst = 0.0
    for value in (G.BAD_VALUES if kind != 'nowhere' else G.BAD_VALUES[:1]):
        g = G.health_planted(n, kind, value)
        bad, s64, sld, mx = health_ref(n, kind, value)
        records = []
        for offset in G.OFFSETS:
            buf, view = placed(g, offset)
            h = dirty_health(ops, 3)                             # a first call's result that this call must overwrite
            before = ops.read_guard_health(h)
            ops.grad_health(view, h, work)
            got = ops.read_guard_health(h)
            assert intact(buf, view) and np.array_equal(bits(view.cpu().numpy()), bits(g))
            assert got['nonfinite'] == bad == len(G.plant_positions(n, kind))
            assert np.float32(got['maxabs']).view(np.uint32) == np.float32(mx).view(np.uint32)
            err = abs(np.longdouble(got['sumsq']) - sld)
            print('health n=%d %s %s offset=%d: sumsq %.17g restatement %.17g error/bound %.3g'
                  % (n, kind, value, offset, got['sumsq'], s64, float(err) / max(G.sumsq_bound(n, sld), 1e-300)))
            assert err <= G.sumsq_bound(n, sld)
            worst = max(worst, float(err) / max(G.sumsq_bound(n, sld), 1e-300))
            assert all(got[k] == before[k] for k in ('skipped_total', 'skipped_run', 'updates'))      # the pass writes nothing else
            records.append(h.cpu().numpy().tobytes())
        assert records[0] == records[1], 'the 16-byte and the 4-byte load path disagree'
    print('ratio kpx_grad_health_f32 n=%d %s %.4f' % (n, kind, worst))


def test_health_record_is_the_same_bits_from_run_to_run(ops):
    n = G.SIZES[-1]
    view = torch.from_numpy(G.health_clean(n, seed=3)).to(DEV)
    a, b = ops.new_guard_health(DEV), ops.new_guard_health(DEV)
    ops.grad_health(view, a)
    ops.grad_health(view, b)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_guard_ops_refuse_wrong_dtypes_and_sizes(ops):
    from kpx_amd._lib import KpxError
    f = torch.zeros(8, device=DEV)
    h = ops.new_guard_health(DEV)
    a = torch.zeros(1, device=DEV)
    for call in (lambda: ops.grad_health(f.double(), h), lambda: ops.grad_health(f, torch.zeros(4, dtype=torch.int32, device=DEV)),
                 lambda: ops.grad_health(f[:0], h), lambda: ops.grad_health(f, h, work=torch.zeros(1, device=DEV)),
                 lambda: ops.grad_health(f, h.cpu()), lambda: ops.adam_tf_flat_guarded_(f, f[:4], f, f, a, 0.5, 0.999, 1e-8, h),
                 lambda: ops.adam_tf_flat_guarded_(f, f, f, f, torch.zeros(2, device=DEV), 0.5, 0.999, 1e-8, h),
                 lambda: ops.adam_tf_flat_guarded_(f, f, f.half(), f, a, 0.5, 0.999, 1e-8, h),
                 lambda: ops.guard_restore_(f, f[:4], h), lambda: ops.guard_restore_(f, f.cpu(), h)):
        with pytest.raises(KpxError):
            call()


# ----------------------------------------------------------------------------------------------- guarded Adam
def _state(n):
    p, m, v = L.adam_state(n)
    return [torch.from_numpy(x).to(DEV) for x in (p, m, v)]


@pytest.mark.parametrize('n', (1, 5, 1003, L.ADAM_GRID_ELEMS + 1027))
def test_guarded_adam_on_a_clean_record_is_the_dev_alpha_update_bit_for_bit(ops, n):
    gs = 1.0 / 3.0
    guarded, plain = _state(n), _state(n)
    h = ops.new_guard_health(DEV)
    for step in (1, 2, 3):
        g = torch.from_numpy(L.adam_grad(n, step)).to(DEV)
        a_dev = torch.tensor([L.adam_alpha(step)], dtype=torch.float32, device=DEV)
        ops.grad_health(g, h)
        ops.adam_tf_flat_guarded_(guarded[0], g, guarded[1], guarded[2], a_dev, L.BETA1, L.BETA2, L.ADAM_EPS, h, gscale=gs)
        ops.adam_tf_flat_dev_alpha_(plain[0], g, plain[1], plain[2], a_dev, L.BETA1, L.BETA2, L.ADAM_EPS, gs)
        for name, a, b in zip('pmv', guarded, plain):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), (name, step)
        rec = ops.read_guard_health(h)
        assert (rec['updates'], rec['skipped_total'], rec['skipped_run'], rec['nonfinite']) == (step, 0, 0, 0)


@pytest.mark.parametrize('n', (1, 5, 1003, L.ADAM_GRID_ELEMS + 1027))
def test_guarded_adam_over_clean_dirty_dirty_clean(ops, n):
    p, m, v = L.adam_state(n)
    pairs = [placed(x) for x in (p, m, v)]
    P, M, V = (view for _, view in pairs)
    h = ops.new_guard_health(DEV)
    counters = G.new_counters()
    a_dev = torch.tensor([L.adam_alpha(1)], dtype=torch.float32, device=DEV)
    for step, poison in enumerate((None, np.nan, -np.inf, None), 1):
        g = L.adam_grad(n, step)
        if poison is not None:
            g[n // 2] = poison
        gd = torch.from_numpy(g).to(DEV)
        before = [bits(t.cpu().numpy()).copy() for t in (P, M, V)]
        ops.grad_health(gd, h)
        ops.adam_tf_flat_guarded_(P, gd, M, V, a_dev, L.BETA1, L.BETA2, L.ADAM_EPS, h)
        after = [bits(t.cpu().numpy()) for t in (P, M, V)]
        _, counters = G.guarded_adam(p, g, m, v, L.adam_alpha(1), int(poison is not None), counters)
        rec = ops.read_guard_health(h)
        assert {k: rec[k] for k in counters} == counters and rec['nonfinite'] == int(poison is not None), (step, rec)
        if poison is not None:
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), 'a skipped update wrote p, m or v (step %d)' % step
        else:
            assert all(not np.array_equal(a, b) for a, b in zip(before, after)) and all(np.isfinite(t.cpu().numpy()).all() for t in (P, M, V))
        assert all(intact(buf, view) for buf, view in pairs) and np.array_equal(bits(gd.cpu().numpy()), bits(g))


# ----------------------------------------------------------------------------------------------- restore
@pytest.mark.parametrize('n', G.RESTORE_SIZES)
@pytest.mark.parametrize('dst_off,src_off', ((0, 0), (1, 1), (0, 1), (1, 0)))
def test_restore_copies_on_a_dirty_record_only(ops, n, dst_off, src_off):
    rs = np.random.RandomState(n)
    src = rs.randn(n).astype(np.float32)
    dst = rs.randn(n).astype(np.float32)
    src[0], dst[-1] = np.float32(np.nan), np.float32(-0.0)        # bit for bit: a NaN payload and a signed zero survive
    for nonfinite in (0, 2):
        (sbuf, S), (dbuf, D) = placed(src, src_off), placed(dst, dst_off)
        h = dirty_health(ops, nonfinite)
        ops.guard_restore_(D, S, h)
        assert np.array_equal(bits(D.cpu().numpy()), bits(G.restore(dst, src, nonfinite)))
        assert np.array_equal(bits(S.cpu().numpy()), bits(src)) and intact(sbuf, S) and intact(dbuf, D)
        assert ops.read_guard_health(h)['nonfinite'] == nonfinite


# ----------------------------------------------------------------------------------------------- the models
def raw(a):
    """The bytes of an array (0-d included)."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _snapshot(model):
    """Every parameter, slot and moving statistic as bits (the counters are checked apart)."""
    return {k: raw(v).copy() for k, v in model.checkpoint_arrays().items()
            if k not in ('global_step', 'beta1_power', 'beta2_power', 'beta1_power_1', 'beta2_power_1')}


def _same(a, b):
    assert set(a) == set(b)
    return [k for k in a if not np.array_equal(a[k], b[k])]


def _dt_model(guard):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
           'model': {'n_pts': 3}, 'paths': {'log_dir': '/tmp/kpx_test', 'vggnet': None}}
    vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(seed=19, width_div=8), device=DEV)        # make_model(32, 3, 2)'s size
    m = kpx_amd.DetectorTranslatorModel(cfg, device=DEV, vgg=vgg, image_size=32, **({'guard': True} if guard else {}))
    m.build()
    return m


def _pair(step, poison=False):
    from oracle import restatement as R
    im, fut = R.synthetic_pair(2, res=32, seed0=50 + step, seed1=60 + step)
    if poison:
        im = im.copy()
        im[1, 7, 11, 2] = np.inf                                 # one pixel; a number like any other
    return {'image': torch.from_numpy(im).to(DEV), 'future_image': torch.from_numpy(fut).to(DEV)}


@pytest.mark.parametrize('graph', (True, False), ids=('graph', 'eager'))
def test_detector_translator_guarded_steps(monkeypatch, graph):
    import kpx_amd.detector_translator_model as dtm
    monkeypatch.setattr(dtm, 'GRAPH', graph)
    guarded, plain = _dt_model(True), _dt_model(False)
    assert guarded.store.moving and set(guarded.store.moving) <= {'D', 'G'} and not plain.store.moving
    assert all(v.data_ptr() % 16 == 0 for n, v in guarded.store.vars.items() if 'moving' in n)
    for step in range(4):                                        # clean steps: the guarded model is the plain model, bit for bit
        for m in (guarded, plain):
            m.train_step(None, _pair(step), step, 2)
    assert (len(guarded._graphs) == 1) == graph and not guarded._graph_failed
    a, b = guarded.checkpoint_arrays(), plain.checkpoint_arrays()
    assert set(a) == set(b) and not [k for k in a if not np.array_equal(raw(a[k]), raw(b[k]))]
    rep = guarded.guard_report()
    assert set(rep) == {'D', 'G'}
    for r in rep.values():
        assert (r['updates'], r['skipped_total'], r['skipped_run'], r['nonfinite']) == (4, 0, 0, 0) and 0 < r['max_abs'] <= r['grad_norm'] < np.inf
    # one step with a +Inf pixel: both buckets skip, nothing but the host's counters moves
    before, powers, gstep = _snapshot(guarded), {w: list(v) for w, v in guarded.beta_power.items()}, guarded.global_step
    guarded.train_step(None, _pair(4, poison=True), 4, 2)
    assert _same(before, _snapshot(guarded)) == []
    assert guarded.global_step == gstep + 1 and all(guarded.beta_power[w][0] == np.float32(powers[w][0] * np.float32(0.5)) for w in 'DG')
    rep = guarded.guard_report()
    for r in rep.values():
        assert (r['updates'], r['skipped_total'], r['skipped_run']) == (5, 1, 1) and r['nonfinite'] > 0
    # one clean step: finite, changed, and the run of skips is over
    guarded.train_step(None, _pair(5), 5, 2)
    after = _snapshot(guarded)
    changed = _same(before, after)
    assert all(np.isfinite(v.view(np.float32)).all() for v in after.values())
    assert any('moving_mean' in k for k in changed) and any(k.endswith('/Adam') for k in changed) and any(k.endswith('kernel') for k in changed)
    for r in guarded.guard_report().values():
        assert (r['updates'], r['skipped_total'], r['skipped_run'], r['nonfinite']) == (6, 1, 0, 0)
    assert np.isfinite(list(guarded.loss_values().values())).all()


def _seq_feed(k, a, b, seed, poison=False):
    rs = np.random.RandomState(seed)
    d = {'keypoints': rs.rand(b, k, 2) * 1.6 - 0.8, 'real_seq': rs.rand(b, 32, k, 2) * 1.6 - 0.8, 'action_code': np.eye(a)[rs.randint(0, a, size=b)],
         'eps_D': rs.randn(b, 8), 'eps_G': rs.randn(b, 8)}
    if poison:
        d['real_seq'][1, 17, 2, 0] = np.nan
    return {n: torch.from_numpy(v.astype(np.float32)).to(DEV) for n, v in d.items()}


def _toy_model(kind, guard):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
           'model': {'n_pts': 5, 'n_action': 4, 'cell_info': [32, 32], 'vae_dim': 8, 'classifier_cells': [32, 16]}, 'paths': {'log_dir': '/tmp/kpx_test'}}
    kw = {'guard': True} if guard else {}
    m = (kpx_amd.MotionGeneratorModel(cfg, device=DEV, discr_cells=(32, 32), **kw) if kind == 'motion_generator'
         else kpx_amd.ActionClassifierModel(cfg, device=DEV, **kw))
    m.build()
    return m


@pytest.mark.parametrize('kind', ('motion_generator', 'action_classifier'))
def test_sequence_models_skip_a_step_with_a_nan_coordinate(kind):
    guarded, plain = _toy_model(kind, True), _toy_model(kind, False)
    buckets = {'motion_generator': {'D', 'G'}, 'action_classifier': {'G'}}[kind]
    for step in range(2):
        for m in (guarded, plain):
            m.train_step(None, _seq_feed(5, 4, 2, step), step, 2)
    a, b = guarded.checkpoint_arrays(), plain.checkpoint_arrays()
    assert set(a) == set(b) and not [k for k in a if not np.array_equal(raw(a[k]), raw(b[k]))]
    before, gstep = _snapshot(guarded), guarded.global_step
    guarded.train_step(None, _seq_feed(5, 4, 2, 2, poison=True), 2, 2)
    assert _same(before, _snapshot(guarded)) == [] and guarded.global_step == gstep + 1
    rep = guarded.guard_report()
    assert set(rep) == buckets
    for r in rep.values():
        assert (r['updates'], r['skipped_total'], r['skipped_run']) == (3, 1, 1) and r['nonfinite'] > 0
    guarded.train_step(None, _seq_feed(5, 4, 2, 3), 3, 2)
    after = _snapshot(guarded)
    assert all(np.isfinite(v.view(np.float32)).all() for v in after.values()) and _same(before, after)
    for r in guarded.guard_report().values():
        assert (r['updates'], r['skipped_total'], r['skipped_run'], r['nonfinite']) == (4, 1, 0, 0)


def test_detector_translator_guard_in_the_data_parallel_segments():
    """The segment form of the step (_train_step_dp: four captured segments around the two exchanges) has its own Adam calls.  Driven here at
    one rank without a process group -- the exchanges are then no-ops --: three clean steps (eager segments, then captured ones) end in the
    bits of the plain model's ordinary steps, and a poisoned step through the captured segments is skipped."""
    guarded, plain = _dt_model(True), _dt_model(False)
    for step in range(3):
        guarded._train_step_dp(_pair(step))
        plain.train_step(None, _pair(step), step, 2)
    assert any(k[0] == 'dp' for k in guarded._graphs) and not guarded._graph_failed
    a, b = guarded.checkpoint_arrays(), plain.checkpoint_arrays()
    assert set(a) == set(b) and not [k for k in a if not np.array_equal(raw(a[k]), raw(b[k]))]
    before = _snapshot(guarded)
    guarded._train_step_dp(_pair(3, poison=True))
    assert _same(before, _snapshot(guarded)) == [] and guarded.global_step == 4
    for r in guarded.guard_report().values():
        assert (r['updates'], r['skipped_total'], r['skipped_run']) == (4, 1, 1) and r['nonfinite'] > 0
    guarded._train_step_dp(_pair(4))
    after = _snapshot(guarded)
    assert all(np.isfinite(v.view(np.float32)).all() for v in after.values()) and _same(before, after)
    assert all(r['skipped_run'] == 0 for r in guarded.guard_report().values())
