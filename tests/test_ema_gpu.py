"""GPU: the averaged generator (csrc/ema.hip, BaseModel._ema_*, kpx_amd/ema.py).  Restatements, sizes and operands live in tests/ema_ref.py.

Kernels:  kpx_ema_flat_f32 against e + (p - e) * rate in float64, every element within 4 fp32 ulps of |e| + |p| (derivation in ema_ref);
          its bitwise properties (e == p, the health record, p and the surroundings untouched, run to run); kpx_swap_flat_f32 word for word.
Models:   the averages of all three training models equal the recurrence replayed with ops.ema_flat_ on the per-step parameters and
          ema.rate, bit for bit, in every launch form, and training is bit-equal to a model without them; a guarded skip is no step for
          the average; save / resume continues bit for bit in both containers; inference under the averages equals a plain restore of the
          exported file; ema_weights() swaps in place and back; train.py --ema --ema-test end to end.
"""
import os

import numpy as np
import pytest
import torch

import ema_ref as E

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 0x7fa5c3e1                   # a NaN bit pattern no kernel here produces
PAD = 8
COUNTERS = ('global_step', 'beta1_power', 'beta2_power', 'beta1_power_1', 'beta2_power_1')


@pytest.fixture(scope='module')
def ops():
    from kpx_amd import ops
    return ops


@pytest.fixture(scope='module')
def ema():
    from kpx_amd import ema
    return ema


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def dev_bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)


def placed(words):
    """(buffer, fp32 view holding the uint32 ``words`` on a 16-byte boundary) with sentinel words before and after the view."""
    words = np.ascontiguousarray(words).reshape(-1).view(np.uint32)
    buf = torch.full((4 + words.size + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    buf[4:4 + words.size].copy_(torch.from_numpy(words.view(np.int32)))
    view = buf[4:4 + words.size].view(torch.float32)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 0
    return buf, view


def intact(buf, view):
    b = buf.cpu().numpy()
    return bool(np.all(b[:4] == SENTINEL) and np.all(b[4 + view.numel():] == SENTINEL))


def dirty_health(ops, nonfinite):
    """A record with ``nonfinite`` planted through the health pass itself (tests/test_guard_gpu.py)."""
    h = ops.new_guard_health(DEV)
    g = np.ones(max(nonfinite, 1), np.float32)
    g[:nonfinite] = np.inf
    ops.grad_health(torch.from_numpy(g).to(DEV), h)
    assert ops.read_guard_health(h)['nonfinite'] == nonfinite
    return h


def rate_dev(r):
    return torch.tensor([float(np.float32(r))], dtype=torch.float32, device=DEV)


# ----------------------------------------------------------------------------------------------- the update kernel
@pytest.mark.parametrize('n', E.SIZES)
def test_ema_update_against_float64(ops, n):
    for r in E.RATES:
        e, p = E.operands(n, r)
        ref, bound = E.update(e, p, r), E.bound(e, p)
        with np.errstate(under='ignore'):
            for form in (E.update_f32_plain, E.update_f32_fma):       # the chosen operands keep both float32 forms inside the bound
                assert (np.abs(form(e, p, r).astype(np.float64) - ref) <= bound).all()
        (ebuf, ev), (pbuf, pv) = placed(e), placed(p)
        rd = rate_dev(r)
        ops.ema_flat_(ev, pv, rd)
        got = ev.cpu().numpy()
        err = np.abs(got.astype(np.float64) - ref)
        print('ratio kpx_ema_flat_f32 n=%d rate=%.9g: worst error/bound %.4f' % (n, float(r), float(np.max(err / bound))))
        assert np.isfinite(got).all() and (err <= bound).all(), (n, r, int(np.argmax(err / bound)))
        assert np.array_equal(dev_bits(pv), bits(p)) and intact(ebuf, ev) and intact(pbuf, pv)
        assert float(rd.cpu()[0]) == float(np.float32(r))
        same = np.arange(n) % 4 == 1
        assert np.array_equal(bits(got)[same], bits(e)[same])                        # e == p (no -0) leaves e's bits
        # a second run gives the same bits
        (ebuf2, ev2), _ = placed(e), None
        ops.ema_flat_(ev2, pv, rd)
        assert np.array_equal(dev_bits(ev2), bits(got))


@pytest.mark.parametrize('n', E.SIZES)
def test_ema_update_under_a_health_record(ops, n):
    r = E.RATES[2]
    e, p = E.operands(n, r, seed=1)
    rd = rate_dev(r)
    (_, plain), (pbuf, pv) = placed(e), placed(p)
    ops.ema_flat_(plain, pv, rd)
    assert not np.array_equal(dev_bits(plain), bits(e))
    clean = ops.new_guard_health(DEV)
    record = clean.cpu().numpy().tobytes()
    ebuf, ev = placed(e)
    ops.ema_flat_(ev, pv, rd, clean)
    assert np.array_equal(dev_bits(ev), dev_bits(plain)) and intact(ebuf, ev)        # a clean record: the bits of the launch without one
    assert clean.cpu().numpy().tobytes() == record                                   # the record is only read
    dirty = dirty_health(ops, 2)
    record = dirty.cpu().numpy().tobytes()
    ebuf, ev = placed(e)
    ops.ema_flat_(ev, pv, rd, dirty)
    assert np.array_equal(dev_bits(ev), bits(e)) and intact(ebuf, ev)                # a dirty one: nothing is written
    assert dirty.cpu().numpy().tobytes() == record
    assert np.array_equal(dev_bits(pv), bits(p)) and intact(pbuf, pv)


def test_ema_ops_refuse_wrong_dtypes_sizes_and_overlap(ops):
    from kpx_amd._lib import KpxError
    f, g = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    r, h = torch.zeros(1, device=DEV), ops.new_guard_health(DEV)
    for call in (lambda: ops.ema_flat_(f, g[:4], r), lambda: ops.ema_flat_(f.double(), g, r), lambda: ops.ema_flat_(f, g, torch.zeros(2, device=DEV)),
                 lambda: ops.ema_flat_(f, g, r.cpu()), lambda: ops.ema_flat_(f, g, r, torch.zeros(4, dtype=torch.int32, device=DEV)),
                 lambda: ops.ema_flat_(f[:0], g[:0], r), lambda: ops.ema_flat_(f[1:5], g[:4], r), lambda: ops.ema_flat_(f, g, r, h.cpu()),
                 lambda: ops.swap_flat_(f, f), lambda: ops.swap_flat_(f, g[:4]), lambda: ops.swap_flat_(f[:6], f[4:]),
                 lambda: ops.swap_flat_(f, g.cpu()), lambda: ops.swap_flat_(f[1:5], g[:4]), lambda: ops.swap_flat_(f.half(), g.half())):
        with pytest.raises(KpxError):
            call()


# ----------------------------------------------------------------------------------------------- the swap kernel
@pytest.mark.parametrize('n', E.SIZES)
def test_swap_exchanges_word_for_word(ops, n):
    a, b = E.swap_operands(n)
    (abuf, av), (bbuf, bv) = placed(a), placed(b)
    ops.swap_flat_(av, bv)
    assert np.array_equal(dev_bits(av), b) and np.array_equal(dev_bits(bv), a)       # NaN payloads, +-Inf and -0 included
    assert intact(abuf, av) and intact(bbuf, bv)
    ops.swap_flat_(av, bv)
    assert np.array_equal(dev_bits(av), a) and np.array_equal(dev_bits(bv), b)       # twice is the identity
    assert intact(abuf, av) and intact(bbuf, bv)


# ----------------------------------------------------------------------------------------------- the models
def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _snapshot(model):
    return {k: raw(v).copy() for k, v in model.checkpoint_arrays().items() if k not in COUNTERS}


def _differ(a, b):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    return [k for k in a if not np.array_equal(raw(a[k]), raw(b[k]))]


_vgg = []


def _dt_model(seed=1234, **kw):
    """tests/test_guard_gpu.py::_dt_model's size: image 32, K = 3, batch 2, the width/8 VGG."""
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
           'model': {'n_pts': 3}, 'paths': {'log_dir': '/tmp/kpx_test', 'vggnet': None}}
    if not _vgg:
        _vgg.append(kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(seed=19, width_div=8), device=DEV))
    m = kpx_amd.DetectorTranslatorModel(cfg, device=DEV, vgg=_vgg[0], image_size=32, seed=seed, **kw)
    m.build()
    return m


def _pair(step, poison=False):
    from oracle import restatement as R
    im, fut = R.synthetic_pair(2, res=32, seed0=50 + step, seed1=60 + step)
    if poison:
        im = im.copy()
        im[1, 7, 11, 2] = np.inf                                 # one pixel; a number like any other
    return {'image': torch.from_numpy(im).to(DEV), 'future_image': torch.from_numpy(fut).to(DEV)}


SEQ_CFG = {'n_pts': 5, 'n_action': 4, 'cell_info': [32, 32], 'vae_dim': 8, 'classifier_cells': [32, 16]}


def _seq_feed(seed, k=5, a=4, b=2):
    rs = np.random.RandomState(seed)
    d = {'keypoints': rs.rand(b, k, 2) * 1.6 - 0.8, 'real_seq': rs.rand(b, 32, k, 2) * 1.6 - 0.8, 'action_code': np.eye(a)[rs.randint(0, a, size=b)],
         'eps_D': rs.randn(b, 8), 'eps_G': rs.randn(b, 8)}                           # the noise of stage 2 is fed explicitly
    return {n: torch.from_numpy(v.astype(np.float32)).to(DEV) for n, v in d.items()}


def _seq_model(kind, seed=777, model_cfg=SEQ_CFG, **kw):
    """tests/test_guard_gpu.py::_toy_model's sizes."""
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2}, 'model': dict(model_cfg),
           'paths': {'log_dir': '/tmp/kpx_test'}}
    m = (kpx_amd.MotionGeneratorModel(cfg, device=DEV, discr_cells=(32, 32), seed=seed, **kw) if kind == 'motion_generator'
         else kpx_amd.ActionClassifierModel(cfg, device=DEV, seed=seed, **kw))
    m.build()
    return m


def _model(kind, **kw):
    return _dt_model(**kw) if kind == 'detector_translator' else _seq_model(kind, **kw)


def _feed(kind, step):
    return _pair(step) if kind == 'detector_translator' else _seq_feed(step)


class Replay:
    """The recurrence replayed beside a model: shadow += (p_t - shadow) * ema.rate(decay, t) with ops.ema_flat_ on the parameters the model
    holds after step t (what the launch behind that step's Adam update read)."""

    def __init__(self, ops, ema, model, decay, warmup=True):
        self.ops, self.ema, self.decay, self.warmup = ops, ema, decay, warmup
        self.bucket = model.store.buckets['G']
        self.shadow = self.bucket.params.detach().clone()
        self.rate = torch.zeros(1, dtype=torch.float32, device=DEV)

    def step(self, t):
        self.ops.fill_raw_(self.rate, float(self.ema.rate(self.decay, t, self.warmup)))
        self.ops.ema_flat_(self.shadow, self.bucket.params.detach(), self.rate)

    def matches(self):
        return np.array_equal(dev_bits(self.shadow), dev_bits(self.bucket.ema))


@pytest.mark.parametrize('graph', (True, False), ids=('graph', 'eager'))
def test_detector_translator_averages_equal_the_replayed_recurrence(monkeypatch, ops, ema, graph):
    import kpx_amd.detector_translator_model as dtm
    monkeypatch.setattr(dtm, 'GRAPH', graph)
    averaged, plain = _dt_model(ema=0.999), _dt_model()
    g, d = averaged.store.buckets['G'], averaged.store.buckets['D']
    assert d.ema is None and plain.store.buckets['G'].ema is None and g.ema.numel() == g.params.numel()
    replay = Replay(ops, ema, averaged, 0.999)
    assert replay.matches()                                              # the averages start as the parameters
    for step in range(4):
        averaged.train_step(None, _pair(step), step, 2)
        plain.train_step(None, _pair(step), step, 2)
        replay.step(step)
        assert replay.matches(), step
        assert averaged._ema_last_rate == float(ema.rate(0.999, step))
    assert (len(averaged._graphs) == 1) == graph and not averaged._graph_failed
    assert not np.array_equal(dev_bits(g.ema), dev_bits(g.params))
    a, b = averaged.checkpoint_arrays(), plain.checkpoint_arrays()
    shadows = sorted(k for k in a if k.endswith(ema.SUFFIX))
    assert shadows and not [k for k in shadows if 'discr' in k]
    assert sorted(k for k in a if k not in shadows) == sorted(b)
    assert [k for k in b if not np.array_equal(raw(a[k]), raw(b[k]))] == []         # the average does not disturb training
    assert sorted(shadows) == sorted(k + ema.SUFFIX for k in b if not k.endswith(('/Adam', '/Adam_1')) and k + '/Adam' in b and 'discr' not in k)


@pytest.mark.parametrize('graph', (True, False), ids=('graph', 'eager'))
def test_a_guarded_skip_is_no_step_for_the_average(monkeypatch, ema, graph):
    import kpx_amd.detector_translator_model as dtm
    monkeypatch.setattr(dtm, 'GRAPH', graph)
    model = _dt_model(ema=0.999, guard=True)
    for step in range(3):
        model.train_step(None, _pair(step), step, 2)
    assert (len(model._graphs) == 1) == graph
    before, gstep = _snapshot(model), model.global_step
    assert any(k.endswith(ema.SUFFIX) for k in before) and any('moving_mean' in k for k in before)
    model.train_step(None, _pair(3, poison=True), 3, 2)                  # one +Inf pixel: both buckets skip
    assert _differ(before, _snapshot(model)) == [] and model.global_step == gstep + 1
    assert all(r['skipped_total'] == 1 for r in model.guard_report().values())
    model.train_step(None, _pair(4), 4, 2)
    changed = _differ(before, _snapshot(model))
    assert any(k.endswith(ema.SUFFIX) for k in changed) and any(k.endswith('kernel') for k in changed)
    assert all(np.isfinite(v.view(np.float32)).all() for v in _snapshot(model).values())
    assert model._ema_last_rate == float(ema.rate(0.999, 4))             # the schedule's index advanced over the skipped step


def test_the_segment_form_ends_in_the_bits_of_the_ordinary_steps(ema):
    """_train_step_dp at one rank without a process group (tests/test_guard_gpu.py): eager segments, then the four captured ones."""
    segments, ordinary = _dt_model(ema=0.999), _dt_model(ema=0.999)
    for step in range(3):
        segments._train_step_dp(_pair(step))
        ordinary.train_step(None, _pair(step), step, 2)
    assert any(k[0] == 'dp' for k in segments._graphs) and not segments._graph_failed
    a, b = segments.checkpoint_arrays(), ordinary.checkpoint_arrays()
    assert any(k.endswith(ema.SUFFIX) for k in a) and _differ(a, b) == []


@pytest.mark.parametrize('kind', ('motion_generator', 'action_classifier'))
def test_sequence_model_averages_equal_the_replayed_recurrence(ops, ema, kind):
    averaged, plain = _seq_model(kind, ema=0.999), _seq_model(kind)
    replay = Replay(ops, ema, averaged, 0.999)
    for step in range(2):
        averaged.train_step(None, _seq_feed(step), step, 2)
        plain.train_step(None, _seq_feed(step), step, 2)
        replay.step(step)
        assert replay.matches(), step
    a, b = averaged.checkpoint_arrays(), plain.checkpoint_arrays()
    shadows = [k for k in a if k.endswith(ema.SUFFIX)]
    assert shadows and not [k for k in shadows if 'discr' in k]
    assert averaged.store.buckets['D'].ema is None
    if kind == 'motion_generator':
        assert any('discr' in k for k in a) and len(shadows) == len(averaged.store.buckets['G'].entries)
    assert [k for k in b if not np.array_equal(raw(a[k]), raw(b[k]))] == [] and sorted(k for k in a if k not in shadows) == sorted(b)
    assert any(not np.array_equal(raw(a[k]), raw(a[k[:-len(ema.SUFFIX)]])) for k in shadows)


def test_no_warmup_takes_the_constant_rate(ops, ema):
    model = _seq_model('action_classifier', ema=0.9, ema_warmup=False)
    replay = Replay(ops, ema, model, 0.9, warmup=False)
    for step in range(2):
        model.train_step(None, _seq_feed(step), step, 2)
        replay.step(step)
        assert model._ema_last_rate == float(np.float32(1) - np.float32(0.9))
    assert replay.matches()


# ----------------------------------------------------------------------------------------------- save and resume
def _save(model, root, fmt):
    model.log_dir = str(root)
    os.makedirs(os.path.join(str(root), model.name), exist_ok=True)
    return model.save_checkpoint(None, model.global_step - 1, fmt=fmt)


@pytest.mark.parametrize('fmt', ('npz', 'tf'))
@pytest.mark.parametrize('kind', ('detector_translator', 'motion_generator', 'action_classifier'))
def test_two_steps_save_resume_two_steps_equal_four_steps(tmp_path, ema, kind, fmt):
    whole = _model(kind, ema=0.999)
    for step in range(4):
        whole.train_step(None, _feed(kind, step), step, 2)
    first = _model(kind, ema=0.999)
    for step in range(2):
        first.train_step(None, _feed(kind, step), step, 2)
    path = _save(first, tmp_path, fmt)
    second = _model(kind, ema=0.999, seed=99)                            # other initial values: everything it ends with was restored
    assert second.resume(None, path)[0] == 2
    assert _differ(_snapshot(first), _snapshot(second)) == []
    for step in range(2, 4):
        second.train_step(None, _feed(kind, step), step, 2)
    a, b = whole.checkpoint_arrays(), second.checkpoint_arrays()
    assert any(k.endswith(ema.SUFFIX) for k in a) and _differ(a, b) == []
    assert int(b['global_step']) == 4


# ----------------------------------------------------------------------------------------------- inference under the averages
def _export(ema, path, out, fmt):
    assert ema.main([path, out, '--ckpt-format', fmt]) == 0
    return out


def test_keypoint_model_under_ema_equals_a_plain_restore_of_the_exported_file(tmp_path, ema):
    import kpx_amd
    trained = _dt_model(ema=0.9, ema_warmup=False)
    for step in range(2):
        trained.train_step(None, _pair(step), step, 2)
    path = _save(trained, tmp_path / 'train', 'npz')
    exported = _export(ema, path, str(tmp_path / 'averaged.npz'), 'npz')
    cfg = {'model': {'n_pts': 3}, 'paths': {'log_dir': str(tmp_path / 'kp')}}
    from oracle import restatement as R
    im, fut = R.synthetic_pair(2, res=32, seed0=8, seed1=9)
    feed = {'image': torch.from_numpy(np.stack([im, fut], axis=1)).to(DEV)}          # [B, T = 2, H, W, 3]
    out = {}
    for name, ckpt, kw in (('ema', path, {'ema': True}), ('exported', exported, {}), ('plain', path, {})):
        km = kpx_amd.KeypointModel(cfg, device=DEV, image_size=32)
        km.build(None)
        km.restore(None, ckpt, **kw)
        out[name] = km.run(None, feed)['pts'].cpu().numpy().copy()
    assert np.isfinite(out['ema']).all() and np.array_equal(bits(out['ema']), bits(out['exported']))
    assert not np.array_equal(bits(out['ema']), bits(out['plain']))
    km = kpx_amd.KeypointModel(cfg, device=DEV, image_size=32)
    km.build(None)
    with pytest.raises(Exception) as e:
        km.restore(None, exported, ema=True)                                         # no averages in it: refused, and named
    assert exported in str(e.value) and 'no averaged weights' in str(e.value)


def test_final_model_under_ema_equals_a_plain_restore_of_the_exported_files(tmp_path, ema):
    """The toy sizes of tests/test_drive_gpu.py (image 32, K = 3, vae_dim 8, nine classes), cells (32, 32)."""
    import kpx_amd
    from oracle import restatement as R
    stage1 = _dt_model(ema=0.9, ema_warmup=False)
    s2_cfg = {'n_pts': 3, 'n_action': 9, 'cell_info': [32, 32], 'vae_dim': 8}
    stage2 = _seq_model('motion_generator', model_cfg=s2_cfg, ema=0.9, ema_warmup=False)
    for step in range(2):
        stage1.train_step(None, _pair(step), step, 2)
        stage2.train_step(None, _seq_feed(step, k=3, a=9), step, 2)
    paths = [_save(stage1, tmp_path / 'train', 'tf'), _save(stage2, tmp_path / 'train', 'npz')]
    exported = [_export(ema, paths[0], str(tmp_path / 'out' / 'stage1'), 'tf'), _export(ema, paths[1], str(tmp_path / 'stage2.npz'), 'npz')]
    cfg = {'model': s2_cfg, 'paths': {'log_dir': str(tmp_path / 'final')}}
    im, _ = R.synthetic_pair(2, res=32, seed0=8, seed1=9)
    feed = {'image': torch.from_numpy(im).to(DEV), 'action_code': torch.from_numpy(np.eye(9, dtype=np.float32)[[2, 7]]).to(DEV)}
    z = torch.from_numpy(np.random.RandomState(6).randn(2, 8).astype(np.float32)).to(DEV)
    keys, out = ('pred_im_seq', 'fut_pt_raw', 'first_pt'), {}
    for name, ckpts, kw in (('ema', paths, {'ema': True}), ('exported', exported, {}), ('plain', paths, {})):
        fm = kpx_amd.FinalModel(cfg, device=DEV, image_size=32, frames_per_launch=32)
        fm.build()
        for p in ckpts:
            fm.restore(None, p, **kw)
        o = fm.run(None, feed, z=z)
        out[name] = {k: o[k].cpu().numpy().copy() for k in keys}
    for k in keys:
        assert np.isfinite(out['ema'][k]).all() and np.array_equal(bits(out['ema'][k]), bits(out['exported'][k])), k
    assert not np.array_equal(bits(out['ema']['pred_im_seq']), bits(out['plain']['pred_im_seq']))
    assert not np.array_equal(bits(out['ema']['fut_pt_raw']), bits(out['plain']['fut_pt_raw']))


# ----------------------------------------------------------------------------------------------- ema_weights()
def test_ema_weights_swaps_in_place_and_back(ema):
    model, twin = _dt_model(ema=0.9, ema_warmup=False), _dt_model(ema=0.9, ema_warmup=False)
    for step in range(2):
        model.train_step(None, _pair(step), step, 2)
        twin.train_step(None, _pair(step), step, 2)
    arrays = model.checkpoint_arrays()
    before = _snapshot(model)
    g = model.store.buckets['G']
    addresses = (g.params.data_ptr(), g.ema.data_ptr())
    fresh = _dt_model(seed=5)                                            # a model without averages, loaded through select
    fresh.store.load_numpy(ema.select(arrays), strict=False)
    want = fresh.test_step(None, _pair(9), 2, 1, 2)[:2]
    own = model.test_step(None, _pair(9), 2, 1, 2)[:2]
    with model.ema_weights() as inside:
        assert inside is model and (g.params.data_ptr(), g.ema.data_ptr()) == addresses
        now = model.checkpoint_arrays()
        for k in arrays:
            if k.endswith(ema.SUFFIX):
                name = k[:-len(ema.SUFFIX)]
                assert np.array_equal(raw(now[name]), raw(arrays[k])) and np.array_equal(raw(now[k]), raw(arrays[name])), k
        assert model.test_step(None, _pair(9), 2, 1, 2)[:2] == want
        with pytest.raises(RuntimeError):
            with model.ema_weights():
                pass
        with pytest.raises(RuntimeError):
            model.train_step(None, _pair(2), 2, 2)
    assert want != own
    assert _differ(before, _snapshot(model)) == [] and model.test_step(None, _pair(9), 2, 1, 2)[:2] == own
    with pytest.raises(ZeroDivisionError):
        with model.ema_weights():
            1 / 0
    assert _differ(before, _snapshot(model)) == [] and not model._ema_active
    for m in (model, twin):                                              # a following step equals that of a model that never entered
        m.train_step(None, _pair(2), 2, 2)
    assert _differ(model.checkpoint_arrays(), twin.checkpoint_arrays()) == []
    with pytest.raises(ValueError):
        with fresh.ema_weights():
            pass


# ----------------------------------------------------------------------------------------------- train.py
@pytest.mark.parametrize('mode', ('detector_translator', 'motion_generator', 'action_classifier'))
def test_train_main_with_ema_and_ema_test(tmp_path, ema, mode, caplog):
    import yaml
    import train
    from kpx_amd import summary
    from kpx_amd.base_model import BaseModel
    log_dir = tmp_path / 'log'
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(log_dir)},
           'training': {'n_steps': 3, 'test_interval': 1, 'checkpoint_interval': 1, 'log_interval': 1, 'summary_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': 5, 'n_action': 9, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    argv = ['--mode', mode, '--config', str(cfg_path), '--synthetic', '--ema', '0.99', '--ema-test'] + (
        ['--synthetic-vgg'] if mode == 'detector_translator' else [])
    torch.manual_seed(0)
    train.main(argv + ['--steps', '2'])
    d = log_dir / mode
    arrays = BaseModel.read_checkpoint(str(d / 'model.ckpt-1.npz'))
    shadows = [k for k in arrays if k.endswith(ema.SUFFIX)]
    assert shadows and not [k for k in shadows if 'discr' in k] and int(arrays['global_step']) == 2
    assert any(not np.array_equal(arrays[k], arrays[k[:-len(ema.SUFFIX)]]) for k in shadows)
    files = summary.event_files(str(d / 'test_ema'))
    assert len(files) == 1
    under = summary.scalars(str(d / 'test_ema'))
    plain = summary.scalars(str(d / 'test'))
    assert under and sorted(under) == sorted(plain) and all([s for s, _ in v] == [0, 1] for v in under.values())
    assert any(e['values'] for e in summary.read_events(files[0]))
    assert any(under[t] != plain[t] for t in under)                      # the second pass ran under other weights
    rates = summary.scalars(str(d / 'train'))['ema/rate']
    assert [s for s, _ in rates] == [0, 1] and [np.float32(v) for _, v in rates] == [ema.rate(0.99, 0), ema.rate(0.99, 1)]
    with caplog.at_level('INFO', logger='kpx'):
        train.main(argv + ['--steps', '3', '--resume', 'latest'])
    assert 'averaged weights restored' in caplog.text and 'global_step 2' in caplog.text
    last = BaseModel.read_checkpoint(str(d / 'model.ckpt-2.npz'))
    assert int(last['global_step']) == 3 and sorted(last) == sorted(arrays)
    assert any(not np.array_equal(last[k], arrays[k]) for k in shadows)                  # the averages went on
    assert [s for s, _ in summary.scalars(str(d / 'test_ema'))[sorted(under)[0]]] == [0, 1, 2]
