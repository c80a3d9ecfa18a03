"""GPU: the key-point action classifier -- the three HIP entries against the float64 restatement (classifier_ref.py) at every lane
boundary, argument errors, graph replay; ActionClassifierModel against the fp32 restatement at a toy size (manifest, two train steps,
checkpoints in both containers), against a float64 arbiter at the default size, and on the planted problem; train.py --mode
action_classifier --synthetic against the model stepped by hand; then train.py --mode action_classifier and evaluate.py --metrics --actions
--action-accuracy end to end on the fixture videos."""
import json
import os

import numpy as np
import pytest
import torch

import classifier_ref as C

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
K, A, CELLS = 5, 9, (32, 32)
ROWS = (1, 3, 64, 65, 257)
CLASSES = (1, 2, 9, 63, 64, 65, 1024)


def _ops():
    from kpx_amd import ops
    return ops


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _logits(kind, b, a, rs, target):
    if kind == 'normal':
        return rs.randn(b, a).astype(np.float32)
    if kind == 'large':                                  # exp overflows without the max subtraction
        return (rs.randn(b, a) * 3e4).astype(np.float32)
    if kind == 'constant':
        return np.repeat(rs.randn(b, 1).astype(np.float32), a, axis=1)
    x = rs.randint(-2, 3, size=(b, a)).astype(np.float32)      # 'ties': small integers, so equal values are exact
    for i in range(b):
        if i % 2 == 0:                                   # the target's value at the maximum, shared with one more class where there is one
            x[i, target[i]] = 2.0
            x[i, (target[i] + 1) % a] = 2.0
        else:                                            # the target below the maximum, tied with one more class
            x[i, target[i]] = 0.0
            x[i, (target[i] + a // 2) % a] = 0.0
    return x


def _labels(kind, b, a, rs, target):
    if kind == 'normal':                                 # soft rows that sum to 1 up to fp32 rounding
        w = rs.rand(b, a) + 0.05
        return (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    return np.eye(a, dtype=np.float32)[target]


@pytest.mark.parametrize('a', CLASSES)
@pytest.mark.parametrize('b', ROWS)
def test_softmax_xent_matches_the_float64_restatement(b, a):
    ops = _ops()
    rs = np.random.RandomState(1000 * b + a)
    for kind in ('normal', 'large', 'constant', 'ties'):
        target = rs.randint(0, a, size=b)
        x, y = _logits(kind, b, a, rs, target), _labels(kind, b, a, rs, target)
        xd, yd = _dev(x).requires_grad_(True), _dev(y)
        loss, lse = ops.SoftmaxXentFn.apply(xd, yd)
        want_loss, want_lse = C.softmax_xent_fwd(x, y)
        u_loss, u_lse = float(C.ulps(loss.detach().cpu().numpy(), [want_loss]).max()), float(C.ulps(lse.cpu().numpy(), want_lse).max())
        # the backward of the autograd function, with a device-side scale (dloss) as kpx_l1_pair_bwd_f32 takes it
        g = np.float32(0.3) if kind == 'large' else np.float32(1.0)
        loss.backward(_dev(np.array([g], np.float32)))
        want_d = C.softmax_xent_bwd(x, y, lse.cpu().numpy(), gscale_dev=g, gscale_host=1.0)
        u_d = float(C.ulps(xd.grad.cpu().numpy(), want_d, floor=C.FLT_MIN).max())
        print('B=%d A=%d %s: ulps loss %.2f lse %.2f dlogits %.2f' % (b, a, kind, u_loss, u_lse, u_d))
        assert u_loss <= 1 and u_lse <= 1 and u_d <= 1, (kind, u_loss, u_lse, u_d)
        assert tuple(loss.shape) == (1,) and tuple(lse.shape) == (b,) and tuple(xd.grad.shape) == (b, a)
        if a == 1:                                       # one class: the loss and its gradient are exactly zero
            assert float(loss.detach()) == 0.0 and not xd.grad.cpu().numpy().any()


@pytest.mark.parametrize('a', CLASSES)
@pytest.mark.parametrize('m', ROWS)
def test_class_scores_match_the_restatement(m, a):
    ops = _ops()
    rs = np.random.RandomState(2000 * m + a)
    conf = torch.zeros((a, a), dtype=torch.int32, device=DEV)
    want_conf = np.zeros((a, a), np.int32)
    for call, kind in enumerate(('normal', 'ties', 'large', 'constant')):          # the confusion counts accumulate over the calls
        target = rs.randint(0, a, size=m)
        x = _logits(kind, m, a, rs, target)
        if kind == 'normal':                             # one row with a NaN, one with +inf
            x[0, rs.randint(0, a)] = np.nan
            if m > 1:
                x[m - 1, rs.randint(0, a)] = np.inf
        pred, rank, logp = ops.class_scores(_dev(x), _dev(target.astype(np.int32)), conf)
        want_pred, want_rank, want_logp = C.class_scores(x, target, want_conf)
        assert pred.dtype == torch.int32 and rank.dtype == torch.int32 and logp.dtype == torch.float32
        assert np.array_equal(pred.cpu().numpy(), want_pred), kind
        assert np.array_equal(rank.cpu().numpy(), want_rank), kind
        u = float(C.ulps(logp.cpu().numpy(), want_logp).max())
        print('M=%d A=%d %s: logp ulps %.2f' % (m, a, kind, u))
        assert u <= 1, (kind, u)
        assert np.array_equal(conf.cpu().numpy(), want_conf), (kind, call)
        if kind == 'normal':
            assert int(pred[0]) == -1 and int(rank[0]) == a and bool(torch.isnan(logp[0]))
    # without the confusion matrix, into given outputs
    out = (torch.empty(m, dtype=torch.int32, device=DEV), torch.empty(m, dtype=torch.int32, device=DEV), torch.empty(m, device=DEV))
    got = ops.class_scores(_dev(x), _dev(target.astype(np.int32)), out=out)
    assert all(g is o for g, o in zip(got, out)) and np.array_equal(out[1].cpu().numpy(), want_rank)


def test_bad_arguments_raise_kpx_error_and_launch_nothing():
    from kpx_amd import _lib
    from kpx_amd._lib import KpxError
    ops = _ops()
    x, y = torch.zeros((4, 9), device=DEV), torch.zeros((4, 9), device=DEV)
    t = torch.zeros(4, dtype=torch.int32, device=DEV)
    wide = torch.zeros((4, 18), device=DEV)
    conf = torch.full((9, 9), 7, dtype=torch.int32, device=DEV)
    out = tuple(torch.full((4,), 7, dtype=dt, device=DEV) for dt in (torch.int32, torch.int32, torch.float32))
    bad = [lambda: ops.softmax_xent(x.cpu(), y),                                          # device
           lambda: ops.softmax_xent(x, y.cpu()),
           lambda: ops.softmax_xent(x.double(), y),                                       # dtype
           lambda: ops.softmax_xent(x, y.double()),
           lambda: ops.softmax_xent(wide[:, ::2], y),                                     # contiguity
           lambda: ops.softmax_xent(x, wide[:, ::2]),
           lambda: ops.softmax_xent(x, y[:3]),                                            # shapes
           lambda: ops.softmax_xent(x, torch.zeros((4, 8), device=DEV)),
           lambda: ops.softmax_xent(x[0], y[0]),
           lambda: ops.softmax_xent(torch.zeros((0, 9), device=DEV), torch.zeros((0, 9), device=DEV)),
           lambda: ops.softmax_xent(torch.zeros((2, 1025), device=DEV), torch.zeros((2, 1025), device=DEV)),
           lambda: ops.class_scores(x.cpu(), t, conf, out),
           lambda: ops.class_scores(x, t.cpu(), conf, out),
           lambda: ops.class_scores(x.double(), t, conf, out),
           lambda: ops.class_scores(x, t.long(), conf, out),
           lambda: ops.class_scores(x, t.float(), conf, out),
           lambda: ops.class_scores(wide[:, ::2], t, conf, out),
           lambda: ops.class_scores(x, t[:3], conf, out),
           lambda: ops.class_scores(x, t, conf.float(), out),
           lambda: ops.class_scores(x, t, conf[:8], out),
           lambda: ops.class_scores(x, t, conf.cpu(), out),
           lambda: ops.class_scores(x, t, conf, (out[0], out[1], out[2].double())),
           lambda: ops.class_scores(x, t, conf, (out[0][:3], out[1], out[2])),
           lambda: ops.class_scores(x, t + 9, conf, out),                                 # a target outside [0, A)
           lambda: ops.class_scores(x, t - 1, conf, out),
           lambda: ops.class_scores(torch.zeros((2, 1025), device=DEV), t[:2], None, None)]
    torch.cuda.synchronize()
    launched = _lib.abi_calls[0]
    for i, fn in enumerate(bad):
        with pytest.raises(KpxError):
            fn()
            pytest.fail('case %d raised nothing' % i)
    assert _lib.abi_calls[0] == launched                                              # no entry was called ...
    assert bool((conf == 7).all()) and all(bool((o == 7).all()) for o in out)         # ... and nothing was written


def test_three_launch_graph_replays_bitwise():
    from kpx_amd._lib import lib, check
    ops = _ops()
    b, a = 65, 9
    rs = np.random.RandomState(4)
    target = rs.randint(0, a, size=b)
    x, y, t = _dev(rs.randn(b, a).astype(np.float32)), _dev(np.eye(a, dtype=np.float32)[target]), _dev(target.astype(np.int32))
    g = _dev(np.array([0.7], np.float32))
    bufs = dict(loss=torch.empty(1, device=DEV), lse=torch.empty(b, device=DEV), dl=torch.empty((b, a), device=DEV),
                pred=torch.empty(b, dtype=torch.int32, device=DEV), rank=torch.empty(b, dtype=torch.int32, device=DEV),
                logp=torch.empty(b, device=DEV), conf=torch.zeros((a, a), dtype=torch.int32, device=DEV))

    def enqueue():
        s = ops._stream()
        check(lib.kpx_softmax_xent_fwd_f32(x.data_ptr(), y.data_ptr(), b, a, bufs['loss'].data_ptr(), bufs['lse'].data_ptr(), s), 'fwd')
        check(lib.kpx_softmax_xent_bwd_f32(x.data_ptr(), y.data_ptr(), bufs['lse'].data_ptr(), b, a, g.data_ptr(), 1.0, bufs['dl'].data_ptr(), s), 'bwd')
        ops.class_scores(x, t, bufs['conf'], out=(bufs['pred'], bufs['rank'], bufs['logp']))

    enqueue()
    torch.cuda.synchronize()
    eager = {n: v.clone() for n, v in bufs.items()}
    assert int(eager['conf'].sum()) == b and float(eager['loss']) > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for n, v in bufs.items():
        v.zero_() if n == 'conf' else v.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    for n, v in bufs.items():
        assert torch.equal(v, eager[n]), n


# ------------------------------------------------------------------------------------------------ 2. the model
def _make(k=K, cells=CELLS, b=3, lr=1e-4, log_dir='/tmp/kpx_classifier'):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': lr, 'step': 20000, 'decay': 0.95}, 'batch_size': b},
           'model': {'n_pts': k, 'n_action': A, 'classifier_cells': list(cells)}, 'paths': {'log_dir': log_dir}}
    model = kpx_amd.ActionClassifierModel(cfg, device=DEV)
    model.build()
    return model


def _batch(rs, b, k=K):
    seq = (rs.rand(b, 32, k, 2) * 1.6 - 0.8).astype(np.float32)
    ac = np.eye(A, dtype=np.float32)[rs.randint(0, A, size=b)]
    return seq, ac, {'real_seq': _dev(seq), 'action_code': _dev(ac)}


def test_manifest_and_train_steps_match_the_restatement():
    model = _make()
    manifest = C.classifier_manifest(K, A, CELLS)
    assert {n: tuple(v.shape) for n, v in model.store.vars.items()} == {n: tuple(s) for n, s in manifest.items()}
    params = C.init_classifier(K, A, CELLS, seed=5)
    model.store.load_numpy(params, strict=True)
    st = C.ClassifierTrainState(params, CELLS)
    rs = np.random.RandomState(1)
    for step in range(2):                                # the second step's loss sees the first step's Adam update
        seq, ac, feed = _batch(rs, 3)
        want = C.classifier_train_step(st, seq, ac)
        model.train_step(None, feed, step, 3)
        got = model.loss_values()
        assert abs(got['loss'] - want['loss']) <= 2e-5 * max(1.0, abs(want['loss'])), (step, got['loss'], want['loss'])
        assert got['accuracy'] == want['accuracy'] and abs(got['lr'] - want['lr']) < 1e-12
        assert rel_l2(model.last['logits'].cpu().numpy(), want['logits'].numpy()) < 1e-5
        assert set(want['grads']) == set(model.store.vars)
        for n, g in want['grads'].items():               # every variable, none skipped: the random inputs give each a gradient
            assert float(g.abs().max()) > 1e-7, n
            assert rel_l2(model.store.grad(n).cpu().numpy(), g.numpy()) < 2e-4, (step, n)
        exp = model.store.export_numpy(include_slots=False)
        for n, p in st.params.items():                   # after Adam: an element whose gradient is rounding noise may flip sign (+-lr)
            diff = np.abs(exp[n] - p.numpy())
            assert diff.max() <= (step + 1) * 2.05e-4 and np.mean(diff > 1e-5) < 0.02, (step, n, float(diff.max()))
    assert model.global_step == 2 and not model.store.buckets['D'].entries
    # classify: the same network without gradients, [M,32,K,2] or [M,32,2K]
    logits, feats = model.classify(feed['real_seq'])
    p = {n: torch.from_numpy(v) for n, v in model.store.export_numpy(include_slots=False).items()}
    want_logits, want_feats = C.classifier_forward(p, torch.from_numpy(seq).reshape(3, 32, 2 * K), CELLS)
    assert tuple(logits.shape) == (3, A) and tuple(feats.shape) == (3, CELLS[-1]) and not logits.requires_grad
    assert rel_l2(logits.cpu().numpy(), want_logits.numpy()) < 1e-5 and rel_l2(feats.cpu().numpy(), want_feats.numpy()) < 1e-5
    assert torch.equal(model.classify(feed['real_seq'].reshape(3, 32, 2 * K))[0], logits)
    loss, n_correct, _, n = model.test_step(None, feed, 2, 0, 3)
    assert n == 3 and 0 <= n_correct <= 3 and model.collect_test_results([(loss, n_correct, 0.1, 3), (2 * loss, 0, 0.1, 1)], 2) == \
        ((3 * loss + 2 * loss) / 4, n_correct / 4.0)


@pytest.mark.parametrize('fmt', ['npz', 'tf'])
def test_checkpoint_round_trip_continues_bitwise(tmp_path, fmt):
    rs = np.random.RandomState(2)
    feeds = [_batch(rs, 3)[2] for _ in range(3)]
    model = _make(log_dir=str(tmp_path))
    model.initialize_loggers(str(tmp_path))
    for step in range(2):
        model.train_step(None, feeds[step], step, 3)
    arrays = model.checkpoint_arrays()
    for name in ('seq_classifier/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel', 'seq_classifier/rnn/multi_rnn_cell/cell_1/basic_lstm_cell/bias',
                 'seq_classifier/fully_connected/weights', 'seq_classifier/fully_connected/biases',
                 'seq_classifier/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel/Adam', 'seq_classifier/fully_connected/biases/Adam_1',
                 'global_step', 'beta1_power', 'beta2_power'):
        assert name in arrays, name
    assert np.asarray(arrays['global_step']).dtype == np.int32 and int(arrays['global_step']) == 2
    assert not any('discr' in n or n.endswith('_power_1') for n in arrays)
    path = model.save_checkpoint(None, 2, fmt=fmt)
    model.close_loggers()
    assert os.path.dirname(path) == str(tmp_path / 'action_classifier')
    model.train_step(None, feeds[2], 2, 3)
    other = _make(log_dir=str(tmp_path))
    other.restore(None, path, strict=True)
    assert other.global_step == 2 and [float(v) for v in other.beta_power] == [0.125, float(np.float32(np.float32(0.999) * np.float32(0.999)) * np.float32(0.999))]
    other.train_step(None, feeds[2], 2, 3)
    assert torch.equal(other.last['loss'], model.last['loss']) and torch.equal(other.last['logits'], model.last['logits'])
    for which in ('params', 'm', 'v'):
        assert torch.equal(getattr(other.store.buckets['G'], which), getattr(model.store.buckets['G'], which)), which
    # a recogniser of another width is refused by name
    with pytest.raises(Exception, match=r'model\.classifier_cells'):
        _make(cells=(32, 16), log_dir=str(tmp_path)).restore(None, path, strict=True)


def test_default_size_gradients_against_the_float64_arbiter():
    """K = 40, cells [256, 256], B = 16, first step: per variable the GPU's gradient error against the float64 restatement is at most
    4x the fp32 restatement's + 2e-6 (the stage-2 arbiter rule)."""
    k, cells, b = 40, (256, 256), 16
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    model = _make(k, cells, b)
    params = C.init_classifier(k, A, cells, seed=5)
    model.store.load_numpy(params, strict=True)
    seq, ac, feed = _batch(np.random.RandomState(1), b, k)
    model.train_step(None, feed, 0, b)
    g32, l32, _ = C.classifier_gradients(params, seq, ac, cells, torch.float32)
    g64, l64, _ = C.classifier_gradients(params, seq, ac, cells, torch.float64)
    assert abs(model.loss_values()['loss'] - l64) <= 2e-5 * max(1.0, abs(l64))
    rep = []
    for n in params:
        e_gpu, e_cpu = rel_l2(model.store.grad(n).cpu().numpy(), g64[n].numpy()), rel_l2(g32[n].numpy(), g64[n].numpy())
        rep.append('%s %.2e (CPU fp32 %.2e)' % (n, e_gpu, e_cpu))
    print('gradient rel-L2 vs float64:\n  ' + '\n  '.join(rep))
    for n in params:
        e_gpu, e_cpu = rel_l2(model.store.grad(n).cpu().numpy(), g64[n].numpy()), rel_l2(g32[n].numpy(), g64[n].numpy())
        assert e_gpu <= 4 * e_cpu + 2e-6, (n, e_gpu, e_cpu)


def test_learns_the_planted_problem():
    """One fixed batch of 16 of kpx_amd.synthetic.planted_action_batch(seed=3), cells (32, 32), lr 1e-2, initial values init_classifier(seed=5).
    The fp32 restatement on the CPU is below half its first loss after N = 4 steps; its loss before the steps 0, 4, 8, ..., 76:
      2.197 0.998 0.653 0.317 0.568 0.476 0.096 0.059 0.041 0.032 0.026 0.022 0.019 0.016 0.014 0.013 0.012 0.010 0.009 0.009
    The GPU model must be below half its own first loss after 2 N = 8 steps (2x for a different rounding path)."""
    from kpx_amd.synthetic import planted_action_batch
    n_half = 4                                           # N of the restatement (see above)
    model = _make(lr=1e-2, b=16)
    model.store.load_numpy(C.init_classifier(K, A, CELLS, seed=5), strict=True)
    feed = {n: _dev(v) for n, v in planted_action_batch(16, K, A, seed=3).items()}
    losses = []
    for step in range(2 * n_half + 1):                   # the loss of step i is taken before its update: after 2 N updates
        model.train_step(None, feed, step, 16)
        losses.append(float(model.last['loss'].cpu()[0]))
    print('planted problem: ' + ' '.join('%.3f' % v for v in losses))
    assert abs(losses[0] - 2.197) < 2e-3 and losses[-1] < 0.5 * losses[0], losses


def test_train_py_synthetic_feeds_the_planted_problem(tmp_path):
    """train.py --mode action_classifier --synthetic: the planted batches of every step, a test pass on the planted test batch, the
    checkpoint of the last interval -- the same final parameters as the model stepped by hand on those batches."""
    import yaml
    import train
    from kpx_amd import summary
    from kpx_amd.synthetic import planted_action_batch
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 100, 'summary_interval': 2, 'test_interval': 2, 'checkpoint_interval': 2, 'log_interval': 1, 'batch_size': 4,
                        'lr': {'start_val': 1e-3, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': K, 'n_action': A, 'classifier_cells': list(CELLS)}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    train.main(['--mode', 'action_classifier', '--config', str(cfg_path), '--synthetic', '--steps', '3'])
    out = tmp_path / 'results' / 'action_classifier'
    got = np.load(str(out / 'model.ckpt-2.npz'))
    model = _make(b=4, lr=1e-3)
    for step in range(3):                                # the checkpoint of step 2 is written after its update: three updates
        model.train_step(None, {n: _dev(v) for n, v in planted_action_batch(4, K, A, seed=step).items()}, step, 4)
    want = model.checkpoint_arrays()
    assert sorted(k.replace('|', '/') for k in got.files) == sorted(want)
    for name, w in want.items():
        assert np.array_equal(got[name.replace('/', '|')], w), name
    scal = summary.scalars(summary.event_files(str(out / 'train'))[0])
    assert sorted(scal) == ['accuracy', 'lr', 'xent_loss'] and [s for s, _ in scal['xent_loss']] == [0, 2]
    assert [s for s, _ in summary.scalars(summary.event_files(str(out / 'test'))[0])['accuracy']] == [0, 2]


# ------------------------------------------------------------------------------------------------ 3. end to end on the fixture videos
def test_train_and_evaluate_end_to_end_on_the_fixture_videos(tmp_path, monkeypatch):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    import train
    from kpx_amd import frechet as F
    from kpx_amd import summary
    from test_data_gpu import _fixture_dataset
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k, n_action = int(golden['n_points']), int(golden['n_action'])
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 3, 'summary_interval': 1, 'test_interval': 2, 'checkpoint_interval': 2, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-3, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8, 'classifier_cells': [32, 32]}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt])

    # ---- train.py --mode action_classifier: a checkpoint and the three scalars in both event directories
    train.main(['--mode', 'action_classifier', '--config', str(cfg_path), '--steps', '3', '--resident-labels'])
    cls_dir = tmp_path / 'results' / 'action_classifier'
    cls_ckpt = str(cls_dir / 'model.ckpt-2.npz')
    assert os.path.exists(cls_ckpt) and os.path.exists(str(cls_dir / 'model.ckpt-0.npz'))
    tags = {}
    for sub in ('train', 'test'):
        files = summary.event_files(str(cls_dir / sub))
        assert len(files) == 1
        tags[sub] = [(ev['step'], v['tag']) for ev in summary.read_events(files[0]) for v in ev.get('values', [])]
    assert tags['train'] == [(s, t) for s in range(3) for t in ('xent_loss', 'accuracy', 'lr')]
    assert tags['test'] == [(s, t) for s in (0, 2) for t in ('xent_loss', 'accuracy')]

    # ---- evaluate.py with the flag, FinalModel.run recorded; and the same run without the flag
    calls = []
    run = kpx_amd.FinalModel.run
    host = lambda t: None if t is None else t.detach().cpu().numpy().copy()

    def recording_run(self, sess, feed_dict, z=None):
        out = run(self, sess, feed_dict, z=z)
        calls.append({'kp': host(out['fut_pt_raw'])})
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    actions, n_draws = [3, 7, 0], 2
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics', '--no-save',
            '--samples', '2', '--actions', '3,7,0']
    torch.manual_seed(11)
    evaluate.main(base + ['--action-accuracy', cls_ckpt, '--save_dir', str(tmp_path / 'eval')])
    rec = list(calls)
    monkeypatch.setattr(kpx_amd.FinalModel, 'run', run)
    torch.manual_seed(11)
    evaluate.main(base + ['--save_dir', str(tmp_path / 'plain')])

    loader = kpx_amd.data.SequenceDataLoader(str(data), 'test', n_points=k, n_action=n_action, random_order=False, randomness=False)
    batches = [{key: b[key].cpu().numpy() for key in ('real_seq', 'action_code')} for b in loader.batches(2, DEV, repeat=False)]
    sizes = [b['real_seq'].shape[0] for b in batches]
    n_cls, s_total = len(actions), sum(sizes)
    assert len(rec) == len(batches) * n_draws * (1 + n_cls)
    group = lambda b, d: rec[(b * n_draws + d) * (1 + n_cls):(b * n_draws + d + 1) * (1 + n_cls)]

    # the recogniser's own logits and features on the recorded key points (the kernels are deterministic: the values evaluate.py saw)
    model = kpx_amd.ActionClassifierModel(cfg, is_training=False, device=DEV)
    model.build()
    model.restore(None, cls_ckpt, strict=True)
    classify = lambda kp: tuple(t.cpu().numpy() for t in model.classify(_dev(kp)))
    own = np.concatenate([b['action_code'].argmax(axis=1) for b in batches])
    real = [classify(b['real_seq']) for b in batches]
    pred = [[classify(group(b, d)[0]['kp']) for d in range(n_draws)] for b in range(len(batches))]
    act = [[[classify(c['kp']) for c in group(b, d)[1:]] for d in range(n_draws)] for b in range(len(batches))]
    real_logits = np.concatenate([r[0] for r in real])
    pred_logits = np.concatenate([np.stack([pred[b][d][0] for d in range(n_draws)], axis=1) for b in range(len(batches))])           # [S, D, A]
    act_logits = np.concatenate([np.stack([np.stack([act[b][d][a][0] for d in range(n_draws)], axis=1) for a in range(n_cls)], axis=1)
                                 for b in range(len(batches))])                                                                 # [S, C, D, A]
    want = C.accuracy_arrays(n_action, own, real_logits, pred_logits, actions, act_logits)

    npz = np.load(str(tmp_path / 'eval' / 'metrics.npz'))
    new_keys = sorted(list(want) + ['kp_fd', 'kp_fd_dim', 'kp_fd_draw0', 'kp_fd_floor'])
    assert sorted(n for n in npz.files if n.startswith('cls_') or n.startswith('kp_fd')) == new_keys
    for name, w in want.items():
        assert npz[name].shape == w.shape, name
        if name.endswith('_logp'):
            assert npz[name].dtype == np.float32 and float(C.ulps(npz[name], w).max()) <= 1, name
        else:
            assert npz[name].dtype == np.int32 and np.array_equal(npz[name], w), name
    assert npz['cls_pred_rank'].shape == (s_total, n_draws) and npz['cls_act_rank'].shape == (s_total, n_cls, n_draws)
    assert int(npz['cls_confusion_commanded'].sum()) == s_total * n_cls * n_draws and int(npz['kp_fd_dim']) == 32

    # ---- the Frechet distances from float64 moments of the same features
    def stats(rows):
        x = np.asarray(rows, np.float32).astype(np.float64)
        return F.stats_from_moments(x.shape[0], x.sum(axis=0), x.T @ x), x
    real_feats = np.concatenate([r[1] for r in real])
    pred_feats = np.concatenate([pred[b][d][1] for b in range(len(batches)) for d in range(n_draws)])
    draw0_feats = np.concatenate([pred[b][0][1] for b in range(len(batches))])
    sets = {'real': stats(real_feats), 'pred': stats(pred_feats), 'pred_draw0': stats(draw0_feats), 'real_even': stats(real_feats[0::2]),
            'real_odd': stats(real_feats[1::2])}
    eps = 2.0 ** -53
    for key, (x, y) in {'kp_fd': ('pred', 'real'), 'kp_fd_draw0': ('pred_draw0', 'real'), 'kp_fd_floor': ('real_even', 'real_odd')}.items():
        (sx, rx), (sy, ry) = sets[x], sets[y]
        w = F.frechet_distance(sx['mean'], sx['cov'], sy['mean'], sy['cov'])
        got = float(npz[key])
        if sx['cov'] is None or sy['cov'] is None:
            assert np.isnan(got) and np.isnan(w), key
            continue
        # moments_add's bound (test_frechet_gpu.py): each moment within (m + 2) eps of the sum of its terms' magnitudes, here and in the
        # float64 sums above; so each covariance entry within e_cov, a covariance within d_cov = dim e_cov in the operator norm.  Through
        # the distance: the traces move by at most dim e_cov each (the mean term by less); S = c1^(1/2) by at most sqrt(d_cov) (the matrix
        # square root is Hoelder-1/2 on PSD matrices); S c2 S by at most d_m = 2 sqrt(d_cov) |c2| |S| + |S|^2 d_cov; each of its dim
        # eigenvalues l by at most d_m, and |sqrt(l + d) - sqrt(l)| <= sqrt(d).  (Most eigenvalues ARE rounding noise around 0 here: three
        # samples span two dimensions of 32.)
        dim = rx.shape[1]
        e_cov = max(4 * (r.shape[0] + 2) * eps * float((r * r).sum()) / max(r.shape[0] - 1, 1) for r in (rx, ry))
        scale = max(float(np.trace(st['cov'])) for st in (sx, sy))                      # >= the operator norm of either covariance
        d_cov = dim * e_cov
        d_m = 2 * np.sqrt(d_cov) * scale * np.sqrt(scale) + scale * d_cov
        bound = 4 * dim * e_cov + 2 * dim * np.sqrt(d_m)
        print('%s: %.6e, restatement %.6e, bound %.2e' % (key, got, w, bound))
        assert abs(got - w) <= bound, (key, got, w, bound)

    # ---- metrics.json: the block is the pure function of the arrays, and says what the quantity is not
    res = json.loads((tmp_path / 'eval' / 'metrics.json').read_text())
    blk = res['action_accuracy']
    assert blk == json.loads(json.dumps(evaluate.summarise_action_accuracy({n: npz[n] for n in npz.files}), allow_nan=False))
    assert blk['definition'].endswith('it is not comparable with published action-recognition accuracies or FVD figures.')
    assert blk['actions'] == actions and blk['n_samples'] == s_total and blk['kp_fd']['rank_deficient']['kp_fd'] is True

    # ---- without the flag: byte for byte what the flag's run wrote, less the new keys
    plain = np.load(str(tmp_path / 'plain' / 'metrics.npz'))
    assert sorted(plain.files) == sorted(n for n in npz.files if not (n.startswith('cls_') or n.startswith('kp_fd')))
    for name in plain.files:
        assert plain[name].dtype == npz[name].dtype and plain[name].tobytes() == npz[name].tobytes(), name
    del res['action_accuracy']
    assert (tmp_path / 'plain' / 'metrics.json').read_text() == json.dumps(res, indent=1, allow_nan=False)
