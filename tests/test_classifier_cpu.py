"""CPU: the key-point action classifier without a GPU -- the restatement (classifier_ref.py) against torch's cross_entropy in float64,
summarise_action_accuracy on hand-made arrays, every parser.error of evaluate.py --action-accuracy and train.py --mode action_classifier,
the argument checks of the three C entries and of their ops wrappers, the model's variable manifest and the planted problem."""
import os
import sys

import numpy as np
import pytest
import torch

import classifier_ref as C

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_abi_has_the_classifier_entries():
    from kpx_amd import _lib
    assert _lib.ABI_VERSION >= 17
    for name in ('kpx_softmax_xent_fwd_f32', 'kpx_softmax_xent_bwd_f32', 'kpx_class_scores_f32'):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('b,a,scale', [(1, 1, 1.0), (3, 9, 1.0), (65, 64, 1.0), (5, 1024, 1.0), (7, 9, 3e4)])
def test_restatement_equals_torch_cross_entropy_in_float64(b, a, scale):
    rs = np.random.RandomState(b * 1000 + a)
    logits = (rs.randn(b, a) * scale).astype(np.float32)
    target = rs.randint(0, a, size=b)
    labels = np.eye(a, dtype=np.float32)[target]
    x = torch.from_numpy(logits).double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(x, torch.from_numpy(target))
    want.backward()
    loss, lse = C.softmax_xent_fwd(logits, labels)
    want = want.detach()
    assert abs(loss - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert np.allclose(lse, torch.logsumexp(x.detach(), dim=1).numpy(), rtol=1e-14, atol=0)
    # the backward takes the forward's lse rounded to fp32: exact-lse gradient up to that rounding (relative 2^-24 of |lse| in the exponent)
    exact = C.softmax_xent_bwd(logits, labels, lse.astype(np.float32), gscale_host=1.0)
    slack = np.abs(lse).max() * 2.0 ** -24 * 1.01 / b + 1e-15
    assert np.abs(exact - x.grad.numpy()).max() <= slack
    # the scale is fl32(host * dev)
    scaled = C.softmax_xent_bwd(logits, labels, lse.astype(np.float32), gscale_dev=np.float32(0.3), gscale_host=1.7)
    assert np.allclose(scaled, exact * float(np.float32(1.7) * np.float32(0.3)), rtol=1e-15, atol=0)
    # the log-probability of the scores is the row's -loss
    pred, rank, logp = C.class_scores(logits, target)
    rows = -torch.nn.functional.cross_entropy(x.detach(), torch.from_numpy(target), reduction='none').numpy()
    assert np.allclose(logp, rows, rtol=1e-12, atol=1e-12)
    assert np.array_equal(pred, logits.argmax(axis=1)) and rank.min() >= 1 and rank.max() <= a


def test_restatement_scores_ties_and_non_finite_rows():
    x = np.array([[1, 3, 3, 0],            # tie at the maximum: pred the lowest index; target 2 ties with 1 -> rank 2
                  [2, 2, 2, 2],            # constant row: every other class ties -> rank A
                  [0, np.nan, 1, 2],       # non-finite
                  [0, 1, np.inf, 2],
                  [5, 1, 1, 0]], np.float32)
    conf = np.zeros((4, 4), np.int32)
    pred, rank, logp = C.class_scores(x, [2, 3, 3, 2, 1], conf)
    assert pred.tolist() == [1, 0, -1, -1, 0] and rank.tolist() == [2, 4, 4, 4, 3]
    assert np.isnan(logp[2]) and np.isnan(logp[3]) and np.isfinite(logp[[0, 1, 4]]).all()
    assert abs(logp[1] - np.log(0.25)) < 1e-15
    want = np.zeros((4, 4), np.int32)
    want[2, 1] = want[3, 0] = want[1, 0] = 1
    assert np.array_equal(conf, want)
    assert C.ulps(np.float32([1.0, np.nan, 0.0]), [1.0 + 2.0 ** -23, np.nan, 1e-45], floor=C.FLT_MIN).tolist() == [1.0, 0.0, 1.0]


def test_classifier_restatement_runs_in_both_precisions_and_learns_the_planted_problem():
    from kpx_amd.synthetic import planted_action_batch
    k, a, cells = 5, 9, (32, 32)
    batch = planted_action_batch(16, k, a, seed=3)
    assert batch['real_seq'].shape == (16, 32, k, 2) and batch['action_code'].sum(axis=1).tolist() == [1.0] * 16
    # the class decides the direction of the drift: the mean displacement of a sample points at 2 pi c / A
    disp = (batch['real_seq'][:, -1] - batch['real_seq'][:, 0]).mean(axis=1)
    ang = np.arctan2(disp[:, 1], disp[:, 0]) % (2 * np.pi)
    cls = batch['action_code'].argmax(axis=1)
    assert np.abs(((ang - 2 * np.pi * cls / a) + np.pi) % (2 * np.pi) - np.pi).max() < 0.2
    params = C.init_classifier(k, a, cells, seed=5)
    assert {n: v.shape for n, v in params.items()} == dict(C.classifier_manifest(k, a, cells))
    g32, l32, _ = C.classifier_gradients(params, batch['real_seq'], batch['action_code'], cells, torch.float32)
    g64, l64, _ = C.classifier_gradients(params, batch['real_seq'], batch['action_code'], cells, torch.float64)
    assert abs(l32 - l64) < 1e-5 and all(g64[n].dtype == torch.float64 and float((g32[n].double() - g64[n]).norm() / g64[n].norm()) < 1e-4 for n in g64)
    st = C.ClassifierTrainState(params, cells, lr_cfg={'start_val': 1e-2, 'step': 20000, 'decay': 0.95})
    first = C.classifier_train_step(st, batch['real_seq'], batch['action_code'])
    assert abs(first['loss'] - np.log(a)) < 0.5 and set(first['grads']) == set(params)
    for _ in range(59):
        last = C.classifier_train_step(st, batch['real_seq'], batch['action_code'])
    assert last['loss'] < 0.5 * first['loss']


# ------------------------------------------------------------------------------------------------ summarise_action_accuracy
def _hand_made():
    """A = 3, S = 4 samples of the classes 0, 1, 1, 0 (class 2 is empty), D = 2 draws, C = 2 listed classes (2, 0)"""
    nan = np.nan
    arrays = {
        'cls_own': np.array([0, 1, 1, 0], np.int32),
        'cls_real_pred': np.array([0, 1, 0, -1], np.int32), 'cls_real_rank': np.array([1, 1, 2, 3], np.int32),       # sample 2: a tie, sample 3: NaN
        'cls_real_logp': np.array([-0.5, -0.25, -1.0, nan], np.float32),
        'cls_confusion_real': np.array([[1, 0, 0], [1, 1, 0], [0, 0, 0]], np.int32),
        'cls_pred_pred': np.array([[0, 2], [0, 1], [2, 2], [0, 0]], np.int32), 'cls_pred_rank': np.array([[1, 3], [2, 1], [2, 3], [1, 1]], np.int32),
        'cls_pred_logp': np.array([[-0.5, -2.0], [-1.0, -0.5], [-1.5, -2.5], [-0.25, -0.25]], np.float32),
        'cls_confusion_pred': np.array([[3, 0, 1], [1, 1, 2], [0, 0, 0]], np.int32),
        'actions': np.array([2, 0], np.int32),
        'cls_act_pred': np.array([[[2, 0], [0, 0]], [[1, 2], [0, 1]], [[2, 2], [0, -1]], [[0, 0], [0, 0]]], np.int32),
        'cls_act_rank': np.array([[[1, 2], [1, 1]], [[3, 1], [1, 2]], [[1, 1], [1, 3]], [[2, 2], [1, 1]]], np.int32),
        'cls_act_logp': np.full((4, 2, 2), -1.0, np.float32),
        'cls_confusion_commanded': np.array([[7, 1, 0], [0, 0, 0], [3, 1, 3]], np.int32),
        'kp_fd': np.float64(2.5), 'kp_fd_draw0': np.float64(nan), 'kp_fd_floor': np.float64(0.5), 'kp_fd_dim': np.int32(4)}
    arrays['cls_act_logp'][2, 1, 1] = nan
    return arrays


def test_summarise_action_accuracy_on_hand_made_arrays():
    import json
    import evaluate
    blk = evaluate.summarise_action_accuracy(_hand_made())
    json.dumps(blk, allow_nan=False)
    assert blk['definition'] == evaluate.ACTION_ACCURACY_DEFINITION
    assert blk['definition'].endswith('it is not comparable with published action-recognition accuracies or FVD figures.')
    assert 'own key-point-space quantity' in blk['definition']
    assert (blk['n_samples'], blk['n_draws'], blk['n_classes']) == (4, 2, 3)
    real = blk['real']
    assert real['n'] == 4 and real['top1'] == 0.5 and real['chance'] == 1 / 3 and real['mean_rank'] == 7 / 4 and real['n_nonfinite'] == 1
    assert abs(real['nll'] - (0.5 + 0.25 + 1.0) / 3) < 1e-7                       # the non-finite row is left out
    assert real['per_class_top1'] == [0.5, 0.5, None]                            # class 2 has no sample
    assert real['confusion'] == [[1, 0, 0], [1, 1, 0], [0, 0, 0]] and 'best_of_draws_top1' not in real
    pred = blk['pred']
    assert pred['n'] == 8 and pred['top1'] == 0.5 and pred['mean_rank'] == 14 / 8 and pred['n_nonfinite'] == 0
    assert pred['per_class_top1'] == [0.75, 0.25, None] and pred['best_of_draws_top1'] == 0.75
    assert abs(pred['nll'] - 8.5 / 8) < 1e-7
    com = blk['commanded']
    assert blk['actions'] == [2, 0] and com['n'] == 16 and com['n_nonfinite'] == 1
    assert com['top1'] == 10 / 16 and com['per_class_top1'] == [6 / 8, None, 4 / 8]
    assert com['best_of_draws_top1'] == 7 / 8 and abs(com['nll'] - 1.0) < 1e-7
    fd = blk['kp_fd']
    assert fd == {'dim': 4, 'n_real': 4, 'n_pred': 8, 'kp_fd': 2.5, 'kp_fd_draw0': None, 'kp_fd_floor': 0.5,
                  'rank_deficient': {'kp_fd': True, 'kp_fd_draw0': True, 'kp_fd_floor': True}}
    # without --actions there is no commanded block; a shape mismatch is named
    plain = {k: v for k, v in _hand_made().items() if not k.startswith('cls_act') and k not in ('actions', 'cls_confusion_commanded')}
    assert 'commanded' not in evaluate.summarise_action_accuracy(plain)
    bad = _hand_made()
    bad['cls_pred_rank'] = bad['cls_pred_rank'][:, :1]
    with pytest.raises(ValueError, match='cls_pred_'):
        evaluate.summarise_action_accuracy(bad)
    # more rows than dimensions: not rank deficient
    big = {k: v for k, v in plain.items()}
    big['kp_fd_dim'] = np.int32(1)
    assert evaluate.summarise_action_accuracy(big)['kp_fd']['rank_deficient'] == {'kp_fd': False, 'kp_fd_draw0': False, 'kp_fd_floor': False}


def test_restatement_arrays_feed_the_summary():
    import evaluate
    rs = np.random.RandomState(0)
    s, d, a, actions = 5, 2, 9, [3, 7, 0]
    own = rs.randint(0, a, size=s)
    arrays = C.accuracy_arrays(a, own, rs.randn(s, a).astype(np.float32), rs.randn(s, d, a).astype(np.float32), actions,
                               rs.randn(s, len(actions), d, a).astype(np.float32))
    arrays.update(actions=np.asarray(actions, np.int32), kp_fd=np.float64(1), kp_fd_draw0=np.float64(1), kp_fd_floor=np.float64(1), kp_fd_dim=np.int32(32))
    blk = evaluate.summarise_action_accuracy(arrays)
    for name, n in (('real', s), ('pred', s * d), ('commanded', s * d * len(actions))):
        assert blk[name]['n'] == n and sum(map(sum, blk[name]['confusion'])) == n
        assert blk[name]['top1'] == sum(blk[name]['confusion'][i][i] for i in range(a)) / n          # no ties in random logits: rank 1 = arg max
    assert arrays['cls_pred_rank'].shape == (s, d) and arrays['cls_act_logp'].shape == (s, len(actions), d)


# ------------------------------------------------------------------------------------------------ the parsers
def test_evaluate_action_accuracy_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import yaml
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    cfg = yaml.safe_load(open(os.path.join(REPO, 'configs', 'penn.yaml')))
    assert 'classifier_cells' not in cfg['model']                     # the key is optional: configs/penn.yaml stays as it is
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    base = ['--config', str(cfg_path), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck), '--save_dir', str(tmp_path / 'eval'),
            '--action-accuracy', str(ck)]
    cases = ((['--samples', '2'], '--action-accuracy adds to the scores of --metrics and needs it'),
             (['--synthetic', '2'], '--action-accuracy classifies the pseudo labels of the real frames'),
             (['--metrics', '--synthetic', '2'], '--action-accuracy classifies the pseudo labels of the real frames'),
             (['--metrics', '--drive', 'hold', '--drive-only'], "--drive-only skips the model's own rollout, which --action-accuracy is about"))
    for extra, text in cases:
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as e:                               # the flag takes a checkpoint
        evaluate.main(base[:-1])
    assert e.value.code == 2 and 'expected one argument' in capsys.readouterr().err
    with pytest.raises(Exception, match='checkpoint not found at .*missing.npz'):
        evaluate.main(base[:-1] + [str(tmp_path / 'missing.npz'), '--metrics'])
    assert not (tmp_path / 'eval').exists()


def test_train_action_classifier_argument_errors(capsys):
    import train
    with pytest.raises(SystemExit):
        train.main(['--mode', 'action_classifier', '--config', 'unused.yaml', '--resident-data'])
    assert '--resident-data keeps JPEG frames in HBM' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.main(['--mode', 'action_classifier', '--config', 'unused.yaml', '--resident-labels', '--synthetic'])
    assert '--resident-labels keeps pseudo labels in HBM' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.main(['--mode', 'action_recogniser', '--config', 'unused.yaml'])
    assert "invalid choice: 'action_recogniser'" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.main(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert 'action_classifier' in text and 'planted problem' in text
    assert 'action_classifier' in train.__doc__


# ------------------------------------------------------------------------------------------------ the entries and the wrappers
def test_entries_reject_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                       # an aligned fake address: nothing is dereferenced before the checks
    fwd = lambda logits=a, labels=a, b=3, n=9, loss=a, lse=a: lib.kpx_softmax_xent_fwd_f32(logits, labels, b, n, loss, lse, None)
    for kw in (dict(logits=None), dict(labels=None), dict(loss=None), dict(lse=None), dict(b=0), dict(b=(1 << 20) + 1), dict(n=0), dict(n=1025),
               dict(logits=a + 2), dict(lse=a + 1)):
        assert fwd(**kw) == -1, kw
    bwd = lambda logits=a, labels=a, lse=a, b=3, n=9, gdev=None, dl=a: lib.kpx_softmax_xent_bwd_f32(logits, labels, lse, b, n, gdev, 1.0, dl, None)
    for kw in (dict(logits=None), dict(labels=None), dict(lse=None), dict(dl=None), dict(b=0), dict(b=(1 << 20) + 1), dict(n=0), dict(n=1025),
               dict(gdev=a + 2), dict(dl=a + 3)):
        assert bwd(**kw) == -1, kw
    sc = lambda logits=a, target=a, m=3, n=9, pred=a, rank=a, logp=a, conf=None: lib.kpx_class_scores_f32(logits, target, m, n, pred, rank, logp,
                                                                                                        conf, None)
    for kw in (dict(logits=None), dict(target=None), dict(pred=None), dict(rank=None), dict(logp=None), dict(m=0), dict(m=(1 << 20) + 1),
               dict(n=0), dict(n=1025), dict(conf=a + 2), dict(target=a + 1)):
        assert sc(**kw) == -1, kw


def test_ops_refuse_cpu_tensors_and_launch_nothing():
    from kpx_amd import _lib, ops
    from kpx_amd._lib import KpxError
    launched = _lib.abi_calls[0]
    x, y = torch.zeros(3, 9), torch.zeros(3, 9)
    with pytest.raises(KpxError, match='no CPU fallback'):
        ops.softmax_xent(x, y)
    with pytest.raises(KpxError, match='no CPU fallback'):
        ops.class_scores(x, torch.zeros(3, dtype=torch.int32))
    assert _lib.abi_calls[0] == launched


def test_model_manifest_and_config_default_on_the_cpu():
    import yaml
    import kpx_amd
    from kpx_amd.action_classifier_model import DEFAULT_CELLS
    assert 'ActionClassifierModel' in kpx_amd.__all__ and kpx_amd.ActionClassifierModel.name == 'action_classifier'
    cfg = yaml.safe_load(open(os.path.join(REPO, 'configs', 'penn.yaml')))
    model = kpx_amd.ActionClassifierModel(cfg, device='cpu')
    assert model.cells == tuple(DEFAULT_CELLS) == (256, 256)
    model.build()
    k, a = cfg['model']['n_pts'], cfg['model']['n_action']
    assert {n: tuple(v.shape) for n, v in model.store.vars.items()} == {n: tuple(s) for n, s in C.classifier_manifest(k, a, (256, 256)).items()}
    assert list(model.store.buckets['G'].entries) == list(model.store.vars) and not model.store.buckets['D'].entries
    cfg['model']['classifier_cells'] = [32, 16]
    small = kpx_amd.ActionClassifierModel(cfg, device='cpu', is_training=False)
    small.build()
    assert tuple(small.store.vars['seq_classifier/fully_connected/weights'].shape) == (16, a)
    arrays = small.checkpoint_arrays()
    assert np.asarray(arrays['global_step']).dtype == np.int32 and 'beta1_power' not in arrays        # no optimiser state outside training
    assert {'global_step', 'beta1_power', 'beta2_power', 'seq_classifier/fully_connected/weights/Adam_1'} <= set(model.checkpoint_arrays())
