"""CPU: the float64 restatement of the VGG feature-space metrics (feature_metrics_ref.py) against closed forms, evaluate.summarise_metrics
with the extra metrics (best draw per direction, ties, non-finite counting, today's result without them), evaluate.py's --vgg-metrics
argument errors, and the argument checks of kpx_feature_pair_metrics_f32."""
import json
import os
import sys

import numpy as np
import pytest

import feature_metrics_ref as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_identical_tensors_score_one_and_zero():
    a = np.maximum(0, np.random.RandomState(0).normal(size=(3, 5, 7, 12)))
    m = F.layer_metrics(a, a)
    assert np.abs(m[:, 0] - 1.0).max() <= 1e-15 and (m[:, 1] == 0).all()


def test_orthogonal_one_hot_channels_score_zero():
    a = np.zeros((1, 4, 4, 8))
    b = np.zeros((1, 4, 4, 8))
    a[..., 2] = 3.0
    b[..., 5] = 0.5
    m = F.layer_metrics(a, b)
    assert m[0, 0] == 0.0
    assert abs(m[0, 1] - 3.5 / 8) <= 1e-15


def test_a_scaled_copy_has_cosine_one_and_the_l1_of_the_difference():
    a = np.maximum(0, np.random.RandomState(1).normal(size=(2, 6, 5, 16))) + 0.01
    m = F.layer_metrics(a, 2 * a)
    assert np.abs(m[:, 0] - 1.0).max() <= 1e-15                       # min(1, .) takes the rounding above 1 away
    assert np.abs(m[:, 1] - np.abs(a).mean(axis=(1, 2, 3))).max() <= 1e-15


def test_zero_positions_follow_the_both_zero_and_one_zero_rules():
    rs = np.random.RandomState(2)
    a = rs.uniform(0.1, 1, size=(1, 2, 2, 4))
    b = a.copy()
    a[0, 0, 0] = 0                                                    # one side zero -> 0
    a[0, 0, 1] = b[0, 0, 1] = 0                                       # both zero -> 1
    b[0, 1, 0] = 0                                                    # the other side zero -> 0
    m = F.layer_metrics(a, b)                                         # position (1, 1): identical -> 1
    assert abs(m[0, 0] - 0.5) <= 1e-15
    assert abs(m[0, 1] - (b[0, 0, 0].sum() + a[0, 1, 0].sum()) / 16) <= 1e-15
    z = np.zeros((1, 3, 3, 4))
    assert F.layer_metrics(z, z)[0].tolist() == [1.0, 0.0]
    assert F.layer_metrics(z, z + 1)[0].tolist() == [0.0, 1.0]
    norm = np.sqrt((a * a).sum(axis=-1))[0]                           # (0, 0) and (0, 1) are zero
    assert abs(F.fragile([a])[0] - min(norm[1, 0], norm[1, 1]) / norm.mean()) <= 1e-15
    assert F.fragile([z]) == [1.0]


def test_frame_scores_stack_the_layers():
    rs = np.random.RandomState(3)
    fa = [rs.uniform(size=(2, 4, 4, 8)), rs.uniform(size=(2, 2, 2, 16))]
    fb = [rs.uniform(size=(2, 4, 4, 8)), rs.uniform(size=(2, 2, 2, 16))]
    s = F.frame_scores(fa, fb)
    assert s.shape == (2, 2, 2)
    assert np.array_equal(s[:, 1], F.layer_metrics(fa[1], fb[1]))


def _draws():
    s, n, t = 2, 3, 32
    ssim = np.full((s, n, t), 0.5)
    psnr = np.full((s, n, t), 20.0)
    mse = np.full((s, n, t), 0.01)
    cos = np.full((s, n, t), 0.4)
    cos[0, 1] = cos[0, 2] = 0.6                                       # sample 0: draws 1 and 2 tie -> draw 1
    cos[1, 2] = np.linspace(0.5, 0.9, t)                              # sample 1: draw 2
    l1 = np.full((s, n, t), 3.0)
    l1[0, 2] = 1.0                                                    # lower is better: draw 2
    l1[1, 0] = l1[1, 1] = 2.0                                         # tie -> draw 0
    return ssim, psnr, mse, cos, l1


def test_summarise_extras_pick_the_best_draw_per_direction_with_ties_to_the_lowest():
    import evaluate
    ssim, psnr, mse, cos, l1 = _draws()
    r = evaluate.summarise_metrics(ssim, psnr, mse, extras={'vgg_cos': cos, 'vgg_l1': l1})
    assert r['vgg_cos']['best_draw'] == [1, 2] and r['vgg_l1']['best_draw'] == [2, 0]
    assert set(r['vgg_cos']) == set(r['ssim']) == set(r['vgg_l1']) == set(r['mse'])
    assert abs(r['vgg_cos']['best_of_draws'] - (0.6 + 0.7) / 2) <= 1e-15
    assert abs(r['vgg_l1']['best_of_draws'] - 1.5) <= 1e-15
    assert r['vgg_cos']['best_of_draws'] >= r['vgg_cos']['mean'] and r['vgg_l1']['best_of_draws'] <= r['vgg_l1']['mean']
    assert np.allclose(r['vgg_cos']['best_of_draws_per_frame'], (cos[0, 1] + cos[1, 2]) / 2, rtol=0, atol=1e-15)
    assert len(r['vgg_l1']['per_frame']) == 32
    assert r['vgg_layers'] == F.LAYERS
    assert r['definition'].startswith(evaluate.METRICS_DEFINITION) and 'conv5_4' in r['definition'] and 'not numerically comparable' in r['definition']
    assert r['n_nonfinite'] == 0
    assert json.loads(json.dumps(r, allow_nan=False)) == r


def test_summarise_counts_non_finite_extras_and_without_extras_is_unchanged():
    import evaluate
    ssim, psnr, mse, cos, l1 = _draws()
    base = evaluate.summarise_metrics(ssim, psnr, mse)
    assert sorted(base) == ['definition', 'mse', 'n_draws', 'n_nonfinite', 'n_samples', 'psnr', 'ssim']      # today's keys
    assert base['definition'] == evaluate.METRICS_DEFINITION and 'vgg' not in base['definition'].lower()
    assert evaluate.summarise_metrics(ssim, psnr, mse, extras=None) == base
    with_extras = evaluate.summarise_metrics(ssim, psnr, mse, extras={'vgg_cos': cos, 'vgg_l1': l1})
    for key in ('ssim', 'psnr', 'mse', 'n_samples', 'n_draws'):
        assert with_extras[key] == base[key]
    cos[0, 1, 3] = np.nan                                             # the draw that would have won sample 0
    l1[1, 2, 7] = np.inf
    psnr[0, 0, 0] = np.inf
    r = evaluate.summarise_metrics(ssim, psnr, mse, extras={'vgg_cos': cos, 'vgg_l1': l1})
    assert r['n_nonfinite'] == 3
    assert evaluate.summarise_metrics(ssim, psnr, mse)['n_nonfinite'] == 1
    assert r['vgg_cos']['best_draw'] == [2, 2]                        # a NaN mean never wins
    assert r['vgg_cos']['mean'] is None and r['vgg_cos']['per_frame'][3] is None
    assert r['vgg_l1']['best_draw'] == [2, 0]
    assert json.loads(json.dumps(r, allow_nan=False)) == r
    with pytest.raises(ValueError):
        evaluate.summarise_metrics(ssim, psnr, mse, extras={'vgg_cos': cos[:, :2], 'vgg_l1': l1})


def test_evaluate_vgg_metrics_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import yaml
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    cfg = yaml.safe_load(open(os.path.join(REPO, 'configs', 'penn.yaml')))
    cfg['paths']['vggnet'] = str(tmp_path / 'absent' / 'vgg19.npy')
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    base = ['--config', str(cfg_path), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck), '--save_dir', str(tmp_path / 'eval')]
    for extra in (['--vgg-metrics'], ['--vgg-metrics', '--synthetic-vgg'], ['--vgg-metrics', '--samples', '2']):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert '--vgg-metrics adds to the scores of --metrics' in capsys.readouterr().err, extra
    with pytest.raises(Exception) as e:                               # the text train.py raises
        evaluate.main(base + ['--metrics', '--vgg-metrics'])
    assert not isinstance(e.value, (ImportError, SystemExit))
    assert str(e.value) == ('file of pretrained vgg19 does not exist at: %s (pass --synthetic-vgg for benchmarking)' % cfg['paths']['vggnet'])
    assert not (tmp_path / 'eval').exists()


def test_feature_pair_metrics_entry_refuses_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    f = lib.kpx_feature_pair_metrics_f32
    a = 1 << 20                                                       # an aligned fake address: never touched
    for args in ((None, a, 1, 4, 4, 64, a, a), (a, None, 1, 4, 4, 64, a, a), (a, a, 1, 4, 4, 64, None, a), (a, a, 1, 4, 4, 64, a, None),
                 (a, a, 1, 4, 4, 6, a, a),                            # C % 4 != 0
                 (a, a, 1, 4, 4, 0, a, a), (a, a, 1, 4, 4, 516, a, a),   # C outside [4, 512]
                 (a, a, 1, 0, 4, 64, a, a), (a, a, 1, 4, 0, 64, a, a), (a, a, 1, 1025, 4, 64, a, a), (a, a, 1, 4, 1025, 64, a, a),
                 (a, a, 0, 4, 4, 64, a, a), (a, a, -1, 4, 4, 64, a, a),
                 (a + 4, a, 1, 4, 4, 64, a, a), (a, a + 8, 1, 4, 4, 64, a, a), (a, a, 1, 4, 4, 64, a + 4, a)):      # misaligned pointers
        assert f(*args, None) == -1, args
    q = lib.kpx_feature_pair_metrics_workspace_bytes
    assert q(1, 128, 128, 64) > 0 and q(3, 1, 1, 512) == 3 * q(1, 1, 1, 512)
    assert q(512, 16, 16, 512) == 512 * q(1, 16, 16, 512)             # the slab count never depends on N
    assert q(1, 4, 4, 6) == 0 and q(1, 0, 4, 64) == 0
    assert lib.kpx_vgg_prep_png8_f32(None, 16, a, None) == -1 and lib.kpx_vgg_prep_png8_f32(a, 16, None, None) == -1
