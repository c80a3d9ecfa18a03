"""CPU: evaluate.py --frechet without a device -- kpx_amd.frechet.frechet_distance against closed forms, the statistics of the accumulator
(from moments computed on the host), summarise_frechet, the parser errors and the argument checks of the two ABI 16 entries."""
import json
import os
import sys

import numpy as np
import pytest

import frechet_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frechet():
    from kpx_amd import frechet
    return frechet


def _orthogonal(rs, d):
    q, _ = np.linalg.qr(rs.normal(size=(d, d)))
    return q


def _sample_stats(rs, n, d, shift=0.0):
    x = np.maximum(0, rs.normal(size=(n, d))) + shift
    return x, x.mean(axis=0), np.cov(x, rowvar=False)


# ------------------------------------------------------------------------------------------------ frechet_distance: closed forms
@pytest.mark.parametrize('d', [3, 64, 300])
def test_commuting_covariances_give_the_closed_form(d):
    rs = np.random.RandomState(d)
    q = _orthogonal(rs, d)
    a, b = rs.uniform(0.1, 4.0, size=d), rs.uniform(0.1, 4.0, size=d)
    m1, m2 = rs.normal(size=d), rs.normal(size=d)
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    got = _frechet().frechet_distance(m1, (q * a) @ q.T, m2, (q * b) @ q.T)
    print('D = %d: rel err %.3e' % (d, abs(got - want) / want))
    assert abs(got - want) <= 1e-12 * want
    assert abs(R.distance(m1, (q * a) @ q.T, m2, (q * b) @ q.T) - want) <= 1e-12 * want      # the restatement too


@pytest.mark.parametrize('n,d', [(500, 16), (200, 64), (96, 512), (96, 1024)])
def test_swapping_the_arguments_agrees(n, d):
    rs = np.random.RandomState(n + d)
    _, m1, c1 = _sample_stats(rs, n, d)
    _, m2, c2 = _sample_stats(rs, n, d, shift=0.3)
    f = _frechet().frechet_distance
    ab, ba = f(m1, c1, m2, c2), f(m2, c2, m1, c1)
    print('n = %d, D = %d: %.6e vs %.6e, rel %.3e' % (n, d, ab, ba, abs(ab - ba) / abs(ab)))
    assert abs(ab - ba) <= 1e-8 * abs(ab)


def test_scaling_both_sets_scales_the_distance_by_the_square():
    rs = np.random.RandomState(5)
    _, m1, c1 = _sample_stats(rs, 300, 32)
    _, m2, c2 = _sample_stats(rs, 300, 32, shift=0.5)
    f = _frechet().frechet_distance
    base = f(m1, c1, m2, c2)
    for s in (2.0, 0.125, 3.7, 1e3):
        got = f(s * m1, s * s * c1, s * m2, s * s * c2)
        assert abs(got - s * s * base) <= 1e-9 * s * s * base, (s, got, base)


@pytest.mark.parametrize('n,d', [(400, 16), (96, 64), (96, 512), (96, 1024)])
def test_identical_statistics_give_zero_within_rounding_and_are_not_clamped(n, d):
    rs = np.random.RandomState(3 * n + d)
    _, m, c = _sample_stats(rs, n, d)
    got = _frechet().frechet_distance(m, c, m.copy(), c.copy())
    print('n = %d, D = %d: FD / tr C = %.3e' % (n, d, got / np.trace(c)))
    assert abs(got) <= 1e-6 * np.trace(c)


# ------------------------------------------------------------------------------------------------ statistics
def _host_accumulator(rows_per_layer, video_rows_per_layer):
    """an accumulator on the CPU device filled with moments computed here in float64 (the device path is ops.moments_add)"""
    F = _frechet()
    acc = F.FrechetAccumulator([r.shape[1] for r in rows_per_layer], 'cpu')
    for layer, (fr, vr) in enumerate(zip(rows_per_layer, video_rows_per_layer)):
        for level, x in (('frame', fr), ('video', vr)):
            acc.add_moments(level, layer, x.shape[0], x.sum(axis=0), x.T @ x)
    return acc


def test_stats_match_numpy_cov_and_merge_is_additive():
    rs = np.random.RandomState(11)
    frames = [np.maximum(0, rs.normal(size=(64, c))) + 5.0 for c in (4, 12)]
    videos = [rs.normal(size=(8, 2 * c)) for c in (4, 12)]
    whole = _host_accumulator(frames, videos).stats()
    for layer in range(2):
        for level, x in (('frame', frames[layer]), ('video', videos[layer])):
            s = whole[level][layer]
            assert s['n'] == x.shape[0] and s['mean'].dtype == np.float64 and s['cov'].dtype == np.float64
            assert np.abs(s['mean'] - x.mean(axis=0)).max() <= 1e-13 * np.abs(x).max()
            want = np.cov(x, rowvar=False)
            assert np.abs(s['cov'] - want).max() <= 1e-10 * np.abs(want).max()
            ref = R.stats(x)
            assert np.abs(s['cov'] - ref['cov']).max() <= 1e-10 * np.abs(want).max()
    a = _host_accumulator([f[:40] for f in frames], [v[:3] for v in videos])
    b = _host_accumulator([f[40:] for f in frames], [v[3:] for v in videos])
    merged = a.merge(b).stats()
    for level in ('frame', 'video'):
        for s, t in zip(merged[level], whole[level]):
            assert s['n'] == t['n']
            assert np.abs(s['mean'] - t['mean']).max() <= 1e-12 * np.abs(t['mean']).max()
            assert np.abs(s['cov'] - t['cov']).max() <= 1e-12 * np.abs(t['cov']).max()
    with pytest.raises(ValueError):
        a.merge(_frechet().FrechetAccumulator([4, 16], 'cpu'))


def test_a_single_row_has_no_covariance_and_a_nan_distance():
    F = _frechet()
    rs = np.random.RandomState(2)
    one = _host_accumulator([rs.normal(size=(1, 8))], [rs.normal(size=(1, 16))]).stats()
    many = _host_accumulator([rs.normal(size=(9, 8))], [rs.normal(size=(3, 16))]).stats()
    empty = F.FrechetAccumulator([8], 'cpu').stats()
    assert one['frame'][0]['n'] == 1 and one['frame'][0]['cov'] is None and one['frame'][0]['mean'].shape == (8,)
    assert empty['frame'][0]['n'] == 0 and empty['frame'][0]['cov'] is None and empty['frame'][0]['mean'] is None
    assert np.isnan(F.frechet_distance(one['frame'][0]['mean'], one['frame'][0]['cov'], many['frame'][0]['mean'], many['frame'][0]['cov']))
    assert np.isnan(F.layer_distances(one, many, 'video')).all() and np.isnan(F.layer_distances(many, empty, 'frame')).all()
    assert np.isfinite(F.layer_distances(many, many, 'frame')).all()


def test_stats_survive_the_npz_round_trip(tmp_path):
    F = _frechet()
    rs = np.random.RandomState(4)
    acc = _host_accumulator([rs.normal(size=(5, 4)), rs.normal(size=(5, 8))], [rs.normal(size=(1, 8)), rs.normal(size=(1, 16))]).stats()
    np.savez(str(tmp_path / 'f.npz'), layers=np.array(['a', 'b']), **F.stats_arrays('pred', acc, ['a', 'b']))
    back = F.stats_from_arrays(np.load(str(tmp_path / 'f.npz')), 'pred', ['a', 'b'])
    for level in F.LEVELS:
        for s, t in zip(acc[level], back[level]):
            assert s['n'] == t['n'] and np.array_equal(s['mean'], t['mean'])
            assert (s['cov'] is None and t['cov'] is None) or np.array_equal(s['cov'], t['cov'])
    assert F.main([str(tmp_path / 'f.npz'), str(tmp_path / 'f.npz')]) == 0           # python -m kpx_amd.frechet a.npz b.npz


# ------------------------------------------------------------------------------------------------ the summary
def test_summarise_frechet_keys_headline_and_rank_deficiency():
    import evaluate
    rs = np.random.RandomState(8)
    dims = [4, 8, 16, 32, 32]

    def some(n_frames, n_videos, shift):
        return _host_accumulator([np.maximum(0, rs.normal(size=(n_frames, c))) + shift for c in dims],
                                 [rs.normal(size=(n_videos, 2 * c)) + shift for c in dims]).stats()
    stats = {'real': some(24, 3, 0.0), 'pred': some(48, 6, 0.2), 'pred_draw0': some(24, 3, 0.2), 'real_even': some(16, 2, 0.0),
             'real_odd': some(8, 1, 0.0)}
    arrays, block = evaluate.summarise_frechet(stats)
    names = ['vgg_fd_draw0_layers', 'vgg_fd_floor_layers', 'vgg_fd_layers', 'vgg_fvd_floor_layers', 'vgg_fvd_layers']
    assert sorted(arrays) == names and all(a.shape == (5,) and a.dtype == np.float64 for a in arrays.values())
    assert sorted(block) == sorted(names + ['definition', 'dims', 'n_pred', 'n_pred_videos', 'n_real', 'n_real_videos', 'rank_deficient',
                                            'vgg_fd', 'vgg_fvd', 'vgg_layers'])
    assert block['vgg_fd'] == float(arrays['vgg_fd_layers'][4]) and block['vgg_fvd'] == float(arrays['vgg_fvd_layers'][4])
    assert (block['n_real'], block['n_pred'], block['n_real_videos'], block['n_pred_videos']) == (24, 48, 3, 6)
    assert block['dims'] == {'frame': dims, 'video': [2 * c for c in dims]}
    assert block['rank_deficient'] == {'frame': [c >= 24 for c in dims], 'video': [True] * 5}          # n <= D
    assert np.isnan(arrays['vgg_fvd_floor_layers']).all() and block['vgg_fvd_floor_layers'] == [None] * 5   # one odd video: no covariance
    assert np.isfinite(arrays['vgg_fd_floor_layers']).all() and np.isfinite(arrays['vgg_fd_layers']).all()
    for layer in range(5):
        p, r = stats['pred']['frame'][layer], stats['real']['frame'][layer]
        want = R.distance(p['mean'], p['cov'], r['mean'], r['cov'])
        assert abs(arrays['vgg_fd_layers'][layer] - want) <= 1e-9 * abs(want)
    assert 'not FID/FVD' in block['definition'] and block['definition'] == evaluate.FRECHET_DEFINITION
    assert json.loads(json.dumps(block, allow_nan=False)) == block


# ------------------------------------------------------------------------------------------------ the parser
def test_evaluate_frechet_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import yaml
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    cfg = yaml.safe_load(open(os.path.join(REPO, 'configs', 'penn.yaml')))
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    base = ['--config', str(cfg_path), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck), '--save_dir', str(tmp_path / 'eval')]
    for extra in (['--frechet'], ['--frechet', '--metrics'], ['--frechet', '--metrics', '--synthetic-vgg']):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert '--frechet adds to the features of --metrics --vgg-metrics and needs both' in capsys.readouterr().err, extra
    with pytest.raises(SystemExit) as e:
        evaluate.main(base + ['--frechet', '--drive', 'hold', '--drive-only'])
    assert e.value.code == 2
    assert "--drive-only skips the model's own rollout, which --frechet is about" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(base + ['--metrics', '--vgg-metrics', '--frechet', '--drive', 'hold', '--drive-only'])
    assert e.value.code == 2
    assert not (tmp_path / 'eval').exists()


# ------------------------------------------------------------------------------------------------ the ABI
def test_abi_16_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION >= 16 and lib.kpx_abi_version() == _lib.ABI_VERSION
    a = 1 << 20                                                       # an aligned fake address: never touched
    pool = lib.kpx_feature_pool_f64
    for args in ((None, 1, 4, 4, 64, a, a), (a, 1, 4, 4, 64, None, a), (a, 1, 4, 4, 64, a, None),
                 (a + 4, 1, 4, 4, 64, a, a), (a + 8, 1, 4, 4, 64, a, a), (a, 1, 4, 4, 64, a + 4, a), (a, 1, 4, 4, 64, a, a + 4),   # misaligned
                 (a, 1, 4, 4, 6, a, a),                               # C % 4 != 0
                 (a, 1, 4, 4, 0, a, a), (a, 1, 4, 4, 516, a, a),      # C outside [4, 512]
                 (a, 1, 0, 4, 64, a, a), (a, 1, 4, 0, 64, a, a), (a, 1, 1025, 4, 64, a, a), (a, 1, 4, 1025, 64, a, a),
                 (a, 0, 4, 4, 64, a, a), (a, -1, 4, 4, 64, a, a)):
        assert pool(*args, None) == -1, args
    q = lib.kpx_feature_pool_workspace_bytes
    assert q(1, 128, 128, 64) > 0 and q(3, 1, 1, 512) == 3 * q(1, 1, 1, 512)
    assert q(512, 16, 16, 512) == 512 * q(1, 16, 16, 512)             # the slab count never depends on N
    assert q(1, 4, 4, 6) == 0 and q(1, 4, 4, 516) == 0 and q(1, 0, 4, 64) == 0 and q(0, 4, 4, 64) == 0
    add = lib.kpx_moments_add_f64
    for args in ((None, 4, 8, a, a), (a, 4, 8, None, a), (a, 4, 8, a, None),
                 (a + 4, 4, 8, a, a), (a, 4, 8, a + 4, a), (a, 4, 8, a, a + 2),                         # misaligned
                 (a, 4, 0, a, a), (a, 4, 1025, a, a), (a, 4, -1, a, a),                                  # D outside [1, 1024]
                 (a, 0, 8, a, a), (a, -3, 8, a, a), (a, (1 << 20) + 1, 8, a, a)):                        # M outside [1, 2^20]
        assert add(*args, None) == -1, args


def test_ops_refuse_cpu_tensors():
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    with pytest.raises(KpxError):
        ops.feature_pool(torch.zeros(1, 2, 2, 4))
    with pytest.raises(KpxError):
        ops.moments_add(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(KpxError):
        _frechet().FrechetAccumulator([4], 'cpu').add([torch.zeros(2, 2, 2, 4)], 2)
