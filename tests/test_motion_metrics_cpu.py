"""CPU: the integer restatement of the draw diversity (motion_metrics_ref.py) against the sum over pairs and at its largest arguments,
evaluate.summarise_metrics(motion=...) (key sets, lowest draw and ties for kp_l2, nulls, motion=None unchanged), evaluate.py's
--motion-metrics argument errors, and the exports and argument checks of the three kpx_*draw* entries."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import motion_metrics_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('d', [2, 3, 5, 8])
def test_moment_identity_equals_the_sum_over_pairs(d):
    rs = np.random.RandomState(d)
    q = rs.randint(0, 256, size=(d, 2, 5, 7, 3)).astype(np.uint8)
    q[:, 0, 0, :2] = 0
    q[: d // 2, 0, 0, 1] = 255                                        # the extremes, and a value no draw changes
    q[:, 0, 0, 2] = 77
    qi = q.astype(np.int64)
    v = R.pair_sums(qi.sum(axis=0), (qi * qi).sum(axis=0), d)
    assert v.dtype == np.int64 and np.array_equal(v, R.pair_sums_brute_force(q)) and (v >= 0).all()
    assert (v[0, 0, 0] == 0).all() and (v[0, 0, 2] == 0).all() and (v[0, 0, 1] == (d // 2) * (d - d // 2) * 65025).all()
    # through the quantisation: draws in [-1,1] whose bytes are q
    x = (q.astype(np.float64) + 0.5) / 255.0 * 2 - 1
    s, ss = R.moments(x.astype(np.float32))
    assert np.array_equal(s, qi.sum(axis=0)) and np.array_equal(ss, (qi * qi).sum(axis=0))
    div_mse, std_map = R.draw_diversity(s, ss, d, (5, 7, 3))
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    want = np.mean([((qi[i] - qi[j]) ** 2).reshape(2, -1).mean(axis=1) / 65025.0 for i, j in pairs], axis=0)
    assert np.abs(div_mse.astype(np.float64) - want).max() <= 1e-7 * want.max()
    var = qi.astype(np.float64).var(axis=0).mean(axis=-1)             # population variance over draws, mean over channels
    assert np.abs(std_map.astype(np.float64) - np.minimum(255, np.floor(2 * np.sqrt(var)))).max() <= 1   # (floor of a float estimate)
    assert std_map.dtype == np.uint8 and std_map.shape == (2, 5, 7)


def test_largest_arguments_stay_inside_int64_and_uint32():
    d = R.MAX_DRAWS
    s = np.array([255 * d, 255 * d // 2, 0], np.int64)               # all 255, half 0 / half 255, all 0
    ss = np.array([65025 * d, 65025 * d // 2, 0], np.int64)
    assert ss.max() < 2 ** 32 and s.max() < 2 ** 32                   # the uint32 accumulators
    assert d * int(ss.max()) >= 2 ** 32                               # ... whose product with D needs 64 bits
    v = R.pair_sums(s, ss, d)
    assert [int(x) for x in v] == [0, d * d * 65025 // 4, 0]
    worst_frame = int(v[1]) * 1024 * 1024 * 3                        # every value of the largest frame at the largest V
    assert worst_frame < 2 ** 63 and 4 * 3 * int(v[1]) < 2 ** 63
    # 0 / 255 halves: mean pairwise MSE = (D/2)^2 / (D (D - 1) / 2) and a spread of 255
    acc_s = np.full((2 * 2 * 3,), s[1], np.int64)
    acc_ss = np.full((2 * 2 * 3,), ss[1], np.int64)
    div_mse, std_map = R.draw_diversity(acc_s, acc_ss, d, (2, 2, 3))
    assert div_mse[0] == np.float32((d / 2) ** 2 / (d * (d - 1) / 2)) and (std_map == 255).all()
    div_mse, std_map = R.draw_diversity(np.array([255, 255]), np.array([65025, 65025]), 2, (1, 2, 1))  # all 0 against all 255
    assert div_mse[0] == 1.0 and (std_map == 255).all()


def test_integer_square_root_of_the_restatement_is_math_isqrt():
    from math import isqrt
    rs = np.random.RandomState(9)
    roots = np.concatenate([np.arange(0, 300), rs.randint(0, 2 ** 30, size=200)]).astype(np.int64)
    m = np.concatenate([roots * roots, roots * roots + 1, np.maximum(roots * roots - 1, 0), rs.randint(0, 65026, size=1000)])
    assert [int(x) for x in R.isqrt_array(m)] == [isqrt(int(x)) for x in m]


def test_keypoint_restatement_on_a_case_worked_by_hand():
    pts = np.zeros((2, 1, 1, 2, 2), np.float32)
    pts[0, 0, 0] = [[3, 4], [0, 0]]                                  # draw 0: distances 5 and 0 from the labels at the origin
    pts[1, 0, 0] = [[0, 0], [6, 8]]                                  # draw 1: 0 and 10
    l2, div = R.keypoint_draw_metrics(pts, np.zeros((1, 1, 2, 2), np.float32))
    assert l2.tolist() == [[[2.5]], [[5.0]]] and div.tolist() == [[7.5]]
    l2, div = R.keypoint_draw_metrics(pts[:1], np.zeros((1, 1, 2, 2), np.float32))
    assert div is None and l2.tolist() == [[[2.5]]]
    assert R.within_one_ulp(np.float32([1.0, np.inf, np.nan]), [1.0 + 5e-8, np.inf, np.nan])
    assert not R.within_one_ulp(np.float32([1.0]), [1.0 + 3e-7]) and not R.within_one_ulp(np.float32([1.0]), [np.nan])


def _scores():
    s, n, t = 2, 3, 32
    rs = np.random.RandomState(0)
    ssim, psnr, mse = rs.uniform(0.2, 0.9, (s, n, t)), rs.uniform(15, 30, (s, n, t)), rs.uniform(1e-3, 1e-2, (s, n, t))
    kp_l2 = np.full((s, n, t), 0.5)
    kp_l2[0, 1] = kp_l2[0, 2] = 0.2                                   # sample 0: draws 1 and 2 tie -> draw 1
    kp_l2[1, 2] = np.linspace(0.1, 0.4, t)                            # sample 1: draw 2, with a curve
    kp_div = rs.uniform(0.0, 0.3, (s, t))
    div_mse = rs.uniform(0.0, 0.01, (s, t))
    return (ssim, psnr, mse), kp_l2, kp_div, div_mse


def test_summarise_motion_blocks_key_sets_and_lowest_draw():
    import evaluate
    three, kp_l2, kp_div, div_mse = _scores()
    base = evaluate.summarise_metrics(*three)
    assert evaluate.summarise_metrics(*three, motion=None) == base and evaluate.summarise_metrics(*three, extras=None, motion=None) == base
    r = evaluate.summarise_metrics(*three, motion={'kp_l2': kp_l2, 'kp_div': kp_div, 'div_mse': div_mse})
    assert set(r) == set(base) | {'kp_l2', 'kp_div', 'div_mse'}
    for key in ('ssim', 'psnr', 'mse', 'n_samples', 'n_draws', 'n_nonfinite'):
        assert r[key] == base[key]
    assert r['definition'] == base['definition'] + ' ' + evaluate.MOTION_METRICS_DEFINITION
    assert set(r['kp_l2']) == set(base['ssim'])                       # the same form as ssim
    assert r['kp_l2']['best_draw'] == [1, 2]                          # lowest mean, the tie to the lowest draw
    assert abs(r['kp_l2']['best_of_draws'] - (0.2 + 0.25) / 2) <= 1e-15 and r['kp_l2']['best_of_draws'] <= r['kp_l2']['mean']
    assert np.allclose(r['kp_l2']['best_of_draws_per_frame'], (kp_l2[0, 1] + kp_l2[1, 2]) / 2, rtol=0, atol=1e-15)
    assert np.allclose(r['kp_l2']['per_frame'], kp_l2.mean(axis=(0, 1)), rtol=0, atol=1e-15)
    for key, x in (('kp_div', kp_div), ('div_mse', div_mse)):
        assert set(r[key]) == {'mean', 'per_frame'} and len(r[key]['per_frame']) == 32
        assert abs(r[key]['mean'] - x.mean()) <= 1e-15 and np.allclose(r[key]['per_frame'], x.mean(axis=0), rtol=0, atol=1e-15)
    assert json.loads(json.dumps(r, allow_nan=False)) == r
    one = evaluate.summarise_metrics(*(x[:, :1] for x in three), motion={'kp_l2': kp_l2[:, :1]})     # --samples 1: kp_l2 alone
    assert set(one) == set(base) | {'kp_l2'} and one['kp_l2']['best_draw'] == [0, 0]
    # the VGG pair keeps its meaning beside it
    both = evaluate.summarise_metrics(*three, extras={'vgg_cos': three[0], 'vgg_l1': three[2]}, motion={'kp_l2': kp_l2})
    assert set(both) == set(base) | {'vgg_layers', 'vgg_cos', 'vgg_l1', 'kp_l2'}
    assert both['definition'] == base['definition'] + ' ' + evaluate.VGG_METRICS_DEFINITION + ' ' + evaluate.MOTION_METRICS_DEFINITION


def test_summarise_motion_counts_non_finite_kp_l2_and_nulls_the_rest():
    import evaluate
    three, kp_l2, kp_div, div_mse = _scores()
    kp_l2[0, 1, 5] = np.nan                                           # the draw that would have won sample 0
    kp_l2[1, 0, 3] = np.inf
    kp_div[1, 7] = np.nan
    r = evaluate.summarise_metrics(*three, motion={'kp_l2': kp_l2, 'kp_div': kp_div, 'div_mse': div_mse})
    assert r['n_nonfinite'] == 2
    assert r['kp_l2']['best_draw'] == [2, 2] and r['kp_l2']['mean'] is None and r['kp_l2']['per_frame'][5] is None
    assert r['kp_l2']['per_frame'][3] is None and r['kp_l2']['per_frame'][4] is not None
    assert r['kp_div']['mean'] is None and r['kp_div']['per_frame'][7] is None and r['kp_div']['per_frame'][6] is not None
    assert r['div_mse']['mean'] is not None and r['ssim']['mean'] is not None
    assert json.loads(json.dumps(r, allow_nan=False)) == r
    for bad in ({'kp_div': kp_div}, {'kp_l2': kp_l2, 'other': kp_div}, {'kp_l2': kp_l2[:, :2]}, {'kp_l2': kp_l2, 'kp_div': kp_div[:, :5]}):
        with pytest.raises(ValueError):
            evaluate.summarise_metrics(*three, motion=bad)


def test_evaluate_motion_metrics_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval')]
    for extra, text in ((['--motion-metrics'], 'needs it'), (['--motion-metrics', '--samples', '3'], 'needs it'),
                        (['--metrics', '--motion-metrics', '--samples', '4097'], 'at most 4096'),
                        (['--metrics', '--motion-metrics', '--synthetic', '2'], 'no ground truth')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_library_exports_the_three_entries_and_refuses_bad_arguments_without_a_gpu():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('kpx_draw_moments_add_f32', 'kpx_draw_diversity_f32', 'kpx_keypoint_draw_metrics_f32'):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 13
    lib = _lib.lib
    a = 1 << 20                                                       # an aligned fake address: never touched
    add = lib.kpx_draw_moments_add_f32
    for args in ((None, 16, a, a), (a, 16, None, a), (a, 16, a, None), (a + 2, 16, a, a), (a, 16, a + 1, a), (a, 16, a, a + 2)):
        assert add(*args, None) == -1, args
    assert add(a, 0, a, a, None) == 0                                 # nothing to do: no launch
    div = lib.kpx_draw_diversity_f32
    for args in ((None, a, 1, 4, 4, 3, 2, a, None), (a, None, 1, 4, 4, 3, 2, a, None), (a, a, 1, 4, 4, 3, 2, None, a),
                 (a, a, 0, 4, 4, 3, 2, a, None), (a, a, 1, 0, 4, 3, 2, a, None), (a, a, 1, 1025, 4, 3, 2, a, None),
                 (a, a, 1, 4, 0, 3, 2, a, None), (a, a, 1, 4, 1025, 3, 2, a, None), (a, a, 1, 4, 4, 2, 2, a, None),
                 (a, a, 1, 4, 4, 0, 2, a, None), (a, a, 1, 4, 4, 4, 2, a, None), (a, a, 1, 4, 4, 3, 1, a, None),
                 (a, a, 1, 4, 4, 3, 0, a, None), (a, a, 1, 4, 4, 3, 4097, a, None), (a, a, 1, 4, 4, 3, -2, a, a)):
        assert div(*args, None) == -1, args
    kp = lib.kpx_keypoint_draw_metrics_f32
    for args in ((None, a, 2, 1, 32, 15, a, a), (a, None, 2, 1, 32, 15, a, a), (a, a, 2, 1, 32, 15, None, a),
                 (a, a, 0, 1, 32, 15, a, None), (a, a, 4097, 1, 32, 15, a, a), (a, a, 2, 0, 32, 15, a, a), (a, a, 2, 1, 0, 15, a, a),
                 (a, a, 2, 1, 32, 0, a, a), (a, a, 1, 1, 32, 15, a, a)):                       # the last: D == 1 with a diversity output
        assert kp(*args, None) == -1, args
