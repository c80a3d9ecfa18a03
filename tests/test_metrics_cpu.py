"""CPU: the float64 frame-metric restatement (metrics_ref.py) against closed forms, evaluate.summarise_metrics (best of draws, ties,
per-frame curves, non-finite values, JSON round trip), evaluate.py's --metrics / --samples argument errors, and the argument checks of
kpx_frame_metrics_f32."""
import json
import os
import sys

import numpy as np
import pytest

import metrics_ref as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_separable_window_equals_tf_softmax_window():
    w = M.window_1d()
    assert abs(w.sum() - 1.0) <= 1e-15 and np.argmax(w) == 5
    assert np.abs(np.outer(w, w) - M.window_2d_tf()).max() <= 1e-15


def test_identical_frames_give_ssim_one_and_infinite_psnr():
    a = np.random.RandomState(0).uniform(0, 1, size=(3, 20, 17, 3))
    m = M.frame_metrics(a, a)
    assert np.abs(m[:, 0] - 1.0).max() <= 1e-14
    assert (m[:, 1] == 0).all() and np.isposinf(m[:, 2]).all()


@pytest.mark.parametrize('va,vb,L', [(0.3, 0.7, 1.0), (0.61, 0.611, 1.0), (12.0, 200.0, 255.0)])
def test_constant_frames_give_the_luminance_closed_form(va, vb, L):
    a = np.full((1, 15, 13, 1), va)
    b = np.full((1, 15, 13, 1), vb)
    c1 = (0.01 * L) ** 2
    m = M.frame_metrics(a, b, L)
    assert abs(m[0, 0] - (2 * va * vb + c1) / (va * va + vb * vb + c1)) <= 1e-12
    assert abs(m[0, 1] - (va - vb) ** 2) <= 1e-12 * (va - vb) ** 2
    assert abs(m[0, 2] - (20 * np.log10(L) - 10 * np.log10((va - vb) ** 2))) <= 1e-9


def test_psnr_of_a_known_mse():
    a = np.zeros((2, 16, 16, 3))
    b = a.copy()
    b[0] += 0.1                                                       # mse 0.01 -> 20 dB
    b[1, ::2] += 0.05
    b[1, 1::2] -= 0.05                                                # mse 0.0025 -> 26.0206 dB
    m = M.frame_metrics(a, b)
    assert abs(m[0, 1] - 0.01) <= 1e-15 and abs(m[0, 2] - 20.0) <= 1e-12
    assert abs(m[1, 1] - 0.0025) <= 1e-15 and abs(m[1, 2] - (-10 * np.log10(0.0025))) <= 1e-12
    assert abs(M.frame_metrics(a, b, 2.0)[0, 2] - (20 * np.log10(2.0) + 20.0)) <= 1e-12


def test_png8_is_the_bytes_save_img_writes():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.uniform(-1, 1, 100000), [-1.0, 1.0, 0.0, -0.99999994, 0.99999994]]).astype(np.float32)
    want = ((0.5 * (x + 1.0)) * 255).astype(np.uint8)                # evaluate._save_img(rescale=True), in range
    assert np.array_equal(M.png8(x), want)
    assert np.array_equal(M.png8(np.array([-1.5, 1.5, np.nan], np.float32)), np.array([0, 255, 0], np.uint8))


def _draws():
    s, n, t = 2, 3, 32
    ssim = np.full((s, n, t), 0.5)
    ssim[0, 1] = ssim[0, 2] = 0.7                                     # sample 0: draws 1 and 2 tie -> draw 1
    ssim[1, 2] = np.linspace(0.6, 0.9, t)                             # sample 1: draw 2, with a curve
    psnr = np.full((s, n, t), 20.0)
    psnr[0, 0] = 30.0
    psnr[1, 1] = 25.0
    mse = np.full((s, n, t), 0.01)
    mse[0, 2] = 0.001                                                 # lower is better
    mse[1, 0] = 0.002
    return ssim, psnr, mse


def test_summarise_picks_the_best_draw_per_metric_with_ties_to_the_lowest():
    import evaluate
    ssim, psnr, mse = _draws()
    r = evaluate.summarise_metrics(ssim, psnr, mse)
    assert (r['n_samples'], r['n_draws'], r['n_nonfinite']) == (2, 3, 0) and 'tf.image.ssim' in r['definition']
    assert r['ssim']['best_draw'] == [1, 2] and r['psnr']['best_draw'] == [0, 1] and r['mse']['best_draw'] == [2, 0]
    assert np.allclose(r['ssim']['per_frame'], ssim.mean(axis=(0, 1)), rtol=0, atol=1e-15)
    assert np.allclose(r['ssim']['best_of_draws_per_frame'], (ssim[0, 1] + ssim[1, 2]) / 2, rtol=0, atol=1e-15)
    assert abs(r['ssim']['best_of_draws'] - (0.7 + 0.75) / 2) <= 1e-15
    assert abs(r['mse']['best_of_draws'] - 0.0015) <= 1e-15
    for k in ('ssim', 'psnr'):
        assert r[k]['best_of_draws'] >= r[k]['mean'] and len(r[k]['per_frame']) == 32
    assert r['mse']['best_of_draws'] <= r['mse']['mean']
    assert json.loads(json.dumps(r, allow_nan=False)) == r


def test_summarise_counts_and_skips_non_finite_values():
    import evaluate
    ssim, psnr, mse = _draws()
    psnr[0, 0, 5] = np.nan                                            # the draw that would have won sample 0
    psnr[1, 0, :] = np.inf                                            # identical frames: a legitimate best
    r = evaluate.summarise_metrics(ssim, psnr, mse)
    assert r['n_nonfinite'] == 1 + 32
    assert r['psnr']['best_draw'] == [1, 0]                           # NaN mean never wins; ties among the rest -> draw 1
    assert r['psnr']['mean'] is None and r['psnr']['per_frame'][5] is None and r['psnr']['best_of_draws'] is None
    assert r['ssim']['mean'] is not None
    assert json.loads(json.dumps(r, allow_nan=False)) == r


def test_evaluate_metrics_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval')]
    for extra, text in ((['--metrics', '--synthetic', '2'], 'no ground truth'), (['--metrics', '--samples', '0'], '--samples must be >= 1'),
                        (['--samples', '-1'], '--samples must be >= 1')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_frame_metrics_entry_refuses_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                       # an aligned fake address: never touched
    for args in ((None, a, 1, 16, 16, 3, 1.0, 0, a), (a, a, 0, 16, 16, 3, 1.0, 0, a), (a, a, 1, 10, 16, 3, 1.0, 0, a),
                 (a, a, 1, 16, 1025, 3, 1.0, 0, a), (a, a, 1, 16, 16, 2, 1.0, 0, a), (a, a, 1, 16, 16, 3, 0.0, 0, a),
                 (a, a, 1, 16, 16, 3, -1.0, 0, a), (a, a, 1, 16, 16, 3, float('inf'), 0, a), (a, a, 1, 16, 16, 3, 1.0, 2, a),
                 (a, a, 1, 16, 16, 3, 1.0, 0, None)):
        assert lib.kpx_frame_metrics_f32(*args, None) == -1, args
