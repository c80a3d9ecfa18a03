"""CPU: evaluate.py --drive without a GPU -- summarise_drive on hand-made arrays (values, per-frame values, skill and its null cases), the
parser errors of the new flags, the degenerate inputs of the retargeting restatement (drive_ref.py) and the argument checks of
kpx_points_retarget_f32."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import drive_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _scores(ssim, psnr, mse):
    return {'ssim': np.asarray(ssim, np.float32), 'psnr': np.asarray(psnr, np.float32), 'mse': np.asarray(mse, np.float32)}


def test_summarise_drive_values_and_skill():
    import evaluate
    # S = 2 samples, T = 2 frames; the model's scores [S, N = 2, T]
    labels = _scores([[0.75, 0.5], [1.0, 0.75]], [[30, 20], [40, 30]], [[0.25, 0.5], [0.0, 0.25]])
    hold = _scores([[0.25, 0.25], [0.5, 0.0]], [[10, 10], [20, 0]], [[0.5, 1.0], [0.5, 1.0]])
    model = {'ssim': np.full((2, 2, 2), 0.5, np.float32), 'psnr': np.full((2, 2, 2), 25.0, np.float32), 'mse': np.full((2, 2, 2), 0.5, np.float32)}
    blk = evaluate.summarise_drive({'hold': hold, 'labels': labels}, model=model)
    assert blk['modes'] == ['labels', 'hold'] and blk['definition'] == evaluate.DRIVE_DEFINITION
    assert 'pseudo labels' in blk['definition'] and 'not human annotations' in blk['definition'] and 'detector' in blk['definition']
    assert blk['labels']['ssim'] == {'mean': 0.75, 'per_frame': [0.875, 0.625]}
    assert blk['labels']['psnr'] == {'mean': 30.0, 'per_frame': [35.0, 25.0]}
    assert blk['labels']['mse'] == {'mean': 0.25, 'per_frame': [0.125, 0.375]}
    assert blk['hold']['ssim'] == {'mean': 0.25, 'per_frame': [0.375, 0.125]}
    assert blk['hold']['psnr'] == {'mean': 10.0, 'per_frame': [15.0, 5.0]}
    assert blk['hold']['mse'] == {'mean': 0.75, 'per_frame': [0.5, 1.0]}
    # (model - hold) / (labels - hold) on the means: (0.5 - 0.25) / (0.75 - 0.25), (25 - 10) / (30 - 10), (0.5 - 0.75) / (0.25 - 0.75)
    assert blk['skill'] == {'ssim': 0.5, 'psnr': 0.75, 'mse': 0.5}
    assert set(blk) == {'definition', 'modes', 'labels', 'hold', 'skill'}
    json.dumps(blk, allow_nan=False)


def test_summarise_drive_skill_is_null_or_absent_where_it_has_no_meaning():
    import evaluate
    one = np.ones((2, 3), np.float32)
    model = {'ssim': np.full((2, 1, 3), 0.5), 'psnr': np.full((2, 1, 3), 20.0), 'mse': np.full((2, 1, 3), 0.5)}
    # a zero denominator (labels and hold score the same SSIM) and a NaN (in hold's MSE) and an infinity (labels' PSNR at MSE = 0)
    labels = _scores(one * 0.5, one * np.inf, one * 0.0)
    hold = _scores(one * 0.5, one * 10, np.where(np.arange(3) == 1, np.nan, 1.0) * one)
    blk = evaluate.summarise_drive({'labels': labels, 'hold': hold}, model=model)
    assert blk['skill'] == {'ssim': None, 'psnr': None, 'mse': None}
    assert blk['labels']['psnr']['mean'] is None and blk['hold']['mse']['mean'] is None
    assert blk['hold']['mse']['per_frame'] == [1.0, None, 1.0]
    json.dumps(blk, allow_nan=False)
    # a NaN in the model's own scores
    fine = _scores(one * 0.75, one * 30, one * 0.25)
    floor = _scores(one * 0.25, one * 10, one * 0.75)
    bad = dict(model, ssim=np.where(np.arange(3) == 2, np.nan, 0.5) * np.ones((2, 1, 3)))
    blk = evaluate.summarise_drive({'labels': fine, 'hold': floor}, model=bad)
    assert blk['skill']['ssim'] is None and blk['skill']['psnr'] == 0.5 and blk['skill']['mse'] == 0.5
    # a missing mode, or no model: no skill
    for kw in (dict(drive={'labels': fine}, model=model), dict(drive={'hold': floor}, model=model), dict(drive={'labels': fine, 'hold': floor})):
        blk = evaluate.summarise_drive(**kw)
        assert 'skill' not in blk and blk['modes'] == [m for m in ('labels', 'hold') if m in kw['drive']]
    # no sample at all
    empty = _scores(*(np.zeros((0, 3), np.float32),) * 3)
    blk = evaluate.summarise_drive({'labels': empty, 'hold': empty}, model={k: np.zeros((0, 1, 3)) for k in model})
    assert blk['labels']['ssim'] == {'mean': None, 'per_frame': [None] * 3} and blk['skill'] == {'ssim': None, 'psnr': None, 'mse': None}
    for bad_arg in ({}, {'transfer': fine}, {'labels': {'ssim': one}}, {'labels': fine, 'hold': _scores(one[:1], one[:1], one[:1])}):
        with pytest.raises(ValueError):
            evaluate.summarise_drive(bad_arg)


def test_evaluate_drive_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    stage1 = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--save_dir', str(tmp_path / 'eval')]
    both = stage1 + ['--checkpoint_stage2', str(ck)]
    for base, extra, text in ((both, ['--drive', 'labels,held'], "'held'"), (both, ['--drive', 'bogus'], 'labels, hold, transfer'),
                              (both, ['--drive', 'hold,labels,hold'], 'twice'), (both, ['--drive', ''], 'nothing'),
                              (both, ['--drive', 'labels', '--synthetic', '2'], '--synthetic'),
                              (both, ['--drive', 'hold,transfer', '--synthetic', '2'], '--synthetic'),
                              (both, ['--drive-only'], 'needs it'), (stage1, ['--drive-only'], 'needs it'),
                              (both, ['--drive', 'hold', '--drive-only', '--samples', '2'], '--samples'),
                              (both, ['--drive', 'hold', '--drive-only', '--actions', '1'], '--actions'),
                              (both, ['--drive', 'hold', '--drive-only', '--metrics', '--vgg-metrics'], '--vgg-metrics'),
                              (both, ['--drive', 'hold', '--drive-only', '--metrics', '--motion-metrics'], '--motion-metrics'),
                              (stage1, ['--drive', 'transfer', '--drive-only', '--metrics'], 'no ground truth'),
                              (both, ['--drive', 'labels,hold', '--drive-scaled'], 'transfer'),
                              (both, ['--drive-scaled'], 'transfer'),
                              (both, ['--drive', 'hold', '--sheet-frames', '7,3'], 'increasing'),
                              (both, ['--drive', 'hold', '--sheet-frames', '32'], 'in [0, 32)'),
                              (both, ['--sheet-frames', '3,7'], 'needs it'),
                              (stage1, [], '--checkpoint_stage2'), (stage1, ['--drive', 'labels,hold'], '--checkpoint_stage2'),
                              (stage1, ['--synthetic', '2'], '--checkpoint_stage2')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2, extra
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_reference_scale_at_the_degenerate_inputs():
    rs = np.random.RandomState(0)
    src = rs.uniform(-1, 1, (7, 2)).astype(np.float32)
    drv = rs.uniform(-1, 1, (7, 2)).astype(np.float32)
    s = D.scale(src, drv)
    assert np.isfinite(s) and s > 0 and s != 1.0
    assert abs(s - np.sqrt(((src - src.mean(0)).astype(np.float64) ** 2).sum() / ((drv - drv.mean(0)).astype(np.float64) ** 2).sum())) < 1e-6
    same = np.repeat(drv[:1], 7, axis=0)
    assert D.spread(same) == 0.0
    assert D.scale(src, same) == 1.0                                   # v_drv = 0
    assert D.scale(same, drv) == 1.0                                   # v_src = 0
    assert D.scale(src[:1], drv[:1]) == 1.0                            # K = 1: both spreads are 0
    for special in (np.nan, np.inf, -np.inf):                          # a non-finite spread, in the source or in the driver
        bad = drv.copy()
        bad[3, 1] = special
        assert not np.isfinite(D.spread(bad))
        assert D.scale(src, bad) == 1.0 and D.scale(bad, drv) == 1.0


def test_reference_retarget_modes():
    rs = np.random.RandomState(1)
    b, t, k = 3, 4, 5
    src, first = (rs.uniform(-1, 1, (b, k, 2)).astype(np.float32) for _ in range(2))
    seq = rs.uniform(-1, 1, (b, t, k, 2)).astype(np.float32)
    hold = D.retarget(src, 'hold', frames=t)
    assert hold.shape == (b, t, k, 2) and hold.dtype == np.float32 and all(np.array_equal(hold[:, i], src) for i in range(t))
    assert np.array_equal(D.retarget(src, 'absolute', first, seq), seq)
    assert np.array_equal(D.retarget(src, 'absolute', first, seq, shift=1), seq[[1, 2, 0]])
    rel = D.retarget(src, 'relative', first, seq, shift=2)
    want = src[:, None].astype(np.float64) + (seq[[2, 0, 1]].astype(np.float64) - first[[2, 0, 1]][:, None].astype(np.float64))
    assert np.array_equal(rel, want.astype(np.float32))
    # a driver that starts where the source stands moves it along the driver's own path
    assert np.allclose(D.retarget(first, 'relative', first, seq), seq, atol=2e-7)
    # scaled: a driver twice the size of the source moves it half as far
    big = D.retarget(src, 'relative', 2 * src, 2 * src[:, None] + 0.5, scaled=True)
    assert np.allclose(big, src[:, None] + 0.25, atol=5e-7)
    # non-finite values stay in the sample that reads them
    first_nan = first.copy()
    first_nan[1, 2, 0] = np.nan
    for scaled in (False, True):
        got, clean = D.retarget(src, 'relative', first_nan, seq, shift=1, scaled=scaled), D.retarget(src, 'relative', first, seq, shift=1, scaled=scaled)
        assert np.isnan(got[0, :, 2, 0]).all() and np.isfinite(np.delete(got[0].reshape(t, -1), 4, axis=1)).all()      # sample 0 reads driver 1
        assert np.array_equal(got[1:], clean[1:])


def test_points_retarget_entry_refuses_bad_arguments_without_a_gpu():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'kpx_points_retarget_f32') and 'kpx_points_retarget_f32' in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 15 and _lib.lib.kpx_abi_version() == _lib.ABI_VERSION
    a = 1 << 20                                                       # an aligned fake address: never touched

    def call(src=a, first=a, seq=a, b=2, t=32, k=15, shift=1, mode=3, out=a):
        return _lib.lib.kpx_points_retarget_f32(src, first, seq, b, t, k, shift, mode, out, None)

    bad = [dict(b=0), dict(t=0), dict(k=0), dict(k=1025), dict(shift=2), dict(shift=-1), dict(mode=4), dict(mode=-1), dict(out=None),
           dict(src=None), dict(first=None), dict(seq=None), dict(mode=2, first=None), dict(mode=1, seq=None), dict(mode=0, src=None),
           dict(src=a + 2), dict(first=a + 1), dict(seq=a + 3), dict(out=a + 2),
           dict(b=1 << 15, t=1 << 10, k=32, shift=0),                                    # B*T*K*2 = 2^31
           dict(b=1 << 30, t=1 << 30, k=1024, shift=0)]                                  # far past 2^63 / int overflow
    for kw in bad:
        assert call(**kw) == -1, kw
