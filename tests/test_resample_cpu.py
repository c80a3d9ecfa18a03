"""CPU: the definition of the key-point resampler on its restatement (tests/resample_ref.py: identity, knots, straight lines, parabolas,
non-finite containment), the refusals of kpx_amd.resample's wrappers and of the two C entries, and FinalModel.run's argument rules -- none
of which needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import resample_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _knots(b, n, k, seed=0):
    rs = np.random.RandomState(seed)
    return rs.uniform(-1, 1, (b, k, 2)).astype(np.float32), rs.uniform(-1, 1, (b, n, k, 2)).astype(np.float32)


def test_constants_mirror_the_header():
    from kpx_amd import ops, resample, tool_ops
    src = open(os.path.join(REPO, 'include', 'kpx.h')).read()
    val = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, src).group(1))
    assert resample.RESAMPLE_MAX_POINTS == val('KPX_RESAMPLE_MAX_POINTS') == 1024 and resample.RESAMPLE_MAX_RATE == val('KPX_RESAMPLE_MAX_RATE') == 64
    assert re.search(r'enum \{ KPX_RESAMPLE_LINEAR = 0, KPX_RESAMPLE_CUBIC = 1 \};', src)
    assert resample.RESAMPLE_MODES == {'linear': R.LINEAR, 'cubic': R.CUBIC} == {'linear': 0, 'cubic': 1}
    assert ops.points_resample is tool_ops.points_resample is resample.points_resample
    assert ops.points_speed is tool_ops.points_speed is resample.points_speed
    assert 'points_resample' not in tool_ops.__all__ and 'points_speed' not in tool_ops.__all__
    assert 'NOTHING IS CLAMPED' in src                              # the header says that a cubic may leave [-1, 1]


@pytest.mark.parametrize('mode', [R.LINEAR, R.CUBIC])
def test_rate_one_is_the_identity_and_knots_survive_bit_for_bit(mode):
    first, seq = _knots(2, 5, 3)
    seq[1, 2, 0, 1] = np.float32(np.inf)
    seq.view(np.uint32)[0, 3, 1, 0] = 0x7fc12345                    # a NaN with a payload
    seq[0, 0, 0, 0] = np.float32(-0.0)
    assert R.resample(first, seq, 1, mode).tobytes() == seq.tobytes()
    for rate in (2, 3, 64):
        out = R.resample(first, seq, rate, mode)
        assert out.shape == (2, 5 * rate, 3, 2) and out.dtype == np.float32
        assert out[:, rate - 1::rate].tobytes() == seq.tobytes()


@pytest.mark.parametrize('mode,n', [(R.LINEAR, 1), (R.LINEAR, 2), (R.LINEAR, 3), (R.LINEAR, 32), (R.CUBIC, 2), (R.CUBIC, 3), (R.CUBIC, 32)])
def test_a_straight_line_is_reproduced_at_every_frame(mode, n):
    rs = np.random.RandomState(n)
    for rate in (2, 3, 5, 64):
        p0 = rs.uniform(-0.5, 0.5, (2, 1, 4, 2))
        v = rs.uniform(-0.5, 0.5, (2, 1, 4, 2)) / n
        # knots exactly on a line in fp32: multiples of 2^-12 with |value| <= 1 are exact, and so is every frame time j / rate ... only for
        # rates that are powers of two; for the others the exact value is rounded to fp32 once, and the result may differ by one ulp
        p0, v = np.round(p0 * 4096) / 4096, np.round(v * 4096) / 4096
        t = np.arange(0, n + 1).reshape(1, -1, 1, 1)
        knots = (p0 + v * t).astype(np.float32)
        assert (knots.astype(np.float64) == p0 + v * t).all()
        out = R.resample(knots[:, 0], knots[:, 1:], rate, mode)
        tj = (np.arange(1, n * rate + 1) / np.float64(rate)).reshape(1, -1, 1, 1)
        want = (p0 + v * tj).astype(np.float32)
        assert R.ulp_distance(out, want).max() <= 1, (mode, n, rate)


def test_cubic_reproduces_a_parabola_on_the_interior_intervals():
    n, rate = 8, 4
    t = np.arange(0, n + 1, dtype=np.float64).reshape(1, -1, 1, 1)
    a, b, c = 1.0 / 128, -3.0 / 64, 1.0 / 4                          # exact in fp32 at every knot and every quarter step
    para = lambda x: a * x * x + b * x + c
    knots = para(t).astype(np.float32) * np.ones((1, 1, 2, 2), np.float32)
    assert (knots.astype(np.float64)[..., 0, 0] == para(t)[..., 0, 0]).all()
    out = R.resample(knots[:, 0], knots[:, 1:], rate, R.CUBIC)
    tj = (np.arange(1, n * rate + 1) / np.float64(rate)).reshape(1, -1, 1, 1)
    want = (para(tj) * np.ones((1, 1, 2, 2))).astype(np.float32)
    inner = (tj[0, :, 0, 0] >= 1) & (tj[0, :, 0, 0] <= n - 1)         # intervals whose two tangents are central differences
    assert R.ulp_distance(out[:, inner], want[:, inner]).max() <= 1
    assert R.ulp_distance(out[:, ~inner], want[:, ~inner]).max() > 1   # the one-sided ends do not (they reproduce lines)
    lin = R.resample(knots[:, 0], knots[:, 1:], rate, R.LINEAR)
    assert R.ulp_distance(lin[:, inner], want[:, inner]).max() > 1     # and LINEAR does not either


@pytest.mark.parametrize('mode', [R.LINEAR, R.CUBIC])
@pytest.mark.parametrize('knot', [0, 1, 3, 6])
def test_a_nan_knot_reaches_exactly_the_frames_of_its_stencil(mode, knot):
    n, rate, k = 6, 3, 4
    first, seq = _knots(2, n, k, seed=knot)
    p = R.knots(first, seq)
    p[1, knot, 2, 0] = np.nan
    out = R.resample(p[:, 0], p[:, 1:], rate, mode)
    want = np.zeros(out.shape, bool)
    for j in range(1, n * rate + 1):
        i, r = divmod(j, rate)
        want[1, j - 1, 2, 0] = (i == knot) if r == 0 else knot in R.stencil(i, n, mode)
    assert (np.isnan(out) == want).all() and want.any()


def test_the_speed_restatement_on_straight_and_stationary_motion():
    first = np.zeros((2, 3, 2), np.float32)
    step = np.array([3.0, 4.0], np.float32) / 64                      # |step| = 5 / 64, exact
    seq = first[:, None] + step * np.arange(1, 6, dtype=np.float32).reshape(1, 5, 1, 1)
    seq[1] = first[1, None]                                           # sample 1 stands still
    sp = R.speed(first, seq, scale=2.0)
    assert sp.shape == (2, 5) and (sp[0] == np.longdouble(10.0) / 64).all() and (sp[1] == 0).all()


def test_seam_ratio_on_hand_made_curves():
    from kpx_amd.resample import seam_ratio
    assert seam_ratio(np.ones(32), 32, 1) is None and seam_ratio(np.ones(64), 32, 2) is None
    sp = np.ones(96)
    sp[[32, 64]] = 3.0
    assert seam_ratio(sp, 96, 1) == 3.0
    sp = np.ones(128)
    sp[64] = 0.5                                                      # frames=64, rate=2: the seam is output frame 65, index 64
    assert seam_ratio(sp, 64, 2) == 0.5
    assert seam_ratio(np.zeros(64), 64, 1) is None                    # 0 / 0: no number


def test_the_wrappers_refuse_every_limit_before_the_library_is_called():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib, ops
    from kpx_amd._lib import KpxError
    z = lambda *shape: torch.zeros(1, dtype=torch.float32).expand(*shape)          # any size without the memory
    first, seq = torch.zeros(2, 3, 2), torch.zeros(2, 4, 3, 2)
    launched = _lib.abi_calls[0]
    for args, kw, text in (((first, seq, 2), dict(mode='spline'), 'mode must be one of'),
                           ((first, seq, 0), {}, 'rate must be an integer in \\[1, 64\\]'), ((first, seq, 65), {}, 'rate must be'),
                           ((first, seq, 2.0), {}, 'rate must be'), ((first, seq, True), {}, 'rate must be'),
                           ((first, seq[:, :1], 2), {}, "seq needs N >= 2 knots"), ((first[0], seq, 2), {}, 'first must be'),
                           ((first, seq[0], 2), {}, 'seq must be'), ((first, None, 2), {}, 'seq must be'),
                           ((z(2, 1025, 2), z(2, 4, 1025, 2), 2), {}, '1 <= K <= 1024'), ((z(2, 0, 2), z(2, 4, 0, 2), 2), {}, '1 <= K <= 1024'),
                           ((z(0, 3, 2), z(0, 4, 3, 2), 2), {}, 'B, N >= 1'), ((first, z(2, 0, 3, 2), 2), dict(mode='linear'), 'B, N >= 1'),
                           ((z(128, 1024, 2), z(128, 128, 1024, 2), 64), {}, 'fewer than 2\\^31'),
                           ((first, seq, 2), {}, 'no CPU fallback'), ((first, seq[:, :1], 2), dict(mode='linear'), 'no CPU fallback')):
        with pytest.raises(KpxError, match='points_resample: .*' + text):
            ops.points_resample(*args, **kw)
    for args, text in (((first, seq, float('nan')), 'scale must be a finite number'), ((first, seq, 'x'), 'scale must be'),
                       ((first, seq[0]), 'seq must be'), ((z(2, 1025, 2), z(2, 4, 1025, 2)), '1 <= K <= 1024'),
                       ((z(1024, 1024, 2), z(1024, 1024, 1024, 2)), 'fewer than 2\\^31'), ((first, seq), 'no CPU fallback')):
        with pytest.raises(KpxError, match='points_speed: .*' + text):
            ops.points_speed(*args)
    assert _lib.abi_calls[0] == launched


def test_the_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                       # an aligned fake address
    rs = lambda first=a, seq=a, b=2, n=4, k=3, f=2, mode=1, out=a: lib.kpx_points_resample_f32(first, seq, b, n, k, f, mode, out, None)
    for bad in (dict(first=None), dict(seq=None), dict(out=None), dict(b=0), dict(n=0), dict(k=0), dict(k=1025), dict(f=0), dict(f=65), dict(mode=2),
                dict(mode=-1), dict(n=1), dict(first=a + 2), dict(seq=a + 1), dict(out=a + 2), dict(b=128, n=128, k=1024, f=64),
                dict(b=1 << 30, n=1 << 30), dict(b=(1 << 31) - 1, n=(1 << 31) - 1, k=1024, f=64)):
        assert rs(**bad) == -1, bad
    sp = lambda first=a, seq=a, b=2, t=4, k=3, scale=1.0, speed=a: lib.kpx_points_speed_f64(first, seq, b, t, k, scale, speed, None)
    for bad in (dict(first=None), dict(seq=None), dict(speed=None), dict(b=0), dict(t=0), dict(k=0), dict(k=1025), dict(first=a + 2), dict(seq=a + 1),
                dict(speed=a + 4), dict(b=1024, t=1024, k=1024), dict(b=(1 << 31) - 1, t=(1 << 31) - 1)):
        assert sp(**bad) == -1, bad


def test_run_checks_frames_rate_and_resample_on_the_host():
    from kpx_amd._lib import KpxError
    from kpx_amd.resample import check_rollout_args
    assert check_rollout_args('x') == (1, 32) and check_rollout_args('x', 96, 4, 'linear') == (3, 384)
    for kw, text in ((dict(frames=0), 'frames must be a positive multiple of 32'), (dict(frames=48), 'frames must be'), (dict(frames=-32), 'frames must be'),
                     (dict(frames=64.0), 'frames must be'), (dict(rate=0), 'rate must be an integer in \\[1, 64\\]'), (dict(rate=65), 'rate must be'),
                     (dict(rate=1.5), 'rate must be'), (dict(resample='nearest'), 'resample must be one of')):
        with pytest.raises(KpxError, match='tool: ' + text):
            check_rollout_args('tool', **kw)


# ------------------------------------------------------------------------------------------------------------------ the tools' parsers
def test_evaluate_refuses_bad_long_rollout_arguments_without_a_gpu(tmp_path, monkeypatch, capsys):
    import sys
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval'), '--synthetic', '2']
    for extra, text in ((['--frames', '64'], 'need it'), (['--rate', '2'], 'need it'), (['--gif', '--resample', 'linear'], '--resample chooses how --rate'),
                        (['--gif', '--frames', '48'], '--frames takes a positive multiple of 32'), (['--gif', '--frames', '0'], '--frames takes'),
                        (['--gif', '--rate', '0'], '--rate takes 1..64'), (['--gif', '--rate', '65'], '--rate takes 1..64'),
                        (['--gif', '--rate', '2', '--resample', 'nearest'], '--resample takes linear or cubic'),
                        (['--gif', '--rate', '6'], '--gif-fps 10 x --rate 6 = 60'), (['--gif', '--gif-fps', '26', '--rate', '2'], 'lower --gif-fps'),
                        (['--gif', '--frames', '512'], '2^24'), (['--gif', '--frames', '64', '--rate', '8', '--gif-fps', '5'], '2^24'),
                        (['--gif', '--frames', '64', '--no-save'], '--no-save'),
                        (['--gif', '--frames', '64', '--drive', 'hold', '--drive-only'], '--drive-only')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_animate_refuses_bad_long_rollout_arguments_before_the_device_is_touched(tmp_path, capsys):
    from PIL import Image
    import animate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    still = tmp_path / 'still.png'
    Image.fromarray(np.full((40, 60, 3), 90, np.uint8)).save(str(still))
    video = tmp_path / 'video'
    video.mkdir()
    for i in range(33):
        Image.fromarray(np.full((16, 16, 3), 7 * i, np.uint8)).save(str(video / ('%03d.png' % i)))
    head = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--save_dir', str(tmp_path / 'out'), '--images', str(still)]
    two = head + ['--checkpoint_stage2', str(ck), '--actions', '0']
    for argv, text in ((two + ['--frames', '48'], '--frames takes a positive multiple of 32'), (two + ['--frames', '-32'], '--frames takes'),
                       (two + ['--rate', '0'], '--rate takes 1..64'), (two + ['--rate', '65'], '--rate takes 1..64'),
                       (two + ['--rate', '2', '--resample', 'nearest'], '--resample takes linear or cubic'), (two + ['--resample', 'linear'], 'needs --rate'),
                       (two + ['--rate', '6'], '--gif-fps 10 x --rate 6 = 60'), (two + ['--rate', '2', '--gif-fps', '26'], 'lower --gif-fps'),
                       (head + ['--driver', str(video), '--frames', '64'], 'with --driver'),
                       (two + ['--driver', str(video), '--frames', '32'], 'with --driver'),
                       (two + ['--frames', '64', '--sheet-frames', '64'], '--sheet-frames'), (two + ['--rate', '2', '--sheet-frames', '3,64'], '--sheet-frames'),
                       (two + ['--frames', '1024'], '2^24')):
        with pytest.raises(SystemExit) as e:
            animate.main(argv)
        assert e.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    assert not (tmp_path / 'out').exists() and not torch.cuda.is_initialized()
