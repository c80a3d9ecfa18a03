"""CPU: the host half of evaluate.py --posterior and animate.py --interpolate / --motion-from -- the constants against the header, the argument
errors of the three wrappers, of the C entries and of the two tools, ``summarise_posterior`` on hand-made states (collapse, dead sigma, an
empty class, a single row), the numpy restatement of the state against tests/posterior_ref.py, and ``python -m kpx_amd.posterior`` on a small
posterior.npz.  None of it needs a GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import posterior_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def test_constants_mirror_the_header():
    from kpx_amd import ops, posterior, tool_ops
    src = open(os.path.join(REPO, 'include', 'kpx.h')).read()
    val = lambda name: eval(re.search(r'#define\s+%s\s+(.+)' % name, src).group(1))
    assert posterior.LATENT_MAX_DIM == val('KPX_LATENT_MAX_DIM') == 1024
    assert posterior.LATENT_STATE_FIELDS == val('KPX_LATENT_STATE_FIELDS') == 8 == len(posterior.STATE_FIELDS)
    assert posterior.LATENT_PATH_MAX_STEPS == val('KPX_LATENT_PATH_MAX_STEPS') == 64
    assert posterior.LATENT_PATH_MIN_SIN == val('KPX_LATENT_PATH_MIN_SIN') == 1e-6
    enum = re.search(r'enum \{ KPX_LATENT_PATH_LERP = (\d+), KPX_LATENT_PATH_SLERP = (\d+) \}', src)
    assert posterior.LATENT_PATH_MODES == {'lerp': int(enum.group(1)), 'slerp': int(enum.group(2))}
    assert val('KPX_ABI_VERSION') == 25                                 # new entries, no signature changed
    for name in ('latent_stats_add', 'latent_sample', 'latent_path'):
        assert getattr(ops, name) is getattr(tool_ops, name) is getattr(posterior, name)
        assert name not in tool_ops.__all__
    assert ops.LATENT_MAX_DIM == 1024 and ops.LATENT_PATH_MAX_STEPS == 64


def test_the_wrappers_and_the_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd import _lib, ops
    from kpx_amd._lib import KpxError, lib
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt)
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    launched = _lib.abi_calls[0]
    logit, state, counts = z(f32, 3, 10), z(f64, 2, 5, 8), z(i64, 2, 3)
    for call, text in ((lambda: ops.latent_stats_add(logit, state, counts, z(i32, 3)), 'latent_stats_add: logit .*no CPU fallback'),
                       (lambda: ops.latent_stats_add(z(f32, 3, 0), state, counts), 'latent_stats_add: logit needs'),           # V = 0
                       (lambda: ops.latent_stats_add(z(f32, 3, 2050), state, counts), 'latent_stats_add: logit needs'),        # V = 1025
                       (lambda: ops.latent_stats_add(z(f32, 3, 9), state, counts), r'latent_stats_add: logit must be an fp32 tensor \[B, 2V\]'),
                       (lambda: ops.latent_stats_add(z(f32, 0, 10), state, counts), 'latent_stats_add: logit needs'),
                       (lambda: ops.latent_stats_add(logit, z(f64, 0, 5, 8), z(i64, 0, 3)), 'latent_stats_add: state must be'),       # G = 0
                       (lambda: ops.latent_stats_add(logit, state, counts), 'latent_stats_add: group is needed'),
                       (lambda: ops.latent_stats_add(logit, state[0], counts), 'latent_stats_add: state must be'),
                       (lambda: ops.latent_sample(logit, z(f32, 3, 5)), 'latent_sample: logit .*no CPU fallback'),
                       (lambda: ops.latent_sample(logit, None, float('nan')), 'latent_sample: tau must be a finite number'),
                       (lambda: ops.latent_sample(logit, None, True), 'latent_sample: tau'),
                       (lambda: ops.latent_sample(z(f32, 10), None), 'latent_sample: logit must be'),
                       (lambda: ops.latent_path(z(f32, 3, 5), z(f32, 3, 5), 3), 'latent_path: za .*no CPU fallback'),
                       (lambda: ops.latent_path(z(f32, 3, 5), z(f32, 3, 5), 1), r'latent_path: steps must be an integer in \[2, 64\]'),
                       (lambda: ops.latent_path(z(f32, 3, 5), z(f32, 3, 5), 65), 'latent_path: steps'),
                       (lambda: ops.latent_path(z(f32, 3, 5), z(f32, 3, 5), 2.0), 'latent_path: steps'),
                       (lambda: ops.latent_path(z(f32, 3, 5), z(f32, 3, 5), 3, 'cubic'), 'latent_path: mode must be one of'),
                       (lambda: ops.latent_path(z(f32, 3, 1025), z(f32, 3, 1025), 3), 'latent_path: needs'),
                       (lambda: ops.latent_path(z(f32, 5), z(f32, 5), 3), 'latent_path: za must be')):
        with pytest.raises(KpxError, match=text):
            call()
    assert _lib.abi_calls[0] == launched
    a = 1 << 20                                                       # an aligned fake address
    stats = lambda logit=a, b=3, v=5, group=a, g=2, state=a, counts=a, rows=a: lib.kpx_latent_stats_add_f64(logit, b, v, group, g, state, counts, rows, None)
    for bad in (dict(v=0), dict(v=1025), dict(b=0), dict(g=0), dict(group=None), dict(logit=None), dict(state=None), dict(counts=None),
                dict(logit=a + 2), dict(group=a + 2), dict(state=a + 4), dict(counts=a + 4), dict(rows=a + 4), dict(b=1 << 21, v=1024),
                dict(g=1 << 19, v=1024)):
        assert stats(**bad) == -1, bad
    sample = lambda logit=a, eps=a, tau=1.0, out=a, b=3, v=5: lib.kpx_latent_sample_f32(logit, eps, tau, out, b, v, None)
    for bad in (dict(v=0), dict(v=1025), dict(b=0), dict(logit=None), dict(out=None), dict(tau=float('nan')), dict(eps=a + 1), dict(out=a + 2),
                dict(b=1 << 21, v=1024)):
        assert sample(**bad) == -1, bad
    path = lambda za=a, zb=a, s=3, mode=1, out=a, b=3, v=5: lib.kpx_latent_path_f32(za, zb, s, mode, out, b, v, None)
    for bad in (dict(s=1), dict(s=65), dict(mode=2), dict(mode=-1), dict(v=0), dict(v=1025), dict(b=0), dict(za=None), dict(zb=None), dict(out=None),
                dict(za=a + 2), dict(out=a + 1), dict(s=64, b=1 << 16, v=1024)):
        assert path(**bad) == -1, bad


def _state(mu, sigma, group=None, groups=1):
    from kpx_amd import posterior
    logit = np.concatenate([np.asarray(mu, np.float32), np.asarray(sigma, np.float32)], axis=1)
    return posterior.state_numpy(logit, group, groups)


def test_state_numpy_is_the_sequential_restatement():
    from kpx_amd import posterior
    for (b, v, g), integer in (((3, 5, 1), True), ((65, 100, 9), False), ((64, 64, 9), True)):
        logit, group = P.stats_inputs(b, v, g, seed=b + v, integer=integer)
        logit[b // 2, 1] = np.nan
        group = group.copy()
        group[0] = g
        got = posterior.state_numpy(logit, group, g)
        want = P.stats_sequential(logit, group, g)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(np.isfinite(got[2]), want[2]) and want[1][0, 2] == 1 and want[1][:, 1].sum() == (0 if b // 2 == 0 else 1)
        # pieces leave the bits of one call
        s, c, _ = posterior.state_numpy(logit[:1], group[:1], g)
        s, c, _ = posterior.state_numpy(logit[1:], group[1:], g, s, c)
        assert np.array_equal(s, got[0]) and np.array_equal(c, got[1])


def test_summary_of_a_collapsed_posterior():
    """every mu equal, sigma = 1: no active unit, kl = 0.5 mu^2, and the aggregate is N(mu, 1)"""
    from kpx_amd import posterior
    mu = np.tile(np.array([[0.5, 0.0, 2.0]], np.float32), (7, 1))
    state, counts, _ = _state(mu, np.ones_like(mu))
    blk = posterior.summarise_posterior(state, counts)
    assert blk['n'] == 7 and blk['vae_dim'] == 3 and blk['active_units'] == 0 and blk['au_threshold'] == 0.01
    assert blk['mu_var'] == [0.0, 0.0, 0.0] and blk['mu_mean'] == [0.5, 0.0, 2.0] and blk['sigma_mean'] == [1.0, 1.0, 1.0]
    want = [0.5 * (m * m - np.log(np.float64(np.float32(1e-8)) + 1.0)) for m in (0.5, 0.0, 2.0)]
    assert np.allclose(blk['kl_per_dim'], want, rtol=0, atol=1e-15) and np.isclose(blk['kl_total'], sum(want), rtol=0, atol=1e-15)
    assert np.allclose(blk['agg_kl_per_dim'], [0.125, 0.0, 2.0], rtol=0, atol=1e-15) and np.isclose(blk['agg_kl_total'], 2.125)
    assert blk['dead_mu_share'] == [0.0, 1.0, 0.0] and blk['dead_sigma_share'] == [0.0, 0.0, 0.0]
    assert blk['counts'] == {'rows': 7, 'non_finite': 0, 'bad_group': 0}
    assert 'not comparable with published figures' in blk['definition']
    json.dumps(blk, allow_nan=False)


def test_summary_of_dead_sigma_an_empty_class_and_a_single_row():
    from kpx_amd import posterior
    rs = np.random.RandomState(3)
    mu = rs.rand(6, 4).astype(np.float32)
    mu[:, 3] = [0, 1, 0, 1, 0, 1]                                      # variance 0.25: active
    sigma = rs.rand(6, 4).astype(np.float32)
    sigma[:, 0] = 0                                                    # a dead sigma unit
    group = np.array([0, 0, 2, 0, 0, 0], np.int32)                    # class 1 empty, class 2 a single row
    state, counts, kl_rows = _state(mu, sigma, group, 3)
    blk = posterior.summarise_posterior(state, counts)
    dead = 0.5 * (-np.log(np.float64(np.float32(1e-8))) - 1.0)         # 8.71 nats
    assert abs(dead - 8.71) < 0.005
    assert np.isclose(blk['kl_per_dim'][0], dead + 0.5 * np.mean(mu[:, 0].astype(np.float64) ** 2), rtol=1e-14)
    assert blk['dead_sigma_share'] == [1.0, 0.0, 0.0, 0.0] and blk['dead_mu_share'][3] == 0.5
    assert blk['n'] == 6 and blk['active_units'] == 1 + sum(np.var(mu[:, d].astype(np.float64)) > 0.01 for d in range(3))
    m64, s64 = mu.astype(np.float64), sigma.astype(np.float64)
    s2 = m64.var(axis=0) + (s64 ** 2).mean(axis=0)
    want = 0.5 * (m64.mean(axis=0) ** 2 + s2 - np.log(s2) - 1)
    assert np.allclose(blk['agg_kl_per_dim'], want, rtol=1e-12, atol=1e-14)
    assert np.allclose(kl_rows, P.stats_longdouble(np.concatenate([mu, sigma], 1), group, 3)[2].astype(np.float64), rtol=1e-14)
    per = blk['per_class']
    assert sorted(per) == ['0', '1', '2'] and per['1'] == {'n': 0, 'non_finite': 0} and per['0']['n'] == 5
    one = per['2']
    assert one['n'] == 1 and one['mu_var'] == [0.0] * 4 and one['active_units'] == 0            # one row: the variance is 0, not NaN
    assert one['mu_mean'] == [float(x) for x in m64[2]]
    # sigma dead and a single row: s2 = 0, the aggregate marginal is a point mass and its KL is null
    assert one['agg_kl_per_dim'][0] is None and all(x is not None for x in one['agg_kl_per_dim'][1:])
    assert posterior.summarise_posterior(state, counts, au_threshold=0.3)['active_units'] == 0
    assert posterior.summarise_posterior(state * 0, counts * 0)['n'] == 0
    json.dumps(blk, allow_nan=False)
    for bad in ((state[0], counts), (state, counts[:2]), (state[:, :, :7], counts)):
        with pytest.raises(ValueError, match='summarise_posterior'):
            posterior.summarise_posterior(*bad)
    with pytest.raises(ValueError, match='au_threshold'):
        posterior.summarise_posterior(state, counts, au_threshold=-1)


def test_module_resummarises_a_stored_file(tmp_path, capsys):
    from kpx_amd import posterior
    logit, group = P.stats_inputs(20, 6, 4, seed=9)
    state, counts, kl_rows = posterior.state_numpy(logit, group, 4)
    path = str(tmp_path / 'posterior.npz')
    np.savez(path, logit=logit, classes=group, kl_rows=kl_rows, state=state, counts=counts, au_threshold=np.float64(0.05))
    assert posterior.main([path]) == 0
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(posterior.summarise_posterior(state, counts, 0.05)))
    assert posterior.main([path, '--au', '0.2']) == 0
    assert json.loads(capsys.readouterr().out)['au_threshold'] == 0.2
    for argv in ([], [path, path], [path, '--au'], [path, '--au', 'x'], [path, '--au', '-1']):
        assert posterior.main(argv) == 2
        assert 'usage: python -m kpx_amd.posterior' in capsys.readouterr().err


def test_evaluate_posterior_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval')]
    for extra, text in ((['--posterior', '--synthetic', '2'], '--synthetic inputs have none'),
                        (['--posterior', '--drive', 'hold', '--drive-only'], '--drive-only'),
                        (['--posterior-transfer'], 'need it'), (['--posterior-au', '0.1'], 'need it'),
                        (['--posterior', '--posterior-au', '-0.5'], '--posterior-au takes a finite threshold'),
                        (['--posterior', '--posterior-au', 'nan'], '--posterior-au takes a finite threshold'),
                        (['--posterior', '--posterior-transfer', '--no-save'], '--no-save writes none'),
                        (['--posterior', '--sheet-frames', '3'], '--sheet-frames picks the frames'),
                        (['--posterior', '--posterior-transfer', '--sheet-frames', '32'], '--sheet-frames')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_animate_latent_argument_errors_need_no_gpu(tmp_path, capsys):
    from PIL import Image
    import animate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    still = tmp_path / 'still.png'
    Image.fromarray(np.zeros((40, 60, 3), np.uint8)).save(str(still))
    video = tmp_path / 'video'
    video.mkdir()
    for i in range(33):
        Image.fromarray(np.full((16, 16, 3), i, np.uint8)).save(str(video / ('%03d.png' % i)))
    short = tmp_path / 'short'
    short.mkdir()
    cfg = os.path.join(REPO, 'configs', 'penn.yaml')                   # n_action = 9
    head = ['--config', cfg, '--checkpoint_stage1', str(ck), '--save_dir', str(tmp_path / 'out'), '--images', str(still)]
    two = head + ['--checkpoint_stage2', str(ck)]
    cases = [(two + ['--interpolate', '3'], '--samples >= 2'), (two + ['--interpolate', '1', '--samples', '2'], '--interpolate takes 2..64'),
             (two + ['--interpolate', '65', '--samples', '2'], '--interpolate takes 2..64'),
             (two + ['--interp-mode', 'lerp'], '--interp-mode'), (two + ['--interpolate', '3', '--samples', '2', '--interp-mode', 'cubic'], '--interp-mode'),
             (head + ['--driver', str(video), '--interpolate', '3', '--samples', '2'], '--checkpoint_stage2'),
             (two + ['--interpolate', '3', '--samples', '2', '--rate', '2'], 'not with --frames or --rate'),
             (two + ['--interpolate', '64', '--samples', '2', '--actions', '0,1,2,3,4,5,6,7'], '2^24'),
             (two + ['--motion-from', str(video)], 'go together'), (two + ['--motion-class', '1'], 'go together'),
             (two + ['--motion-from', str(video), '--motion-class', '9'], '--motion-class'),
             (two + ['--motion-from', str(video), '--motion-class', '-1'], '--motion-class'),
             (two + ['--motion-from', str(short), '--motion-class', '1'], '--motion-from'),
             (two + ['--motion-from', str(video), '--motion-class', '1', '--driver', str(video)], 'give one of them'),
             (head + ['--driver', str(video), '--motion-from', str(video), '--motion-class', '1'], 'give one of them'),
             (two + ['--motion-from', str(video), '--motion-class', '1', '--frames', '64'], 'not with --frames or --rate')]
    for argv, text in cases:
        with pytest.raises(SystemExit) as e:
            animate.main(argv)
        assert e.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    assert not (tmp_path / 'out').exists() and not torch.cuda.is_initialized()
