"""GPU: evaluate.py --frechet -- kpx_feature_pool_f64 (ops.feature_pool) and kpx_moments_add_f64 (ops.moments_add) against the longdouble
restatement (frechet_ref.py) with derived bounds, their exact integer cases, bitwise batch / run / graph-replay invariance and argument
errors; vgg.FeatureScorer feeding a FrechetAccumulator against the float64 VGG19 of the oracle without a second forward; and
evaluate.py --frechet end to end on the fixture videos."""
import json
import os

import numpy as np
import pytest
import torch

import feature_metrics_ref as F
import frechet_ref as R
from test_feature_metrics_gpu import VGG_CASES, _contents, _dev, _vgg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EPS = 2.0 ** -53
POOL_SHAPES = [(3, 1, 1, 512), (2, 2, 3, 64), (2, 5, 7, 4), (2, 37, 12, 132), (4, 8, 8, 512), (1, 128, 128, 64), (70000, 1, 1, 4)]
MOMENT_SHAPES = [(1, 1), (5, 3), (7, 64), (33, 65), (100, 132), (64, 512), (9, 1024), (300, 16)]
PARITY_BAR = 1e-4       # the project's parity bar
# Through VGG19 (test 5): |got - want| / (tr C1 + tr C2 + |m1 - m2|^2) of the distance from the device path (fp32 VGG19, fp64 pooling and
# moments) against the float64 network, the largest over the cases, layers and both levels as printed by the test on an MI355X, and the
# bound: twice that, capped by the parity bar (the convention of VGG_COS_ABS in test_feature_metrics_gpu.py).
# Measured: 3.391e-6 (full width, 64 x 64, seed 0, conv5_4, two frames: frame and video level alike); the width / 8 cases stay under 9.9e-7.
VGG_FD_REL_MEASURED = 3.391e-6
VGG_FD_REL = min(2 * VGG_FD_REL_MEASURED, PARITY_BAR)         # 6.782e-6, under the parity bar


def _ops():
    from kpx_amd import ops
    return ops


def _dev64(x):
    return torch.from_numpy(np.array(x, dtype=np.float64)).to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the pool against float64
@pytest.mark.parametrize('shape', POOL_SHAPES)
def test_pool_matches_the_longdouble_restatement(shape):
    n, h, w, c = shape
    p = h * w
    rs = np.random.RandomState(sum(shape) % 65521)
    for name, a, _ in _contents(shape, rs):
        got = _ops().feature_pool(_dev(a))
        assert got.shape == (n, c) and got.dtype == torch.float64 and got.is_cuda
        want = R.pool(a, R.LD)
        # any-order fp64 summation of P exact inputs and one division: (P + 2) 2^-53 mean |x|, per element
        bound = (p + 2) * EPS * R.pool(np.abs(a), R.LD)
        err = np.abs(got.cpu().numpy().astype(R.LD) - want)
        worst = float((err / np.where(bound > 0, bound, 1)).max())
        print('%s %s: worst error / bound %.3f' % (name, shape, worst))
        assert (err <= bound).all(), (name, shape, worst)


@pytest.mark.parametrize('shape', [(2, 16, 16, 64), (3, 4, 4, 132), (1, 128, 128, 64), (5, 1, 2, 512), (2, 64, 128, 4)])
def test_pool_of_integers_over_a_power_of_two_is_bit_equal_to_the_integer_mean(shape):
    n, h, w, c = shape
    rs = np.random.RandomState(7 + sum(shape))
    q = rs.randint(0, 1 << 20, size=shape).astype(np.int64)
    q[0, :, :, 0] = 0                                                          # a channel that is zero everywhere
    got = _ops().feature_pool(_dev(q)).cpu().numpy()
    want = q.reshape(n, h * w, c).sum(axis=1).astype(np.float64) / float(h * w)   # < 2^34: exact, and so is the division by 2^k
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 2. the moments against longdouble
def _moment_inputs(m, d, rs, integers=False):
    """rows and symmetric non-zero starting accumulators"""
    if integers:
        x = rs.randint(0, 1 << 20, size=(m, d)).astype(np.float64)
        s0 = rs.randint(1, 1 << 20, size=d).astype(np.float64)
        o0 = rs.randint(1, 1 << 20, size=(d, d)).astype(np.float64)
    else:
        x = np.maximum(0, rs.normal(size=(m, d))) * rs.choice([1.0, 1e3, 1e-3], size=(1, d)) + rs.normal(size=(m, d)) * 0.1
        s0 = rs.normal(size=d) * 10
        o0 = rs.normal(size=(d, d)) * 10
    return x, s0, o0 + o0.T


def _moments_on_device(x, s0, o0, splits=None):
    s, o = _dev64(s0), _dev64(o0)
    xd = _dev64(x)
    for part in ([xd] if splits is None else [xd[:splits].contiguous(), xd[splits:].contiguous()]):
        rs_, ro_ = _ops().moments_add(part, s, o)
        assert rs_ is s and ro_ is o
    return s, o


def _moment_bounds(x, s0, o0):
    m = x.shape[0]
    sa, oa = R.abs_moments(x, s0, o0)
    return (m + 2) * EPS * sa, (m + 2) * EPS * oa


@pytest.mark.parametrize('m,d', MOMENT_SHAPES)
def test_moments_match_the_longdouble_restatement(m, d):
    rs = np.random.RandomState(100 * m + d)
    x, s0, o0 = _moment_inputs(m, d, rs)
    s, o = _moments_on_device(x, s0, o0)
    want_s, want_o = R.moments(x, s0, o0)
    bound_s, bound_o = _moment_bounds(x, s0, o0)
    err_s = np.abs(s.cpu().numpy().astype(R.LD) - want_s)
    err_o = np.abs(o.cpu().numpy().astype(R.LD) - want_o)
    print('(%d, %d): worst error / bound: sum %.3f, outer %.3f' % (m, d, float((err_s / bound_s).max()), float((err_o / bound_o).max())))
    assert (err_s <= bound_s).all() and (err_o <= bound_o).all()
    assert torch.equal(o, o.t())                                               # bitwise symmetric
    s2, o2 = _moments_on_device(x, s0, o0)
    assert torch.equal(s, s2) and torch.equal(o, o2)                           # run to run
    if m >= 2:                                                                 # two calls on the halves: the same bound
        sh, oh = _moments_on_device(x, s0, o0, splits=m // 2)
        assert (np.abs(sh.cpu().numpy().astype(R.LD) - want_s) <= bound_s).all()
        assert (np.abs(oh.cpu().numpy().astype(R.LD) - want_o) <= bound_o).all()
        assert torch.equal(oh, oh.t())


@pytest.mark.parametrize('m,d', [(1, 1), (7, 64), (33, 65), (300, 16), (1024, 132), (64, 512), (9, 1024)])
def test_moments_of_integers_are_bit_equal_to_the_integer_restatement(m, d):
    rs = np.random.RandomState(m + 3 * d)
    x, s0, o0 = _moment_inputs(m, d, rs, integers=True)
    s, o = _moments_on_device(x, s0, o0)
    xi = x.astype(np.int64)
    want_s = s0.astype(np.int64) + xi.sum(axis=0)
    want_o = o0.astype(np.int64) + xi.T @ xi                                   # < 2^21 + 1024 * 2^40 < 2^53: every partial sum is exact
    assert np.array_equal(s.cpu().numpy(), want_s.astype(np.float64))
    assert np.array_equal(o.cpu().numpy(), want_o.astype(np.float64))
    sh, oh = _moments_on_device(x, s0, o0, splits=(m + 1) // 2) if m >= 2 else (s, o)
    assert torch.equal(sh, s) and torch.equal(oh, o)


# ------------------------------------------------------------------------------------------------ 3. bitwise invariance
@pytest.mark.parametrize('h,w,c', [(16, 16, 256), (4, 4, 512)])
def test_pool_rows_are_bitwise_independent_of_batch_position_and_run(h, w, c):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(5)
    a = torch.relu(torch.randn((64, h, w, c), generator=g, device=DEV))
    full = ops.feature_pool(a)
    assert torch.equal(ops.feature_pool(a), full)                              # run to run
    for i in range(64):
        assert torch.equal(ops.feature_pool(a[i:i + 1])[0], full[i]), i
    assert torch.equal(ops.feature_pool(a[17:40]), full[17:40])                # another batch size and position


def test_graph_replay_of_pool_and_moments_is_bitwise_the_eager_launches():
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(6)
    a = torch.relu(torch.randn((64, 16, 16, 256), generator=g, device=DEV))
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
    pooled, s, o = ops.feature_pool(a), zeros(256), zeros(256, 256)
    ops.moments_add(pooled, s, o)
    out, gs, go = torch.empty((64, 256), dtype=torch.float64, device=DEV), zeros(256), zeros(256, 256)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.feature_pool(a, out=out)
        ops.moments_add(out, gs, go)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.feature_pool(a, out=out)
        ops.moments_add(out, gs, go)
    out.fill_(-1.0)
    gs.zero_()
    go.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, pooled) and torch.equal(gs, s) and torch.equal(go, o)
    graph.replay()                                                             # in place: the second replay adds the same rows again
    torch.cuda.synchronize()
    ops.moments_add(pooled, s, o)
    assert torch.equal(gs, s) and torch.equal(go, o)


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_bad_arguments_raise_kpx_error():
    from kpx_amd._lib import KpxError
    ops = _ops()
    a = torch.zeros((2, 4, 6, 8), device=DEV)
    flat = torch.zeros(2 * 4 * 6 * 8 + 1, device=DEV)
    off = flat[1:].view(2, 4, 6, 8)                                            # contiguous, 4 bytes past a 16-byte boundary
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
    x, s, o = f64(5, 8), f64(8), f64(8, 8)
    bad = [lambda: ops.feature_pool(a.double()),
           lambda: ops.feature_pool(a.bfloat16()),
           lambda: ops.feature_pool(a.transpose(1, 2)),
           lambda: ops.feature_pool(a[0]),
           lambda: ops.feature_pool(torch.zeros((2, 4, 6, 6), device=DEV)),
           lambda: ops.feature_pool(torch.zeros((1, 2, 2, 516), device=DEV)),
           lambda: ops.feature_pool(torch.zeros((1, 1025, 1, 4), device=DEV)),
           lambda: ops.feature_pool(torch.zeros((0, 4, 6, 8), device=DEV)),
           lambda: ops.feature_pool(off),
           lambda: ops.feature_pool(a.cpu()),
           lambda: ops.feature_pool(a, out=f64(3, 8)),
           lambda: ops.feature_pool(a, out=torch.empty((2, 8), device=DEV)),
           lambda: ops.feature_pool(a, out=f64(2, 16)[:, :8]),
           lambda: ops.feature_pool(a, out=torch.empty((2, 8), dtype=torch.float64)),
           lambda: ops.moments_add(x.float(), s, o),
           lambda: ops.moments_add(x, s.float(), o),
           lambda: ops.moments_add(x, s, o.float()),
           lambda: ops.moments_add(x.t(), f64(5), f64(5, 5)),
           lambda: ops.moments_add(x, s, f64(8, 16)[:, :8]),
           lambda: ops.moments_add(x[0], s, o),
           lambda: ops.moments_add(f64(0, 8), s, o),
           lambda: ops.moments_add(f64(2, 1025), f64(1025), f64(1025, 1025)),
           lambda: ops.moments_add(x, f64(7), o),
           lambda: ops.moments_add(x, s, f64(8, 7)),
           lambda: ops.moments_add(x, s, f64(64)),
           lambda: ops.moments_add(x.cpu(), s, o),
           lambda: ops.moments_add(x, s.cpu(), o),
           lambda: ops.moments_add(x, s, o.cpu())]
    for i, f in enumerate(bad):
        with pytest.raises(KpxError):
            f()
            print('no error from case %d' % i)


# ------------------------------------------------------------------------------------------------ 5. through VGG19 against float64
_refs = {}


def _frames_per_video(n):
    """the longest video length that still splits n frames into two or more videos"""
    return max(t for t in range(1, n + 1) if n % t == 0 and n // t >= 2) if n >= 2 else 1


def _vgg_case(width_div, h, w, n, seed):
    """The frames a (predicted), b (real) in [-1,1] of a case and the float64 statistics of both at both levels, computed once and shared."""
    key = (width_div, h, w, n, seed)
    if key not in _refs:
        rs = np.random.RandomState(seed)
        a = rs.uniform(-1, 1, size=(n, h, w, 3)).astype(np.float32)
        b = np.clip(a + rs.normal(0, 0.2, size=a.shape), -1, 1).astype(np.float32)
        t = _frames_per_video(n)
        feats = F.vgg_features(_vgg(width_div)[1], np.concatenate([a, b], axis=0))
        want = {}
        for level in ('frame', 'video'):
            rows = [R.pool(f) for f in feats]
            pa, pb = [r[:n] for r in rows], [r[n:] for r in rows]
            if level == 'video':
                pa, pb = [R.descriptor(r, t) for r in pa], [R.descriptor(r, t) for r in pb]
            want[level] = ([R.stats(r) for r in pa], [R.stats(r) for r in pb])
        for arr in (a, b):
            arr.setflags(write=False)
        _refs[key] = (a, b, t, want)
    return _refs[key]


@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('width_div,h,w,n', VGG_CASES)
def test_scorer_feeds_the_accumulator_and_matches_the_float64_network(width_div, h, w, n, seed, monkeypatch):
    from kpx_amd import frechet as K, vgg as V
    assert VGG_FD_REL <= PARITY_BAR
    a, b, t, want = _vgg_case(width_div, h, w, n, seed)
    net = _vgg(width_div)[0]
    calls = [0]
    build = net.build

    def counting(*args, **kwargs):
        calls[0] += 1
        return build(*args, **kwargs)
    monkeypatch.setattr(net, 'build', counting)
    plain = V.FeatureScorer(net, _dev(b))
    scores = plain(_dev(a))
    today = calls[0]
    calls[0] = 0
    dims = [int(net.params[name][0].shape[3]) for name in V.FEATURE_LAYERS]
    real, pred = K.FrechetAccumulator(dims, DEV), K.FrechetAccumulator(dims, DEV)
    scorer = V.FeatureScorer(net, _dev(b), frechet=real, frames_per_video=t)
    with_acc = scorer(_dev(a), frechet=pred)
    assert calls[0] == today == 2                                              # no second forward for the accumulators
    assert torch.equal(with_acc, scores)                                       # and the scores are today's, bit for bit
    sr, sp = real.stats(), pred.stats()
    worst = 0.0
    for level in ('frame', 'video'):
        rows = n if level == 'frame' else n // t
        for layer in range(5):
            wa, wb = want[level][0][layer], want[level][1][layer]
            assert sp[level][layer]['n'] == sr[level][layer]['n'] == rows
            got = K.frechet_distance(sp[level][layer]['mean'], sp[level][layer]['cov'], sr[level][layer]['mean'], sr[level][layer]['cov'])
            ref = R.distance(wa['mean'], wa['cov'], wb['mean'], wb['cov'])
            if rows < 2:
                assert np.isnan(got) and np.isnan(ref)
                continue
            rel = abs(got - ref) / R.scale(wa['mean'], wa['cov'], wb['mean'], wb['cov'])
            print('vgg /%d %dx%d seed %d %s layer %d: FD %.6e (float64 %.6e), error / scale %.3e' % (width_div, h, w, seed, level, layer, got, ref, rel))
            worst = max(worst, rel)
    print('worst error / scale %.3e (bound %.3e)' % (worst, VGG_FD_REL))
    assert worst <= VGG_FD_REL, worst


def test_scorer_joins_chunks_before_it_splits_videos(monkeypatch):
    """FEATURE_CHUNK = 2 cuts 3 frames into chunks of 2 and 1; the accumulator still sees them as videos of 3 and of 1 frames"""
    from kpx_amd import frechet as K, vgg as V
    a, b, _, _ = _vgg_case(8, 16, 16, 3, 0)
    net = _vgg(8)[0]
    dims = [int(net.params[name][0].shape[3]) for name in V.FEATURE_LAYERS]
    res = {}
    for chunk in (2, 64):
        monkeypatch.setattr(V, 'FEATURE_CHUNK', chunk)
        one, three = K.FrechetAccumulator(dims, DEV), K.FrechetAccumulator(dims, DEV)
        V.FeatureScorer(net, _dev(b), frechet=one, frames_per_video=3)(_dev(a), frechet=[one, three])
        V.FeatureScorer(net, _dev(b), frechet=three, frames_per_video=1)
        res[chunk] = (one, three)
        assert [int(m['n'].item()) for m in one.moments['video']] == [2] * 5 and [int(m['n'].item()) for m in three.moments['video']] == [4] * 5
        assert [int(m['n'].item()) for m in one.moments['frame']] == [6] * 5
    for x, y in zip(res[2], res[64]):                                          # pooled rows do not depend on the chunking: the same bits
        for level in K.LEVELS:
            for m, k in zip(x.moments[level], y.moments[level]):
                assert torch.equal(m['sum'], k['sum']) and torch.equal(m['outer'], k['outer'])
    with pytest.raises(Exception):
        V.FeatureScorer(net, _dev(b), frames_per_video=2)


def test_split_routes_videos_by_global_parity():
    from kpx_amd import frechet as K
    rs = np.random.RandomState(3)
    rows = rs.normal(size=(5 * 4, 8))                                          # five videos of four frames
    for first in (0, 1):
        even, odd = K.FrechetAccumulator([8], DEV), K.FrechetAccumulator([8], DEV)
        K.FrechetSplit([even, odd], first).add_pooled([_dev64(rows)], 4)
        vid = rows.reshape(5, 4, 8)
        for acc, sel in ((even, vid[(np.arange(5) + first) % 2 == 0]), (odd, vid[(np.arange(5) + first) % 2 == 1])):
            s = acc.stats()
            want = R.stats(sel.reshape(-1, 8))
            assert s['frame'][0]['n'] == want['n'] and s['video'][0]['n'] == len(sel)
            assert np.abs(s['frame'][0]['mean'] - want['mean']).max() <= 1e-14
            assert np.abs(s['frame'][0]['cov'] - want['cov']).max() <= 1e-13
            wv = R.stats(R.descriptor(sel.reshape(-1, 8), 4))
            assert np.abs(s['video'][0]['mean'] - wv['mean']).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ 6. evaluate.py end to end
FRECHET_ARRAYS = ['vgg_fd_draw0_layers', 'vgg_fd_floor_layers', 'vgg_fd_layers', 'vgg_fvd_floor_layers', 'vgg_fvd_layers']


def test_evaluate_frechet_end_to_end_on_the_fixture_videos(tmp_path):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    from kpx_amd import frechet as K
    from test_data_gpu import _fixture_dataset
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k = int(golden['n_points'])
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': int(golden['n_action']), 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt])
    without = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics', '--samples', '2',
               '--vgg-metrics', '--synthetic-vgg']
    base = without + ['--frechet']
    torch.manual_seed(11)
    evaluate.main(base + ['--save_dir', str(tmp_path / 'eval')])
    torch.manual_seed(11)
    evaluate.main(base + ['--save_dir', str(tmp_path / 'nosave'), '--no-save'])
    torch.manual_seed(11)
    evaluate.main(without + ['--save_dir', str(tmp_path / 'plain')])

    ev = tmp_path / 'eval'
    npz = np.load(str(ev / 'metrics.npz'))
    today = ['mse', 'psnr', 'ssim', 'vgg_cos', 'vgg_cos_layers', 'vgg_l1', 'vgg_l1_layers']
    assert sorted(npz.files) == sorted(today + FRECHET_ARRAYS)
    for key in FRECHET_ARRAYS:
        assert npz[key].shape == (5,) and npz[key].dtype == np.float64
    summary = json.loads((ev / 'metrics.json').read_text())
    blk = summary['frechet']
    assert (blk['n_real'], blk['n_pred'], blk['n_real_videos'], blk['n_pred_videos']) == (96, 192, 3, 6)
    assert blk['dims'] == {'frame': [64, 128, 256, 512, 512], 'video': [128, 256, 512, 1024, 1024]}
    assert blk['rank_deficient'] == {'frame': [False, True, True, True, True], 'video': [True] * 5}           # n <= D, n = 96 real frames
    assert blk['vgg_layers'] == F.LAYERS and 'not FID/FVD' in blk['definition']
    assert summary['definition'].endswith(evaluate.FRECHET_DEFINITION) and evaluate.VGG_METRICS_DEFINITION in summary['definition']
    assert blk['vgg_fd'] == blk['vgg_fd_layers'][4] and blk['vgg_fvd'] == blk['vgg_fvd_layers'][4]
    # 2 + 1 videos: the odd half has one video and no covariance; the frame-level floor is 64 frames against 32
    assert np.isnan(npz['vgg_fvd_floor_layers']).all() and blk['vgg_fvd_floor_layers'] == [None] * 5
    for key in ('vgg_fd_layers', 'vgg_fvd_layers', 'vgg_fd_draw0_layers', 'vgg_fd_floor_layers'):
        assert np.isfinite(npz[key]).all(), key
        assert blk[key] == [float(v) for v in npz[key]]
    # every distance from the stored statistics, by the restatement
    stored = np.load(str(ev / 'frechet.npz'))
    layers = [str(v) for v in stored['layers']]
    assert layers == F.LAYERS

    def stat(name, level, layer):
        key = '%s_%s_%s_' % (name, level, layers[layer])
        cov = stored[key + 'cov']
        return int(stored[key + 'n']), stored[key + 'mean'], cov if cov.size else None
    for key, (x, y, level) in {'vgg_fd_layers': ('pred', 'real', 'frame'), 'vgg_fvd_layers': ('pred', 'real', 'video'),
                               'vgg_fd_draw0_layers': ('pred_draw0', 'real', 'frame'),
                               'vgg_fd_floor_layers': ('real_even', 'real_odd', 'frame'),
                               'vgg_fvd_floor_layers': ('real_even', 'real_odd', 'video')}.items():
        for layer in range(5):
            (n1, m1, c1), (n2, m2, c2) = stat(x, level, layer), stat(y, level, layer)
            want = R.distance(m1, c1, m2, c2)
            got = npz[key][layer]
            if key == 'vgg_fvd_floor_layers':
                assert (n1, n2) == (2, 1) and c2 is None and np.isnan(want) and np.isnan(got)
                continue
            print('%s %s: %.6e (n = %d, %d), rel to restatement %.3e' % (key, layers[layer], got, n1, n2, abs(got - want) / abs(want)))
            assert abs(got - want) <= 1e-9 * abs(want), (key, layer, got, want)
            if key == 'vgg_fd_floor_layers':
                assert (n1, n2) == (64, 32)
                assert got >= -1e-6 * (np.trace(c1) + np.trace(c2)), (layer, got)
    assert stat('pred', 'frame', 0)[0] == 192 and stat('pred_draw0', 'frame', 0)[0] == 96 and stat('pred', 'video', 4)[0] == 6
    assert K.main([str(ev / 'frechet.npz'), str(tmp_path / 'nosave' / 'frechet.npz')]) == 0

    # --no-save: the same arrays
    assert sorted(os.listdir(str(tmp_path / 'nosave'))) == ['frechet.npz', 'metrics.json', 'metrics.npz']
    npz2 = np.load(str(tmp_path / 'nosave' / 'metrics.npz'))
    assert sorted(npz2.files) == sorted(npz.files)
    for key in npz.files:
        assert np.array_equal(npz[key], npz2[key], equal_nan=True), key
    # without the flag: exactly the files, keys and values written before it existed
    plain = tmp_path / 'plain'
    assert sorted(os.listdir(str(plain))) == [n for n in sorted(os.listdir(str(ev))) if n != 'frechet.npz']
    assert sorted(os.listdir(str(plain / '0000'))) == sorted(os.listdir(str(ev / '0000')))
    npz3 = np.load(str(plain / 'metrics.npz'))
    assert sorted(npz3.files) == today
    for key in today:
        assert np.array_equal(npz[key], npz3[key]), key
    plain_summary = json.loads((plain / 'metrics.json').read_text())
    assert sorted(plain_summary) == ['definition', 'mse', 'n_draws', 'n_nonfinite', 'n_samples', 'psnr', 'ssim', 'vgg_cos', 'vgg_l1', 'vgg_layers']
    assert plain_summary['definition'] == evaluate.METRICS_DEFINITION + ' ' + evaluate.VGG_METRICS_DEFINITION
    assert all(plain_summary[key] == summary[key] for key in plain_summary if key != 'definition')
