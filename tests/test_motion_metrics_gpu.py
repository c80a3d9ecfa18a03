"""GPU: the motion metrics -- kpx_draw_moments_add_f32 and kpx_draw_diversity_f32 bit for bit against the int64 restatement
(motion_metrics_ref.py), kpx_keypoint_draw_metrics_f32 within one fp32 ulp of the float64 restatement (the same fp64 operations in the
same order, one final rounding); exact cases (identical draws, 0 against 255, D = 4096); bitwise batch and graph-replay invariance; argument
errors; and evaluate.py --metrics --motion-metrics end to end on the fixture videos."""
import json
import os

import numpy as np
import pytest
import torch

import motion_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _ops():
    from kpx_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pool():
    """NaN, the infinities, values outside [-1,1], every bucket edge k / 255 * 2 - 1 and its two neighbours, then noise: 4099 + 3 values"""
    edges = (np.arange(257, dtype=np.float64) / 255.0 * 2 - 1).astype(np.float32)
    near = np.concatenate([edges, np.nextafter(edges, np.float32(2)), np.nextafter(edges, np.float32(-2))])
    special = np.array([np.nan, np.inf, -np.inf, -1.5, 1.5, -1.0, 1.0, 0.0, -0.0, 3e38, -3e38, 1e-45], np.float32)
    rs = np.random.RandomState(0)
    noise = rs.uniform(-1.3, 1.3, size=4102 - special.size - near.size).astype(np.float32)
    return np.concatenate([special, near, noise])


POOL = _pool()


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4099])
def test_draw_moments_add_is_bit_equal_after_three_draws(n):
    ops = _ops()
    draws = [np.roll(POOL, -r)[:n].copy() for r in (0, 1, 2)]         # the specials reach the small sizes; every edge the large ones
    want_s, want_ss = R.moments(draws)
    # offsets in elements of (x, sum, sumsq): all 16-byte aligned; all 4-byte but not 16-byte aligned; one of the three off (scalar path)
    for offs in ((0, 0, 0), (1, 1, 1), (3, 2, 1), (1, 0, 0), (0, 0, 2)):
        xs = [torch.empty(n + 4, device=DEV)[o:o + n] for o in (offs[0],) * 3]
        guard = [torch.zeros(n + 4, dtype=torch.int32, device=DEV) for _ in range(2)]
        acc = [g[o:o + n] for g, o in zip(guard, offs[1:])]
        for x, d in zip(xs, draws):
            x.copy_(_dev(d))
            assert x.data_ptr() % 16 == 4 * offs[0] and x.is_contiguous()
            ops.draw_moments_add(x, acc[0], acc[1])
        got_s, got_ss = (a.cpu().numpy().view(np.uint32).astype(np.int64) for a in acc)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_ss, want_ss), (n, offs)
        for g, o in zip(guard, offs[1:]):                             # nothing written beside the n values
            g = g.cpu().numpy()
            assert not g[:o].any() and not g[o + n:].any(), (n, offs)


def _draws(n, h, w, c, d, rs):
    """d correlated draws of n frames in (and a little outside) [-1,1]: a base frame plus noise whose scale changes from frame to frame"""
    base = rs.uniform(-1.1, 1.1, size=(n, h, w, c))
    scale = rs.uniform(0.0, 0.6, size=(n, 1, 1, 1))
    return [(base + scale * rs.normal(size=base.shape)).astype(np.float32) for _ in range(d)]


def _accumulate(draws):
    ops = _ops()
    acc = torch.zeros((2, draws[0].size), dtype=torch.int32, device=DEV)
    for x in draws:
        ops.draw_moments_add(_dev(x), acc[0], acc[1])
    return acc


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (2, 5, 7, 3), (3, 16, 16, 1), (2, 128, 128, 3)])
def test_draw_diversity_is_bit_equal_for_both_outputs(shape):
    ops = _ops()
    n, h, w, c = shape
    rs = np.random.RandomState(n * 1000 + h)
    for d in (2, 3, 5):
        draws = _draws(n, h, w, c, d, rs)
        acc = _accumulate(draws)
        s, ss = R.moments(draws)
        assert np.array_equal(acc[0].cpu().numpy().astype(np.int64), s.reshape(-1))
        want_div, want_map = R.draw_diversity(s, ss, d, (h, w, c))
        div_mse, std_map = ops.draw_diversity(acc[0], acc[1], d, (h, w, c), std_map=True)
        assert div_mse.dtype == torch.float32 and tuple(div_mse.shape) == (n,) and std_map.dtype == torch.uint8
        assert np.array_equal(div_mse.cpu().numpy().view(np.uint32), want_div.view(np.uint32)), (shape, d)
        assert np.array_equal(std_map.cpu().numpy(), want_map), (shape, d)
        alone = ops.draw_diversity(acc[0], acc[1], d, (h, w, c))      # without the map: the same figure
        assert torch.equal(alone, div_mse)
        if h * w * c > 1:
            assert want_div.min() > 0 and want_map.max() > 0          # (the case says something)


def test_draw_diversity_exact_cases():
    ops = _ops()
    rs = np.random.RandomState(7)
    h, w, c = 9, 11, 3
    x = rs.uniform(-1.1, 1.1, size=(2, h, w, c)).astype(np.float32)
    for d in (2, 5):                                                  # identical draws: exactly 0 and an all-zero map
        acc = _accumulate([x] * d)
        div_mse, std_map = ops.draw_diversity(acc[0], acc[1], d, (h, w, c), std_map=True)
        assert (div_mse == 0).all() and not std_map.any()
    acc = _accumulate([np.full((2, h, w, c), -1.0, np.float32), np.full((2, h, w, c), 1.0, np.float32)])     # all 0 against all 255
    div_mse, std_map = ops.draw_diversity(acc[0], acc[1], 2, (h, w, c), std_map=True)
    assert (div_mse == 1.0).all() and (std_map == 255).all()
    # hand-written accumulators of 4096 draws, half of them 0 and half 255: D * sumsq = 2^12 * 2^11 * 65025 needs the 64-bit product
    d = 4096
    acc = torch.empty((2, 12), dtype=torch.int32, device=DEV)
    acc[0].fill_(255 * d // 2)
    acc[1].fill_(65025 * d // 2)
    want_div, want_map = R.draw_diversity(np.full(12, 255 * d // 2), np.full(12, 65025 * d // 2), d, (2, 2, 3))
    div_mse, std_map = ops.draw_diversity(acc[0], acc[1], d, (2, 2, 3), std_map=True)
    assert np.array_equal(div_mse.cpu().numpy().view(np.uint32), want_div.view(np.uint32)) and np.array_equal(std_map.cpu().numpy(), want_map)
    assert want_div[0] == np.float32(2048.0 * 2048.0 / (4096.0 * 4095.0 / 2.0)) and (want_map == 255).all()
    acc[0].fill_(255 * d)                                              # every draw 255: the largest accumulators, no diversity
    acc[1].fill_(65025 * d)
    div_mse, std_map = ops.draw_diversity(acc[0], acc[1], d, (2, 2, 3), std_map=True)
    assert (div_mse == 0).all() and not std_map.any()


KP_SHAPES = [(1, 1, 1, 1), (2, 3, 32, 15), (5, 2, 32, 40), (3, 1, 2, 64)]


def _points(d, n, t, k, rs):
    real = rs.uniform(-0.9, 0.9, size=(n, t, k, 2)).astype(np.float32)
    pts = (real[None] + rs.normal(scale=0.2, size=(d, n, t, k, 2))).astype(np.float32)
    return pts, real


@pytest.mark.parametrize('shape', KP_SHAPES)
def test_keypoint_draw_metrics_within_one_ulp_of_the_float64_restatement(shape):
    ops = _ops()
    d, n, t, k = shape
    pts, real = _points(d, n, t, k, np.random.RandomState(d * 100 + k))
    want_l2, want_div = R.keypoint_draw_metrics(pts, real)
    l2, div = ops.keypoint_draw_metrics(_dev(pts), _dev(real), diversity=d > 1)
    assert tuple(l2.shape) == (d, n, t) and l2.dtype == torch.float32
    assert R.within_one_ulp(l2.cpu().numpy(), want_l2), shape
    if d == 1:
        assert div is None and want_div is None
        return
    assert tuple(div.shape) == (n, t) and R.within_one_ulp(div.cpu().numpy(), want_div), shape
    assert want_l2.min() > 0 and want_div.min() > 0
    only_l2, none = ops.keypoint_draw_metrics(_dev(pts), _dev(real), diversity=False)
    assert none is None and torch.equal(only_l2, l2)
    same = np.repeat(pts[:1], d, axis=0)                               # identical draws: no diversity, one error
    l2, div = ops.keypoint_draw_metrics(_dev(same), _dev(real))
    assert (div == 0).all() and all(torch.equal(l2[i], l2[0]) for i in range(d))


def test_keypoint_non_finite_inputs_propagate_to_their_frames_alone():
    ops = _ops()
    d, n, t, k = 3, 2, 32, 15
    pts, real = _points(d, n, t, k, np.random.RandomState(5))
    pts[1, 0, 3, 7, 0] = np.nan
    pts[2, 1, 30, 0, 1] = np.inf
    pts[0, 1, 5, 14, 0] = -np.inf
    real[0, 9, 2, 1] = np.nan                                          # a label: every draw of that frame, but not their diversity
    want_l2, want_div = R.keypoint_draw_metrics(pts, real)
    l2, div = (x.cpu().numpy() for x in ops.keypoint_draw_metrics(_dev(pts), _dev(real)))
    assert R.within_one_ulp(l2, want_l2) and R.within_one_ulp(div, want_div)
    bad_l2 = np.zeros((d, n, t), bool)
    bad_l2[1, 0, 3] = bad_l2[2, 1, 30] = bad_l2[0, 1, 5] = bad_l2[:, 0, 9] = True
    bad_div = np.zeros((n, t), bool)
    bad_div[0, 3] = bad_div[1, 30] = bad_div[1, 5] = True
    assert np.array_equal(~np.isfinite(l2), bad_l2) and np.array_equal(~np.isfinite(div), bad_div)
    assert np.isnan(l2[1, 0, 3]) and np.isposinf(l2[2, 1, 30]) and np.isposinf(l2[0, 1, 5]) and np.isnan(l2[:, 0, 9]).all()
    assert np.isnan(div[0, 3]) and np.isposinf(div[1, 30]) and np.isposinf(div[1, 5])


def test_frame_results_are_bitwise_independent_of_batch_size_and_position():
    ops = _ops()
    rs = np.random.RandomState(8)
    n, h, w, c, d = 9, 33, 20, 3, 4
    draws = _draws(n, h, w, c, d, rs)
    acc = _accumulate(draws)
    div_mse, std_map = ops.draw_diversity(acc[0], acc[1], d, (h, w, c), std_map=True)
    again = ops.draw_diversity(acc[0], acc[1], d, (h, w, c), std_map=True)
    assert torch.equal(again[0], div_mse) and torch.equal(again[1], std_map)
    per = h * w * c
    for lo, hi in ((0, 1), (4, 5), (8, 9), (2, 7)):
        part = _accumulate([x[lo:hi] for x in draws])
        assert torch.equal(part, acc[:, lo * per:hi * per])
        pd, pm = ops.draw_diversity(part[0], part[1], d, (h, w, c), std_map=True)
        assert torch.equal(pd, div_mse[lo:hi]) and torch.equal(pm, std_map[lo:hi]), (lo, hi)
    pts, real = _points(d, 5, 32, 15, rs)
    l2, div = ops.keypoint_draw_metrics(_dev(pts), _dev(real))
    for lo, hi in ((0, 1), (4, 5), (1, 4)):
        pl, pdv = ops.keypoint_draw_metrics(_dev(pts[:, lo:hi]), _dev(real[lo:hi]))
        assert torch.equal(pl, l2[:, lo:hi]) and torch.equal(pdv, div[lo:hi]), (lo, hi)
    for t in (0, 31):                                                  # ... and of the other frames of the sample
        pl, pdv = ops.keypoint_draw_metrics(_dev(pts[:, :, t:t + 1]), _dev(real[:, t:t + 1]))
        assert torch.equal(pl, l2[:, :, t:t + 1]) and torch.equal(pdv, div[:, t:t + 1]), t


def test_graph_replay_of_the_three_calls_is_bitwise_the_eager_result():
    ops = _ops()
    rs = np.random.RandomState(9)
    n, h, w, c, d, k = 8, 64, 64, 3, 3, 15
    draws = [_dev(x) for x in _draws(n, h, w, c, d, rs)]
    pts, real = (_dev(x) for x in _points(d, n, 1, k, rs))
    acc = torch.zeros((2, n * h * w * c), dtype=torch.int32, device=DEV)
    div_mse, std_map = torch.empty((n,), device=DEV), torch.empty((n, h, w), dtype=torch.uint8, device=DEV)
    l2, div = torch.empty((d, n, 1), device=DEV), torch.empty((n, 1), device=DEV)

    def enqueue():
        ops.fill_raw_(acc, 0.0)
        for x in draws:
            ops.draw_moments_add(x, acc[0], acc[1])
        ops.draw_diversity(acc[0], acc[1], d, (h, w, c), std_map=std_map, out=div_mse)
        ops.keypoint_draw_metrics(pts, real, out=(l2, div))

    enqueue()
    torch.cuda.synchronize()
    outs = (acc, div_mse, std_map, l2, div)
    eager = [x.clone() for x in outs]
    assert float(eager[1].min()) > 0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for x in outs:
        x.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    for x, e in zip(outs, eager):
        assert torch.equal(x, e)


def test_bad_arguments_raise_kpx_error():
    from kpx_amd._lib import KpxError
    ops = _ops()
    x = torch.zeros((2, 4, 4, 3), device=DEV)
    acc = torch.zeros((2, x.numel()), dtype=torch.int32, device=DEV)
    s, ss = acc[0], acc[1]
    pts, real = torch.zeros((3, 2, 32, 15, 2), device=DEV), torch.zeros((2, 32, 15, 2), device=DEV)
    bad = [lambda: ops.draw_moments_add(x.double(), s, ss),                                     # dtype
           lambda: ops.draw_moments_add(x, s.float(), ss),
           lambda: ops.draw_moments_add(x, s, ss.long()),
           lambda: ops.draw_moments_add(x.cpu(), s, ss),                                        # device
           lambda: ops.draw_moments_add(x, s.cpu(), ss),
           lambda: ops.draw_moments_add(x.transpose(1, 2), s, ss),                              # contiguity
           lambda: ops.draw_moments_add(x, torch.zeros((2, 2 * x.numel()), dtype=torch.int32, device=DEV)[:, ::2][0], ss),
           lambda: ops.draw_moments_add(x, s[:-1], ss),                                         # sizes
           lambda: ops.draw_moments_add(x[:1], s, ss),
           lambda: ops.draw_moments_add(x, s, s),
           lambda: ops.draw_diversity(s.float(), ss, 2, (4, 4, 3)),
           lambda: ops.draw_diversity(s.cpu(), ss.cpu(), 2, (4, 4, 3)),
           lambda: ops.draw_diversity(s, ss[:-1], 2, (4, 4, 3)),
           lambda: ops.draw_diversity(s, ss, 2, (4, 5, 3)),                                     # not whole frames
           lambda: ops.draw_diversity(s, ss, 2, (4, 4)),
           lambda: ops.draw_diversity(s[:64], ss[:64], 2, (4, 8, 2)),                           # C = 2
           lambda: ops.draw_diversity(s, ss, 2, (1025, 1, 3)),
           lambda: ops.draw_diversity(s, ss, 1, (4, 4, 3)),                                     # one draw has no diversity
           lambda: ops.draw_diversity(s, ss, 4097, (4, 4, 3)),                                  # D > 4096
           lambda: ops.draw_diversity(s, ss, 2, (4, 4, 3), out=torch.empty((3,), device=DEV)),
           lambda: ops.draw_diversity(s, ss, 2, (4, 4, 3), std_map=torch.empty((2, 4, 4), device=DEV)),
           lambda: ops.draw_diversity(s, ss, 2, (4, 4, 3), std_map=torch.empty((2, 4, 4, 3), dtype=torch.uint8, device=DEV)),
           lambda: ops.keypoint_draw_metrics(pts.double(), real.double()),
           lambda: ops.keypoint_draw_metrics(pts, real.double()),
           lambda: ops.keypoint_draw_metrics(pts.cpu(), real.cpu()),
           lambda: ops.keypoint_draw_metrics(pts, real.cpu()),
           lambda: ops.keypoint_draw_metrics(pts.transpose(1, 2), real.transpose(0, 1)),
           lambda: ops.keypoint_draw_metrics(pts, real[:1]),                                    # shapes
           lambda: ops.keypoint_draw_metrics(pts[0], real),
           lambda: ops.keypoint_draw_metrics(pts, torch.zeros((2, 32, 14, 2), device=DEV)),
           lambda: ops.keypoint_draw_metrics(torch.zeros((3, 2, 32, 10, 3), device=DEV), torch.zeros((2, 32, 10, 3), device=DEV)),
           lambda: ops.keypoint_draw_metrics(pts[:1], real),                                    # D = 1 with the diversity
           lambda: ops.keypoint_draw_metrics(pts[:1], real, diversity=True),
           lambda: ops.keypoint_draw_metrics(torch.zeros((4097, 1, 1, 1, 2), device=DEV), torch.zeros((1, 1, 1, 2), device=DEV)),
           lambda: ops.keypoint_draw_metrics(pts, real, out=(torch.empty((3, 2, 31), device=DEV), None)),
           lambda: ops.keypoint_draw_metrics(pts, real, diversity=False, out=(None, torch.empty((2, 32), device=DEV)))]
    for i, f in enumerate(bad):
        with pytest.raises(KpxError):
            f()
            pytest.fail('case %d raised nothing' % i)
    assert not acc.any()                                               # nothing was launched


def _read_seq(d, n=32):
    from PIL import Image
    ims = [Image.open(os.path.join(d, '%06d.png' % i)) for i in range(n)]
    assert all(im.mode == 'L' for im in ims)
    return np.stack([np.asarray(im, np.uint8) for im in ims])


def test_evaluate_motion_metrics_end_to_end_on_the_fixture_videos(tmp_path, monkeypatch):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    from test_data_gpu import _fixture_dataset
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k, n_action = int(golden['n_points']), int(golden['n_action'])
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt])

    calls = []
    run = kpx_amd.FinalModel.run

    def recording_run(self, sess, feed_dict, z=None):
        out = run(self, sess, feed_dict, z=z)
        calls.append((out['pred_im_seq'].clone(), out['fut_pt_raw'].clone()))
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics',
            '--motion-metrics']
    recorded = {}
    for name, extra in (('eval', ['--samples', '3']), ('nosave', ['--samples', '3', '--no-save']), ('one', ['--samples', '1'])):
        del calls[:]
        torch.manual_seed(11)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
        recorded[name] = [(p.cpu().numpy(), q.cpu().numpy()) for p, q in calls]
    loader = kpx_amd.data.SequenceDataLoader(str(data), 'test', n_points=k, n_action=n_action, random_order=False, randomness=False,
                                             with_image_seq=True)
    labels = [b['real_seq'].cpu().numpy() for b in loader.batches(2, DEV, repeat=False, num_preprocess_threads=2)]
    assert [x.shape for x in labels] == [(2, 32, k, 2), (1, 32, k, 2)]               # batches of 2 and 1

    def expected(rec, d):
        assert len(rec) == d * len(labels)
        out = {'kp_l2': [], 'kp_div': [], 'div_mse': [], 'std': []}
        for b, real in enumerate(labels):
            draws = rec[b * d:(b + 1) * d]
            l2, div = R.keypoint_draw_metrics(np.stack([q for _, q in draws]), real)
            out['kp_l2'].append(l2.transpose(1, 0, 2))                                  # [B, D, 32]
            if d > 1:
                out['kp_div'].append(div)
                s, ss = R.moments([p for p, _ in draws])
                div_mse, std_map = R.draw_diversity(s, ss, d, (128, 128, 3))
                out['div_mse'].append(div_mse.reshape(-1, 32))
                out['std'].append(std_map.reshape(-1, 32, 128, 128))
        return {key: np.concatenate(v) for key, v in out.items() if v}

    ev = tmp_path / 'eval'
    want = expected(recorded['eval'], 3)
    npz = np.load(str(ev / 'metrics.npz'))
    assert sorted(npz.files) == ['div_mse', 'kp_div', 'kp_l2', 'mse', 'psnr', 'ssim']
    assert npz['kp_l2'].shape == (3, 3, 32) and npz['kp_div'].shape == (3, 32) and npz['div_mse'].shape == (3, 32)
    assert all(npz[key].dtype == np.float32 for key in npz.files)
    assert np.array_equal(npz['div_mse'].view(np.uint32), want['div_mse'].view(np.uint32))
    assert R.within_one_ulp(npz['kp_l2'], want['kp_l2']) and R.within_one_ulp(npz['kp_div'], want['kp_div'])
    assert npz['div_mse'].max() > 0 and npz['kp_div'].max() > 0 and np.isfinite(npz['kp_l2']).all()      # fresh z per draw
    samples = sorted(n for n in os.listdir(str(ev)) if n.isdigit())
    assert samples == ['0000', '0001', '0002']
    for s, name in enumerate(samples):
        assert np.array_equal(_read_seq(str(ev / name / 'pred_std')), want['std'][s]), name
        assert len(os.listdir(str(ev / name / 'pred_std'))) == 32 and len(os.listdir(str(ev / name / 'pred_seq'))) == 32
    summary = json.loads((ev / 'metrics.json').read_text())
    assert (summary['n_samples'], summary['n_draws'], summary['n_nonfinite']) == (3, 3, 0)
    assert summary['definition'].endswith(evaluate.MOTION_METRICS_DEFINITION)
    assert set(summary['kp_l2']) == set(summary['ssim']) and len(summary['kp_l2']['per_frame']) == 32
    per_draw = npz['kp_l2'].astype(np.float64).mean(axis=2)
    assert summary['kp_l2']['best_draw'] == [int(i) for i in per_draw.argmin(axis=1)]
    assert summary['kp_l2']['best_of_draws'] <= summary['kp_l2']['mean']
    for key in ('kp_div', 'div_mse'):
        assert set(summary[key]) == {'mean', 'per_frame'} and len(summary[key]['per_frame']) == 32
        assert abs(summary[key]['mean'] - npz[key].astype(np.float64).mean()) <= 1e-12

    assert sorted(os.listdir(str(tmp_path / 'nosave'))) == ['metrics.json', 'metrics.npz']
    npz2 = np.load(str(tmp_path / 'nosave' / 'metrics.npz'))
    assert sorted(npz2.files) == sorted(npz.files)
    for key in npz.files:
        assert np.array_equal(npz[key], npz2[key]), key

    one = tmp_path / 'one'
    npz1 = np.load(str(one / 'metrics.npz'))
    assert sorted(npz1.files) == ['kp_l2', 'mse', 'psnr', 'ssim'] and npz1['kp_l2'].shape == (3, 1, 32)
    assert R.within_one_ulp(npz1['kp_l2'], expected(recorded['one'], 1)['kp_l2'])
    summary1 = json.loads((one / 'metrics.json').read_text())
    assert 'kp_l2' in summary1 and 'kp_div' not in summary1 and 'div_mse' not in summary1
    for name in samples:
        assert os.path.isdir(str(one / name / 'pred_seq')) and not os.path.exists(str(one / name / 'pred_std'))
