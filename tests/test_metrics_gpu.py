"""GPU: the frame metrics kernel (kpx_frame_metrics_f32 via ops.frame_metrics) against the float64 restatement (metrics_ref.py) on noise,
ramps, the flat cases where fp32 moments fail and the fixture videos; its exact cases (identical frames, one 8-bit bucket); bitwise batch,
run, alignment and graph-replay invariance; argument errors; and evaluate.py --metrics end to end on the fixture videos."""
import io
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device('cuda:0')
SHAPES = [(11, 11), (12, 37), (128, 128), (129, 67), (256, 256)]
KINDS = ['noise', 'ramp', 'const', 'eps', 'eps_noise', 'flat8']


def _ops():
    from kpx_amd import ops
    return ops


def _content(kind, n, h, w, c, rs):
    shape = (n, h, w, c)
    if kind == 'noise':
        return rs.uniform(0, 1, shape), rs.uniform(0, 1, shape)
    if kind == 'ramp':
        y = np.linspace(0, 1, h)[None, :, None, None]
        x = np.linspace(0, 1, w)[None, None, :, None]
        ch = np.arange(c)[None, None, None, :]
        a = 0.1 + 0.6 * x + 0.2 * y + 0.05 * ch + np.zeros(shape)
        return a, 0.15 + 0.5 * x + 0.25 * y + 0.05 * ch + 0.01 * rs.uniform(0, 1, shape)
    if kind == 'const':
        return np.full(shape, 0.3), np.full(shape, 0.7)
    if kind == 'eps':
        return np.full(shape, 0.61), np.full(shape, 0.611)
    if kind == 'eps_noise':
        a = 0.61 + 1e-3 * rs.uniform(0, 1, shape)
        return a, a + 1e-3
    return rs.randint(180, 185, size=shape) / 255.0, rs.randint(181, 186, size=shape) / 255.0      # flat8


def _check(got, want, what):
    got = got.cpu().numpy().astype(np.float64)
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 1e-5, (what, got[:, 0], want[:, 0])
    assert (np.abs(got[:, 1] - want[:, 1]) <= 1e-6 * np.abs(want[:, 1])).all(), (what, got[:, 1], want[:, 1])
    fin = np.isfinite(want[:, 2])
    assert np.array_equal(np.isfinite(got[:, 2]), fin) and (got[~fin, 2] == want[~fin, 2]).all(), what
    assert np.abs(got[fin, 2] - want[fin, 2]).max(initial=0) <= 1e-4, (what, got[:, 2], want[:, 2])


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('c', [1, 3])
def test_kernel_matches_the_float64_restatement(h, w, c):
    ops = _ops()
    rs = np.random.RandomState(h * 1000 + w * 10 + c)
    for kind in KINDS:
        a, b = (x.astype(np.float32) for x in _content(kind, 2, h, w, c, rs))
        got = ops.frame_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
        _check(got, M.frame_metrics(a, b), (kind, h, w, c))
    a = rs.uniform(0, 255, size=(2, h, w, c)).astype(np.float32)                  # another dynamic range
    b = np.clip(a + rs.normal(0, 8, size=a.shape), 0, 255).astype(np.float32)
    _check(_ops().frame_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), max_val=255.0), M.frame_metrics(a, b, 255.0),
           ('L255', h, w, c))


def _fixture_frames():
    from PIL import Image
    golden = np.load(os.path.join(HERE, 'golden', 'image_pair_ref.npz'))
    names = [str(n) for n in golden['file_names']]
    ims = [np.asarray(Image.open(io.BytesIO(golden['file_%03d' % k].tobytes())).convert('RGB'), np.float32) / 255.0
           for k, n in enumerate(names) if n.endswith('.jpg')][:9]
    h = min(i.shape[0] for i in ims)
    w = min(i.shape[1] for i in ims)
    return np.stack([i[:h, :w] for i in ims])


def test_kernel_matches_the_restatement_on_fixture_video_frames():
    frames = _fixture_frames()
    a, b = frames[:-1], frames[1:]                                                # consecutive frames of the fixture videos
    got = _ops().frame_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    _check(got, M.frame_metrics(a, b), 'fixture')
    q = a * 2 - 1, b * 2 - 1                                                      # the png8 path on the same frames in [-1, 1]
    got8 = _ops().frame_metrics(torch.from_numpy(q[0]).to(DEV), torch.from_numpy(q[1]).to(DEV), png8=True)
    _check(got8, M.frame_metrics_png8(*q), 'fixture png8')


@pytest.mark.parametrize('png8', [False, True])
def test_identical_inputs_are_exact(png8):
    rs = np.random.RandomState(3)
    for h, w in SHAPES:
        for c in (1, 3):
            a = torch.from_numpy(rs.uniform(-1, 1, size=(2, h, w, c)).astype(np.float32)).to(DEV)
            m = _ops().frame_metrics(a, a.clone(), png8=png8).cpu()
            assert (m[:, 0] == 1.0).all() and (m[:, 1] == 0).all() and torch.isposinf(m[:, 2]).all(), (h, w, c, m)


def test_png8_matches_the_restatement_and_one_bucket_scores_one():
    rs = np.random.RandomState(4)
    for h, w, c in ((128, 128, 3), (129, 67, 1), (37, 12, 3)):
        a = rs.uniform(-1.2, 1.2, size=(3, h, w, c)).astype(np.float32)           # out-of-range values clamp
        b = rs.uniform(-1.2, 1.2, size=(3, h, w, c)).astype(np.float32)
        _check(_ops().frame_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), png8=True), M.frame_metrics_png8(a, b),
               ('png8', h, w, c))
        # values a few ulps apart in the same 8-bit bucket: different floats, the same bytes
        q = rs.randint(1, 255, size=(3, h, w, c))
        x = ((q + 0.3) / 255.0 * 2 - 1).astype(np.float32)                         # never 0 (whose neighbouring bit patterns are NaN)
        y = (x.view(np.int32) + rs.randint(-3, 4, size=x.shape).astype(np.int32)).view(np.float32)
        assert np.array_equal(M.png8(x), M.png8(y)) and not np.array_equal(x, y)
        m = _ops().frame_metrics(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), png8=True).cpu()
        assert (m[:, 0] == 1.0).all() and (m[:, 1] == 0).all() and torch.isposinf(m[:, 2]).all()


def test_frame_results_are_bitwise_independent_of_batch_position_alignment_and_run():
    ops = _ops()
    n, h, w, c = 2048, 128, 128, 3
    g = torch.Generator(device=DEV).manual_seed(5)
    a = torch.rand((n, h, w, c), generator=g, device=DEV)
    b = torch.rand((n, h, w, c), generator=g, device=DEV)
    full = ops.frame_metrics(a, b)
    again = ops.frame_metrics(a, b)
    assert torch.equal(full, again)
    for i in (0, 1, 777, 2047):
        assert torch.equal(ops.frame_metrics(a[i:i + 1], b[i:i + 1])[0], full[i]), i
    # the same frames at a 4-byte offset (no 16-byte loads) give the same bits
    fa = torch.empty(8 * h * w * c + 1, device=DEV)
    fb = torch.empty(8 * h * w * c + 1, device=DEV)
    ua, ub = fa[1:].view(8, h, w, c), fb[1:].view(8, h, w, c)
    ua.copy_(a[100:108])
    ub.copy_(b[100:108])
    assert torch.equal(ops.frame_metrics(ua, ub), full[100:108])


def test_graph_replay_is_bitwise_the_eager_launch():
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(6)
    a = torch.rand((64, 128, 128, 3), generator=g, device=DEV) * 2 - 1
    b = torch.rand((64, 128, 128, 3), generator=g, device=DEV) * 2 - 1
    eager = ops.frame_metrics(a, b, png8=True)
    out = torch.empty((64, 3), device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.frame_metrics(a, b, png8=True, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.frame_metrics(a, b, png8=True, out=out)
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_bad_arguments_raise_kpx_error():
    from kpx_amd._lib import KpxError
    ops = _ops()
    a = torch.zeros((2, 16, 16, 3), device=DEV)
    bad = [lambda: ops.frame_metrics(a.double(), a.double()),
           lambda: ops.frame_metrics(a, a.double()),
           lambda: ops.frame_metrics(a.transpose(1, 2), a),
           lambda: ops.frame_metrics(a, torch.zeros((2, 16, 17, 3), device=DEV)),
           lambda: ops.frame_metrics(a[:, :10], a[:, :10].contiguous()),
           lambda: ops.frame_metrics(torch.zeros((2, 10, 16, 3), device=DEV), torch.zeros((2, 10, 16, 3), device=DEV)),
           lambda: ops.frame_metrics(torch.zeros((2, 16, 16, 2), device=DEV), torch.zeros((2, 16, 16, 2), device=DEV)),
           lambda: ops.frame_metrics(a, a, max_val=0.0),
           lambda: ops.frame_metrics(a, a, max_val=-1.0),
           lambda: ops.frame_metrics(a.cpu(), a.cpu()),
           lambda: ops.frame_metrics(a, a, out=torch.empty((3, 3), device=DEV))]
    for f in bad:
        with pytest.raises(KpxError):
            f()


def _read_seq(d):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(d, '%06d.png' % i)), np.float64) for i in range(32)])


def test_evaluate_metrics_end_to_end_on_the_fixture_videos(tmp_path):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
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
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics', '--samples', '2']
    torch.manual_seed(11)
    evaluate.main(base + ['--save_dir', str(tmp_path / 'eval')])
    torch.manual_seed(11)
    evaluate.main(base + ['--save_dir', str(tmp_path / 'nosave'), '--no-save'])

    ev = tmp_path / 'eval'
    npz = np.load(str(ev / 'metrics.npz'))
    samples = sorted(n for n in os.listdir(str(ev)) if n.isdigit())
    assert samples == ['0000', '0001', '0002']                                    # batches of 2 and 1
    for key in ('ssim', 'psnr', 'mse'):
        assert npz[key].shape == (3, 2, 32) and npz[key].dtype == np.float32
    for s, name in enumerate(samples):
        pred, real = _read_seq(str(ev / name / 'pred_seq')), _read_seq(str(ev / name / 'real_seq'))
        want = M.frame_metrics(pred / 255.0, real / 255.0)                          # draw 0 = the written PNGs
        got = np.stack([npz['ssim'][s, 0], npz['mse'][s, 0], npz['psnr'][s, 0]], axis=1)
        _check(torch.from_numpy(got), want, name)
    summary = json.loads((ev / 'metrics.json').read_text())
    assert (summary['n_samples'], summary['n_draws'], summary['n_nonfinite']) == (3, 2, 0)
    for key in ('ssim', 'psnr'):
        per_draw = npz[key].astype(np.float64).mean(axis=2)                         # [S, N]
        assert (per_draw.max(axis=1) >= per_draw.mean(axis=1)).all()
        assert summary[key]['best_of_draws'] >= summary[key]['mean'] and len(summary[key]['per_frame']) == 32
    assert not np.array_equal(npz['ssim'][:, 0], npz['ssim'][:, 1])                 # fresh z per draw
    assert sorted(os.listdir(str(tmp_path / 'nosave'))) == ['metrics.json', 'metrics.npz']
    npz2 = np.load(str(tmp_path / 'nosave' / 'metrics.npz'))
    for key in ('ssim', 'psnr', 'mse'):
        assert np.array_equal(npz[key], npz2[key]), key
