"""GPU: evaluate.py --actions -- kpx_sheet_paste_u8_f32 bit for bit against the numpy restatement (sheet_ref.py) on every load / store path
(16-byte, 4-byte and scalar; RGB and grey), with the bytes around the pasted cells untouched; a whole sheet, batch invariance, graph replay
and argument errors; then evaluate.py --metrics --actions end to end on the fixture videos: the shared z, the two sheets against the
recorded rollouts and against the PNGs of the sample's own rollout, the class scores against motion_metrics_ref, and the run without
--actions unchanged."""
import json
import os

import numpy as np
import pytest
import torch

import motion_metrics_ref as M
import sheet_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FILL = 0xA5
SHEET_FRAMES = [3, 7, 11, 15, 19, 23, 27, 31]


def _ops():
    from kpx_amd import ops
    return ops


def _pool():
    """NaN, the infinities, values below 0 / -1 and above 1, every bucket edge of both quantisers (k / 255 and k / 255 * 2 - 1) with its two
    float32 neighbours, then noise"""
    unit = np.arange(257, dtype=np.float64) / 255.0
    edges = np.concatenate([unit, unit * 2 - 1]).astype(np.float32)
    near = np.concatenate([edges, np.nextafter(edges, np.float32(2)), np.nextafter(edges, np.float32(-2))])
    special = np.array([np.nan, np.inf, -np.inf, -1.5, 1.5, -1.0, 1.0, 0.0, -0.0, 3e38, -3e38, 1e-45, -0.25, 1.25, 2.0, -2.0], np.float32)
    rs = np.random.RandomState(0)
    noise = rs.uniform(-1.3, 1.3, size=4099 - special.size - near.size).astype(np.float32)
    return np.concatenate([special, near, noise])


POOL = _pool()


def _src(shape, shift=0):
    return np.resize(np.roll(POOL, -shift), int(np.prod(shape))).reshape(shape).astype(np.float32)


def _dev_at(a, off):
    """a on the device, contiguous, its first element ``off`` elements past a 16-byte boundary"""
    buf = torch.empty(a.size + 16, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    assert t.is_contiguous() and t.data_ptr() % 16 == (off * a.itemsize) % 16
    return t


def _canvas(b, rows, cols, h, w, off=0):
    """-> (guard buffer, canvas view into it ``off`` bytes past a 16-byte boundary), all FILL"""
    n = b * rows * h * cols * w * 3
    guard = torch.full((n + 48,), FILL, dtype=torch.uint8, device=DEV)
    return guard, guard[16 + off:16 + off + n].view(b, rows * h, cols * w, 3)


#        name                (B, F, H, W, C)       sheet    cell    frames            src off, canvas off    path
CASES = [('smallest',         (1, 1, 1, 1, 1),      (1, 1),  (0, 0), [0],              0, 0),                # scalar, degenerate sizes
         ('scalar path',      (2, 5, 5, 7, 3),      (3, 4),  (1, 1), [4, 0, 2],        0, 0),                # odd W, unordered frames
         ('grey',             (3, 4, 16, 16, 1),    (2, 5),  (1, 0), [0, 1, 2, 3, 3],  0, 0),                # C = 1, 16-byte path, a repeat
         ('workload cell',    (2, 32, 128, 128, 3), (3, 9),  (2, 1), SHEET_FRAMES,     0, 0),                # the real cell, 16-byte path
         ('misaligned bases', (2, 3, 8, 12, 3),     (2, 3),  (1, 1), [2, 0],           1, 1),                # scalar: both bases off
         ('misaligned src',   (2, 3, 8, 12, 3),     (2, 3),  (1, 1), [2, 0],           1, 0),
         ('misaligned sheet', (2, 3, 8, 12, 3),     (2, 3),  (1, 1), [2, 0],           0, 1),
         ('4-byte rgb',       (2, 3, 8, 12, 3),     (2, 3),  (0, 1), [1, 2],           0, 0),                # W % 4 == 0 only: 4-byte stores
         ('4-byte sheet',     (2, 3, 4, 16, 3),     (2, 3),  (1, 0), [0, 2, 1],        0, 4),                # W % 16 == 0, sheet 4-byte aligned
         ('4-byte grey',      (3, 4, 16, 16, 1),    (2, 5),  (0, 2), [3, 0],           0, 12),
         ('grey scalar',      (2, 2, 3, 5, 1),      (2, 2),  (1, 1), [1],              0, 0),
         ('full limits',      (1, 64, 1, 1, 3),     (64, 64), (63, 0), list(range(63, -1, -1)), 0, 0)]     # J = 64, the last row


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_sheet_paste_is_bit_equal_to_the_restatement(case):
    ops = _ops()
    _, shape, (rows, cols), (row, col), frames, src_off, canvas_off = case
    b, f, h, w, c = shape
    for shift, premap in enumerate(('unit', 'raw')):
        x = _src(shape, shift=7 * shift)
        src = _dev_at(x, src_off)
        guard, canvas = _canvas(b, rows, cols, h, w, canvas_off)
        want = R.paste(np.full(tuple(canvas.shape), FILL, np.uint8), x, frames, row, col, premap)
        assert ops.sheet_paste(canvas, src, frames, row, col, premap) is canvas
        got = canvas.cpu().numpy()
        assert np.array_equal(got, want), (case[0], premap, int((got != want).sum()))
        g = guard.cpu().numpy()                                       # nothing before or after the sheet, nothing outside the cells
        assert (g[:16 + canvas_off] == FILL).all() and (g[16 + canvas_off + got.size:] == FILL).all()
        outside = np.ones(got.shape, bool)
        outside[:, row * h:(row + 1) * h, col * w:(col + len(frames)) * w] = False
        assert (got[outside] == FILL).all()
        if got.size > 64:
            assert (got[~outside] != FILL).any()


def test_a_whole_sheet_built_by_several_pastes():
    ops = _ops()
    b, f, h, w = 2, 6, 6, 8
    image, grey, seq_a, seq_b = _src((b, 1, h, w, 3), 1), _src((b, f, h, w, 1), 2), _src((b, f, h, w, 3), 3), _src((b, f, h, w, 3), 4)
    frames = [1, 3, 5]
    _, canvas = _canvas(b, 3, 4, h, w)
    want = np.full(tuple(canvas.shape), FILL, np.uint8)
    for row, seq, premap in ((0, seq_a, 'unit'), (1, seq_b, 'unit'), (2, grey, 'raw')):
        for args in ((image, [0], row, 0, 'unit'), (seq, frames, row, 1, premap)):
            R.paste(want, *args)
            ops.sheet_paste(canvas, _dev_at(args[0], 0), *args[1:])
    got = canvas.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 2 * h:, w:, 0], got[:, 2 * h:, w:, 2])                  # the grey row: one value in three channels


def test_pasting_a_batch_equals_pasting_its_samples_one_by_one():
    ops = _ops()
    for shape in ((3, 4, 16, 16, 3), (3, 4, 5, 7, 1)):
        b, f, h, w, c = shape
        src = _dev_at(_src(shape, 5), 0)
        _, whole = _canvas(b, 2, 3, h, w)
        _, parts = _canvas(b, 2, 3, h, w)
        ops.sheet_paste(whole, src, [3, 1], 1, 1, 'unit')
        for i in range(b):
            ops.sheet_paste(parts[i:i + 1], src[i:i + 1], [3, 1], 1, 1, 'unit')
        assert torch.equal(whole, parts) and bool((whole != FILL).any())


def test_graph_replay_of_three_pastes_is_bitwise_the_eager_result():
    ops = _ops()
    b, f, h, w = 4, 8, 32, 32
    image, seq, grey = _dev_at(_src((b, 1, h, w, 3), 1), 0), _dev_at(_src((b, f, h, w, 3), 2), 0), _dev_at(_src((b, f, h, w, 1), 3), 0)
    _, canvas = _canvas(b, 2, 4, h, w)

    def enqueue():
        ops.sheet_paste(canvas, image, [0], 0, 0, 'unit')
        ops.sheet_paste(canvas, seq, [7, 2, 5], 0, 1, 'unit')
        ops.sheet_paste(canvas, grey, [6, 0, 0, 1], 1, 0, 'raw')

    enqueue()
    torch.cuda.synchronize()
    eager = canvas.clone()
    assert not bool((eager == FILL).all())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    canvas.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(canvas, eager)                                 # (the three pastes cover the sheet: the frame indices replayed too)


def test_bad_arguments_raise_kpx_error_and_launch_nothing():
    from kpx_amd._lib import KpxError
    ops = _ops()
    b, f, h, w = 2, 4, 8, 8
    src = torch.zeros((b, f, h, w, 3), device=DEV)
    _, canvas = _canvas(b, 2, 3, h, w)
    wide = torch.full((b, 2 * h, 6 * w, 3), FILL, dtype=torch.uint8, device=DEV)
    bad = [lambda: ops.sheet_paste(canvas.float(), src, [0], 0, 0, 'unit'),                       # dtype
           lambda: ops.sheet_paste(canvas, src.double(), [0], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src.to(torch.uint8), [0], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas.cpu(), src, [0], 0, 0, 'unit'),                         # device
           lambda: ops.sheet_paste(canvas, src.cpu(), [0], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas.cpu(), src.cpu(), [0], 0, 0, 'unit'),
           lambda: ops.sheet_paste(wide[:, :, ::2], src, [0], 0, 0, 'unit'),                      # contiguity
           lambda: ops.sheet_paste(canvas, src.transpose(2, 3), [0], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas[0], src, [0], 0, 0, 'unit'),                            # dimensions
           lambda: ops.sheet_paste(canvas, src[:, 0], [0], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas[:1], src, [0], 0, 0, 'unit'),                           # batch sizes
           lambda: ops.sheet_paste(canvas, src[:, :, :5], [0], 0, 0, 'unit'),                     # 16 rows are no multiple of 5
           lambda: ops.sheet_paste(canvas, src[:, :, :, :5].contiguous(), [0], 0, 0, 'unit'),     # 24 columns are no multiple of 5
           lambda: ops.sheet_paste(canvas[..., :2].contiguous(), src, [0], 0, 0, 'unit'),         # a sheet has three channels
           lambda: ops.sheet_paste(canvas, torch.zeros((b, f, h, w, 2), device=DEV), [0], 0, 0, 'unit'),        # C = 2
           lambda: ops.sheet_paste(torch.zeros((1, 65, 1, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 1, 1, 1, 3), device=DEV), [0], 0, 0,
                                   'unit'),                                                       # 65 rows of cells
           lambda: ops.sheet_paste(torch.zeros((1, 1, 2050, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 1, 1, 1025, 3), device=DEV), [0],
                                   0, 0, 'unit'),                                                 # W = 1025
           lambda: ops.sheet_paste(canvas, src, [], 0, 0, 'unit'),                                # frames
           lambda: ops.sheet_paste(torch.zeros((1, 1, 64, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 1, 1, 1, 3), device=DEV), [0] * 65,
                                   0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [f], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [-1], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [0.5], 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src, 3, 0, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [0, 1], 0, 2, 'unit'),                            # col + J > cols
           lambda: ops.sheet_paste(canvas, src, [0], 0, 3, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [0], 0, -1, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [0], 2, 0, 'unit'),                               # row >= rows
           lambda: ops.sheet_paste(canvas, src, [0], -1, 0, 'unit'),
           lambda: ops.sheet_paste(canvas, src, [0], 0, 0, 'png'),                                # premap
           lambda: ops.sheet_paste(canvas, src, [0], 0, 0, 0)]
    from kpx_amd import _lib
    launched = _lib.abi_calls[0]
    for i, fn in enumerate(bad):
        with pytest.raises(KpxError):
            fn()
            pytest.fail('case %d raised nothing' % i)
    assert _lib.abi_calls[0] == launched                              # no entry was called ...
    assert bool((canvas == FILL).all()) and bool((wide == FILL).all())          # ... and nothing was written


def _png(path, mode=None):
    from PIL import Image
    im = Image.open(path)
    assert mode is None or im.mode == mode
    return np.asarray(im, np.uint8)


def test_evaluate_actions_end_to_end_on_the_fixture_videos(tmp_path, monkeypatch):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    from test_data_gpu import _fixture_dataset
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k, n_action = int(golden['n_points']), int(golden['n_action'])
    assert n_action == 9
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
    host = lambda t: None if t is None else t.detach().cpu().numpy().copy()

    def recording_run(self, sess, feed_dict, z=None):
        out = run(self, sess, feed_dict, z=z)
        calls.append({'z': host(z), 'act': host(feed_dict['action_code']), 'pred': host(out['pred_im_seq']), 'kp': host(out['fut_pt_raw']),
                      'cur': host(out.get('current_points')), 'fut': host(out.get('future_points'))})
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics']
    recorded = {}
    for name, extra in (('eval', ['--actions', '3,7,0,5', '--samples', '2']), ('nosave', ['--actions', '3,7,0,5', '--samples', '2', '--no-save']),
                        ('one', ['--actions', '5']), ('plain', ['--samples', '2'])):
        del calls[:]
        torch.manual_seed(11)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
        recorded[name] = list(calls)
    loader = kpx_amd.data.SequenceDataLoader(str(data), 'test', n_points=k, n_action=n_action, random_order=False, randomness=False,
                                             with_image_seq=True)
    batches = [{key: b[key].cpu().numpy() for key in ('image', 'real_im_seq', 'real_seq', 'action_code')}
               for b in loader.batches(2, DEV, repeat=False, num_preprocess_threads=2)]
    assert [b['image'].shape[0] for b in batches] == [2, 1]                              # batches of 2 and 1
    actions, n_cls, n_draws, res = [3, 7, 0, 5], 4, 2, 128
    eye = np.eye(n_action, dtype=np.float32)

    # ---- every sweep run of a (batch, draw) got the own run's z and the one-hot row of its class; the next draw another z
    rec = recorded['eval']
    assert len(rec) == len(batches) * n_draws * (1 + n_cls)
    group = lambda b, d: rec[(b * n_draws + d) * (1 + n_cls):(b * n_draws + d + 1) * (1 + n_cls)]
    for b, batch in enumerate(batches):
        bsz = batch['image'].shape[0]
        for d in range(n_draws):
            own, sweep = group(b, d)[0], group(b, d)[1:]
            assert own['z'] is not None and own['z'].shape == (bsz, 8) and np.array_equal(own['act'], batch['action_code'])
            for a, call in zip(actions, sweep):
                assert np.array_equal(call['z'], own['z']) and np.array_equal(call['act'], np.repeat(eye[a:a + 1], bsz, axis=0))
        assert not np.array_equal(group(b, 0)[0]['z'], group(b, 1)[0]['z'])
    assert all(c['z'] is None for c in recorded['plain']) and len(recorded['plain']) == len(batches) * n_draws

    # ---- the sheets of each sample: the restatement's paste of the recorded tensors, and the PNGs of the sample's own rollout
    ev = tmp_path / 'eval'
    samples = sorted(n for n in os.listdir(str(ev)) if n.isdigit())
    assert samples == ['0000', '0001', '0002']
    cols = 1 + len(SHEET_FRAMES)
    own_class, s = [], 0
    for b, batch in enumerate(batches):
        sweep = group(b, 0)[1:]
        for i in range(batch['image'].shape[0]):
            d = ev / samples[s]
            image = batch['image'][i:i + 1, None]
            want = np.zeros((1, (1 + n_cls) * res, cols * res, 3), np.uint8)
            R.paste(want, image, [0], 0, 0, 'unit')
            R.paste(want, batch['real_im_seq'][i:i + 1], SHEET_FRAMES, 0, 1, 'unit')
            want_pts = np.zeros((1, n_cls * res, cols * res, 3), np.uint8)
            for a, call in enumerate(sweep):
                R.paste(want, image, [0], 1 + a, 0, 'unit')
                R.paste(want, call['pred'][i:i + 1], SHEET_FRAMES, 1 + a, 1, 'unit')
                R.paste(want_pts, call['cur'][i:i + 1, None], [0], a, 0, 'raw')
                R.paste(want_pts, call['fut'][i:i + 1], SHEET_FRAMES, a, 1, 'raw')
            sheet, pts = _png(str(d / 'classes.png'), 'RGB'), _png(str(d / 'classes_points.png'), 'RGB')
            assert sheet.shape == ((1 + n_cls) * res, cols * res, 3) and pts.shape == (n_cls * res, cols * res, 3)
            assert np.array_equal(sheet, want[0]) and np.array_equal(pts, want_pts[0]), samples[s]
            assert pts.max() > 0 and len(np.unique(sheet)) > 16
            own = int(batch['action_code'][i].argmax())
            own_class.append(own)
            r = actions.index(own)
            cell = lambda img, row, col: img[row * res:(row + 1) * res, col * res:(col + 1) * res]
            for row in range(1 + n_cls):
                assert np.array_equal(cell(sheet, row, 0), _png(str(d / 'input_im.png')))
            assert np.array_equal(cell(pts, r, 0), _png(str(d / 'current_points.png')))
            for j, fr in enumerate(SHEET_FRAMES):
                assert np.array_equal(cell(sheet, 0, 1 + j), _png(str(d / 'real_seq' / ('%06d.png' % fr))))
                assert np.array_equal(cell(sheet, 1 + r, 1 + j), _png(str(d / 'pred_seq' / ('%06d.png' % fr)))), (samples[s], fr)
                assert np.array_equal(cell(pts, r, 1 + j), _png(str(d / 'pred_points' / ('%06d.png' % fr)))), (samples[s], fr)
            s += 1
    assert own_class == [3, 7, 0]
    assert json.loads((ev / 'actions.json').read_text()) == {'actions': actions, 'sheet_frames': SHEET_FRAMES, 'rows': ['real', 3, 7, 0, 5],
                                                             'points_rows': actions, 'cell': [res, res]}

    # ---- the class scores against the restatements on the recorded key points and frames
    npz = np.load(str(ev / 'metrics.npz'))
    assert sorted(npz.files) == ['act_div_mse', 'act_kp_div', 'act_kp_l2', 'act_own', 'act_rank', 'actions', 'mse', 'psnr', 'ssim']
    want = {'l2': [], 'div': [], 'mse': []}
    for b, batch in enumerate(batches):
        bsz = batch['image'].shape[0]
        kp = np.stack([np.stack([c['kp'] for c in group(b, d)[1:]]) for d in range(n_draws)])        # [D, A, B, 32, K, 2]
        l2, _ = M.keypoint_draw_metrics(kp.reshape((n_draws * n_cls,) + kp.shape[2:]), batch['real_seq'])
        want['l2'].append(l2.reshape(n_draws, n_cls, bsz, 32).transpose(2, 1, 0, 3))
        want['div'].append(np.stack([M.keypoint_draw_metrics(kp[d], batch['real_seq'])[1] for d in range(n_draws)]).transpose(1, 0, 2))
        div_mse = []
        for d in range(n_draws):
            s_, ss_ = M.moments([c['pred'] for c in group(b, d)[1:]])
            div_mse.append(M.draw_diversity(s_, ss_, n_cls, (res, res, 3))[0].reshape(bsz, 32))
        want['mse'].append(np.stack(div_mse).transpose(1, 0, 2))
    want = {key: np.concatenate(v) for key, v in want.items()}
    assert npz['act_kp_l2'].shape == (3, n_cls, n_draws, 32) and npz['act_kp_div'].shape == (3, n_draws, 32) == npz['act_div_mse'].shape
    assert all(npz[key].dtype == np.float32 for key in ('act_kp_l2', 'act_kp_div', 'act_div_mse'))
    assert all(npz[key].dtype == np.int32 for key in ('actions', 'act_own', 'act_rank'))
    assert M.within_one_ulp(npz['act_kp_l2'], want['l2']) and M.within_one_ulp(npz['act_kp_div'], want['div'])
    assert np.array_equal(npz['act_div_mse'].view(np.uint32), want['mse'].view(np.uint32))
    assert npz['act_kp_div'].max() > 0
    assert npz['act_own'].tolist() == [3, 7, 0] and npz['actions'].tolist() == actions
    score, rank = evaluate.action_ranks(npz['actions'], npz['act_own'], npz['act_kp_l2'])
    assert np.array_equal(npz['act_rank'], rank) and (rank >= 0).all()
    summary = json.loads((ev / 'metrics.json').read_text())
    block = evaluate.summarise_actions(npz['actions'], npz['act_own'], npz['act_kp_l2'], npz['act_kp_div'], npz['act_div_mse'])
    assert summary['actions'] == json.loads(json.dumps(block, allow_nan=False))
    assert block['n_ranked'] == 3 and block['chance'] == 0.25 and np.sum(block['confusion']) == 3
    assert not any(key.startswith('act') for key in summary if key != 'actions')         # summarise_metrics gained nothing

    # ---- one class that no sample has: nothing ranked, no diversity, sheets of two rows and one
    one = tmp_path / 'one'
    npz1 = np.load(str(one / 'metrics.npz'))
    assert sorted(npz1.files) == ['act_kp_l2', 'act_own', 'act_rank', 'actions', 'mse', 'psnr', 'ssim']
    assert npz1['act_kp_l2'].shape == (3, 1, 1, 32) and npz1['act_rank'].tolist() == [-1, -1, -1]
    blk1 = json.loads((one / 'metrics.json').read_text())['actions']
    assert blk1['n_ranked'] == 0 and blk1['top1'] is None and blk1['mean_rank'] is None and 'kp_div' not in blk1 and 'div_mse' not in blk1
    for name in samples:
        assert _png(str(one / name / 'classes.png')).shape == (2 * res, cols * res, 3)
        assert _png(str(one / name / 'classes_points.png')).shape == (res, cols * res, 3)
    assert json.loads((one / 'actions.json').read_text())['rows'] == ['real', 5]

    # ---- --no-save: the same scores under the same seed, and only the two score files
    assert sorted(os.listdir(str(tmp_path / 'nosave'))) == ['metrics.json', 'metrics.npz']
    npz2 = np.load(str(tmp_path / 'nosave' / 'metrics.npz'))
    assert sorted(npz2.files) == sorted(npz.files)
    for key in npz.files:
        assert np.array_equal(npz[key], npz2[key]), key

    # ---- without --actions: the files and scores of before
    plain = tmp_path / 'plain'
    assert sorted(os.listdir(str(plain))) == ['0000', '0001', '0002', 'metrics.json', 'metrics.npz']
    for name in samples:
        assert sorted(os.listdir(str(plain / name))) == ['crude', 'current_points.png', 'input_im.png', 'mask', 'pred_points', 'pred_seq', 'real_seq']
    assert sorted(np.load(str(plain / 'metrics.npz')).files) == ['mse', 'psnr', 'ssim']
    assert 'actions' not in json.loads((plain / 'metrics.json').read_text())


def test_evaluate_actions_on_synthetic_inputs(tmp_path, monkeypatch):
    """--synthetic has no real frames: sheets without the real row, at chosen frames, and no scores"""
    import yaml
    import kpx_amd
    import evaluate
    k, n_action, res = 5, 6, 128
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    calls = []
    run = kpx_amd.FinalModel.run
    host = lambda t: t.detach().cpu().numpy().copy()

    def recording_run(self, sess, feed_dict, z=None):
        out = run(self, sess, feed_dict, z=z)
        calls.append({key: host(v) for key, v in (('z', z), ('image', feed_dict['image']), ('act', feed_dict['action_code']),
                                                  ('pred', out['pred_im_seq']), ('cur', out['current_points']), ('fut', out['future_points']))})
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    actions, frames = [4, 1], [0, 31]
    ev = tmp_path / 'eval'
    evaluate.main(['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--synthetic', '3',
                   '--actions', '4,1', '--sheet-frames', '0,31', '--save_dir', str(ev)])
    assert len(calls) == 2 * 3 and sorted(os.listdir(str(ev))) == ['0000', '0001', '0002', 'actions.json']
    assert json.loads((ev / 'actions.json').read_text()) == {'actions': actions, 'sheet_frames': frames, 'rows': actions, 'points_rows': actions,
                                                             'cell': [res, res]}
    eye, s = np.eye(n_action, dtype=np.float32), 0
    for b in range(2):
        own, sweep = calls[3 * b], calls[3 * b + 1:3 * b + 3]
        bsz = own['image'].shape[0]
        for a, call in zip(actions, sweep):
            assert np.array_equal(call['z'], own['z']) and np.array_equal(call['image'], own['image'])
            assert np.array_equal(call['act'], np.repeat(eye[a:a + 1], bsz, axis=0))
        for i in range(bsz):
            want, want_pts = (np.zeros((1, 2 * res, 3 * res, 3), np.uint8) for _ in range(2))
            for r, call in enumerate(sweep):
                R.paste(want, own['image'][i:i + 1, None], [0], r, 0, 'unit')
                R.paste(want, call['pred'][i:i + 1], frames, r, 1, 'unit')
                R.paste(want_pts, call['cur'][i:i + 1, None], [0], r, 0, 'raw')
                R.paste(want_pts, call['fut'][i:i + 1], frames, r, 1, 'raw')
            d = ev / ('%04d' % s)
            assert np.array_equal(_png(str(d / 'classes.png'), 'RGB'), want[0]) and np.array_equal(_png(str(d / 'classes_points.png'), 'RGB'), want_pts[0])
            assert sorted(os.listdir(str(d))) == ['classes.png', 'classes_points.png', 'crude', 'current_points.png', 'input_im.png', 'mask',
                                                  'pred_points', 'pred_seq']
            s += 1
    assert s == 3
