"""GPU: kpx_points_resample_f32 and kpx_points_speed_f64 against tests/resample_ref.py (knots bit for bit, in-between frames to one fp32 ulp,
the 16-byte and the 4-byte path bit-equal, non-finite containment, the speed against longdouble), and FinalModel.run(frames=, rate=,
resample=) on the toy configuration: the chained segments, the resampled rollout, the graph replays and the driven rollout; evaluate.py
and animate.py --frames --rate end to end on synthetic inputs."""
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as R
from test_drive_gpu import B, CELLS, K, VDIM, _equal, _snap, _toy_arrays, _toy_feed, _toy_model

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BATCHES, POINTS, KNOTS, RATES = (1, 3), (1, 2, 15, 40), (1, 2, 3, 32, 96), (1, 2, 3, 5, 64)


def _ops():
    from kpx_amd import ops
    return ops


def _dev_at(a, off):
    """a on the device, contiguous, its first element ``off`` floats past a 16-byte boundary"""
    buf = torch.empty(a.size + 16, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return t


def _resample(first, seq, rate, mode, off):
    """through the wrapper, every pointer ``off`` floats past a 16-byte boundary (off = 1: the 4-byte path whatever K is)"""
    b, n, k, _ = seq.shape
    out = _dev_at(np.zeros((b, n * rate, k, 2), np.float32), off)
    got = _ops().points_resample(_dev_at(first, off), _dev_at(seq, off), rate, mode, out=out)
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize('k', POINTS)
@pytest.mark.parametrize('mode', ['linear', 'cubic'])
def test_resample_matches_the_restatement_on_both_paths(mode, k):
    rs = np.random.RandomState(100 + k)
    for b in BATCHES:
        for n in KNOTS:
            if mode == 'cubic' and n < 2:
                continue                                              # N = 1 is LINEAR's alone
            first = rs.uniform(-1, 1, (b, k, 2)).astype(np.float32)
            seq = rs.uniform(-1, 1, (b, n, k, 2)).astype(np.float32)
            for rate in RATES:
                want = R.resample(first, seq, rate, R.MODES[mode])
                wide = _resample(first, seq, rate, mode, 0)            # 16-byte accesses when K is even
                narrow = _resample(first, seq, rate, mode, 1)
                what = (mode, b, n, k, rate)
                assert wide.tobytes() == narrow.tobytes(), what
                assert wide[:, rate - 1::rate].tobytes() == seq.tobytes(), what          # the knots, bit for bit
                assert R.ulp_distance(wide, want).max() <= 1, what
                if rate == 1:
                    assert wide.tobytes() == seq.tobytes(), what


@pytest.mark.parametrize('mode', ['linear', 'cubic'])
def test_resample_keeps_payloads_and_contains_non_finite_knots(mode):
    n, rate = 6, 3
    for k, off in ((4, 0), (4, 1), (3, 0)):
        rs = np.random.RandomState(k + off)
        for knot in (0, 1, 3, 6):
            p = rs.uniform(-1, 1, (3, n + 1, k, 2)).astype(np.float32)
            p.view(np.uint32)[1, knot, 2, 0] = 0x7fc12345              # a NaN with a payload
            p[2, knot, 0, 1] = np.float32(-np.inf)
            got = _resample(p[:, 0], p[:, 1:], rate, mode, off)
            bad = np.zeros(got.shape, bool)
            for j in range(1, n * rate + 1):
                i, r = divmod(j, rate)
                bad[1, j - 1, 2, 0] = bad[2, j - 1, 0, 1] = (i == knot) if r == 0 else knot in R.stencil(i, n, R.MODES[mode])
            assert (~np.isfinite(got) == bad).all(), (k, off, knot)
            assert got[:, rate - 1::rate].tobytes() == p[:, 1:].tobytes()          # payload and sign included
            want = R.resample(p[:, 0], p[:, 1:], rate, R.MODES[mode])
            assert R.ulp_distance(got[~bad], want[~bad]).max() <= 1


def test_resample_reproduces_lines_and_the_wrapper_checks_its_tensors():
    from kpx_amd._lib import KpxError
    ops = _ops()
    n, rate = 4, 8                                                     # a power of two: every frame of the line is an fp32 number
    t = np.arange(0, n + 1, dtype=np.float64).reshape(1, -1, 1, 1)
    p0, v = np.array([0.25, -0.5]).reshape(1, 1, 1, 2), np.array([3.0, -5.0]).reshape(1, 1, 1, 2) / 64
    knots = np.broadcast_to(p0 + v * t, (2, n + 1, 2, 2)).astype(np.float32)
    tj = (np.arange(1, n * rate + 1) / rate).reshape(1, -1, 1, 1)
    want = np.broadcast_to(p0 + v * tj, (2, n * rate, 2, 2)).astype(np.float32)
    for mode in ('linear', 'cubic'):
        assert _resample(knots[:, 0], knots[:, 1:], rate, mode, 0).tobytes() == want.tobytes()
    first, seq = torch.zeros(2, 3, 2, device=DEV), torch.zeros(2, 4, 3, 2, device=DEV)
    for args, kw, text in (((first[:1], seq, 2), {}, 'first must be a contiguous'), ((first.double(), seq, 2), {}, 'first must be a contiguous'),
                           ((first, seq.transpose(1, 2).contiguous().transpose(1, 2), 2), {}, 'seq must be a contiguous'),
                           ((first, seq, 2), dict(out=torch.zeros(2, 4, 3, 2, device=DEV)), 'out must be a contiguous'),
                           ((first.cpu(), seq, 2), {}, 'no CPU fallback')):
        with pytest.raises(KpxError, match='points_resample: .*' + text):
            ops.points_resample(*args, **kw)


def test_speed_matches_longdouble_and_is_exact_on_lines():
    ops = _ops()
    rs = np.random.RandomState(7)
    for b in BATCHES:
        for k in POINTS + (1024,):
            for t in (1, 3, 32, 96):
                first = rs.uniform(-1, 1, (b, k, 2)).astype(np.float32)
                seq = rs.uniform(-1, 1, (b, t, k, 2)).astype(np.float32)
                for off, scale in ((0, 1.0), (1, 3.0)):
                    got = ops.points_speed(_dev_at(first, off), _dev_at(seq, off), scale)
                    assert got.dtype == torch.float64 and tuple(got.shape) == (b, t)
                    want = R.speed(first, seq, scale)
                    err = np.abs(got.cpu().numpy().astype(np.longdouble) - want)
                    assert (err <= (k + 4) * 2.0 ** -52 * np.abs(want)).all(), (b, k, t, off, float((err / np.abs(want)).max()))
    first = np.zeros((2, 3, 2), np.float32)
    step = np.array([3.0, 4.0], np.float32) / 64                       # |step| = 5 / 64
    seq = first[:, None] + step * np.arange(1, 6, dtype=np.float32).reshape(1, 5, 1, 1)
    seq[1] = first[1, None]                                            # sample 1 stands still
    got = ops.points_speed(torch.from_numpy(first).to(DEV), torch.from_numpy(seq).to(DEV), 2.0).cpu().numpy()
    assert (got[0] == 10.0 / 64).all() and (got[1] == 0.0).all()
    # a resampled line moves 1 / F as far per frame: scale = F keeps the unit
    fine = ops.points_resample(torch.from_numpy(first).to(DEV), torch.from_numpy(seq).to(DEV), 4, 'cubic')
    assert (ops.points_speed(torch.from_numpy(first).to(DEV), fine, 4.0).cpu().numpy()[0] == 5.0 / 64).all()


# ------------------------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope='module')
def toy():
    """the toy FinalModel, its feed, z [3,B,V] and the plain rollout of z[0] (computed once, never changed)"""
    fm = _toy_model(_toy_arrays())
    feed, z, _ = _toy_feed()
    z3 = torch.cat([z[None], torch.from_numpy(np.random.RandomState(61).randn(2, B, VDIM).astype(np.float32)).to(DEV)])
    plain = _snap(fm.run(None, feed, z=z))
    return fm, feed, z3, plain


def test_run_with_the_default_frames_and_rate_is_todays_rollout(toy):
    fm, feed, z3, plain = toy
    graphs = set(fm._graphs)
    for call in range(3):
        assert _equal(_snap(fm.run(None, feed, z=z3[0], frames=32, rate=1, resample='linear')), plain), call
        assert _equal(_snap(fm.run(None, feed, z=z3[0])), plain), call
    assert {key for key in fm._graphs if key not in graphs} <= {(tuple(feed['image'].shape), tuple(feed['action_code'].shape), 0)}


def test_a_chained_rollout_is_its_segments(toy):
    from kpx_amd import networks, variables
    fm, feed, z3, plain = toy
    runs = [_snap(fm.run(None, feed, z=z3, frames=96)) for _ in range(3)]              # eager, capture + replay, replay
    got = runs[0]
    assert got['fut_pt_raw'].shape == (B, 96, K, 2) and got['pred_im_seq'].shape[:2] == (B, 96) and got['mask'].shape[:2] == (B, 96)
    for call in (1, 2):
        assert _equal(runs[call], got), call
    assert not fm._graph_failed
    assert np.array_equal(got['fut_pt_raw'][:, :32], plain['fut_pt_raw']) and np.array_equal(got['first_pt'], plain['first_pt'])
    assert np.array_equal(got['pred_im_seq'][:, :32], plain['pred_im_seq'])          # frames_per_launch = 32: the same slabs
    pose = torch.from_numpy(got['fut_pt_raw'][:, 31]).to(DEV).reshape(B, 2 * K).contiguous()
    with variables.as_default(fm.store), torch.no_grad():
        seg = networks.vae_decoder(z3[1].contiguous(), pose, feed['action_code'], list(CELLS), VDIM, K)
    assert np.array_equal(got['fut_pt_raw'][:, 32:64], seg.reshape(B, 32, K, 2).cpu().numpy())
    assert not np.array_equal(got['fut_pt_raw'][:, 32:64], got['fut_pt_raw'][:, 64:])
    # frames 33..64 are rendered from the source image and the pose, like any frame: a one-segment drive on them gives the same pictures
    driven = _snap(fm.run(None, feed, drive={'mode': 'absolute', 'seq': torch.from_numpy(got['fut_pt_raw'][:, 32:64]).to(DEV), 'shift': 0}))
    assert np.array_equal(driven['pred_im_seq'], got['pred_im_seq'][:, 32:64])


def test_a_resampled_rollout_keeps_the_knots(toy):
    fm, feed, z3, plain = toy
    rel_l2 = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
    for mode in ('cubic', 'linear'):
        runs = [_snap(fm.run(None, feed, z=z3[0], rate=3, resample=mode)) for _ in range(3)]
        got = runs[0]
        assert got['fut_pt_raw'].shape == (B, 96, K, 2) and got['pred_im_seq'].shape[:2] == (B, 96)
        for call in (1, 2):
            assert _equal(runs[call], got), (mode, call)
        assert np.array_equal(got['fut_pt_raw'][:, 2::3], plain['fut_pt_raw'])
        want = R.resample(plain['first_pt'].reshape(B, K, 2), plain['fut_pt_raw'], 3, R.MODES[mode])
        assert R.ulp_distance(got['fut_pt_raw'], want).max() <= 1
        for key in ('pred_im_seq', 'pred_im_crude', 'mask'):
            err = rel_l2(got[key][:, 2::3], plain[key])
            print('%s rate 3 %s at the knots: rel-L2 %.3g' % (mode, key, err))
            assert err < 1e-6, (mode, key)
    lin, cub = (_snap(fm.run(None, feed, z=z3[0], rate=3, resample=m))['fut_pt_raw'] for m in ('linear', 'cubic'))
    assert not np.array_equal(lin, cub)
    assert not fm._graph_failed


def test_chained_and_resampled_with_slabs_inside_a_sample(toy):
    """frames * rate = 128 > frames_per_launch = 32 x 2: a sample's frames span several slabs; the pictures match the 32-frame slabs'"""
    fm, feed, z3, plain = toy
    got = _snap(fm.run(None, feed, z=z3[:2], frames=64, rate=2))
    fm.frames_per_launch = 48                                          # 128 frames in slabs of 48, 48, 32: no multiple of anything
    try:
        odd = _snap(fm.run(None, feed, z=z3[:2], frames=64, rate=2))   # the same key: eager once more is not promised, so compare values
    finally:
        fm.frames_per_launch = 32
    assert got['pred_im_seq'].shape[:2] == (B, 128) and np.array_equal(got['fut_pt_raw'][:, 1:64:2], plain['fut_pt_raw'])
    assert np.array_equal(got['fut_pt_raw'], odd['fut_pt_raw'])
    rel_l2 = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
    assert rel_l2(odd['pred_im_seq'], got['pred_im_seq']) < 1e-6 and rel_l2(got['pred_im_seq'][:, 1:64:2], plain['pred_im_seq']) < 1e-6


def test_run_refuses_bad_frames_rate_and_z(toy):
    from kpx_amd._lib import KpxError
    fm, feed, z3, plain = toy
    for kw, text in ((dict(frames=48), 'frames must be a positive multiple of 32'), (dict(rate=0), 'rate must be'), (dict(rate=65), 'rate must be'),
                     (dict(resample='nearest'), 'resample must be one of'), (dict(frames=64, z=z3[0]), 'z must be an fp32 tensor \\[2, 2, 8\\]'),
                     (dict(frames=64, z=z3), 'z must be an fp32 tensor'), (dict(rate=2, z=z3), 'z must be an fp32 tensor \\[1, 2, 8\\]'),
                     (dict(frames=64, drive={'mode': 'hold'}), 'frames must be 32 with drive=')):
        with pytest.raises(KpxError, match='FinalModel.run: ' + text):
            fm.run(None, feed, **kw)
    assert _equal(_snap(fm.run(None, feed, z=z3[0])), plain)


def test_a_driven_rollout_takes_a_rate(toy):
    fm, feed, z3, plain = toy
    rs = np.random.RandomState(12)
    seq = torch.from_numpy(rs.uniform(-1, 1, (B, 32, K, 2)).astype(np.float32)).to(DEV)
    drive = {'mode': 'absolute', 'seq': seq, 'shift': 1}
    base = _snap(fm.run(None, feed, drive=drive))
    runs = [_snap(fm.run(None, feed, drive=drive, rate=2, resample='linear')) for _ in range(3)]
    for call in (1, 2):
        assert _equal(runs[call], runs[0]), call
    got = runs[0]
    assert got['fut_pt_raw'].shape == (B, 64, K, 2) and np.array_equal(got['fut_pt_raw'][:, 1::2], base['fut_pt_raw'])
    want = R.resample(base['first_pt'].reshape(B, K, 2), base['fut_pt_raw'], 2, R.LINEAR)
    assert R.ulp_distance(got['fut_pt_raw'], want).max() <= 1
    assert _equal(_snap(fm.run(None, feed, drive=drive)), base) and not fm._graph_failed


# ------------------------------------------------------------------------------------------------------------------ the tools
def _gif(path):
    """-> (number of frames, the frames' durations in ms, the size) as PIL reads the file"""
    from PIL import Image, ImageSequence
    with Image.open(path) as im:
        durations = [f.info['duration'] for f in ImageSequence.Iterator(im)]
        return len(durations), durations, im.size


def test_evaluate_writes_the_long_rollout_beside_an_untouched_run(tmp_path, capsys):
    import evaluate
    from test_gif_gpu import _checkpoint, _files, _tiny_config
    k = 5
    cfg, cfg_path = _tiny_config(tmp_path, k, 6, tmp_path / 'none')
    ckpt = _checkpoint(cfg, tmp_path)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--synthetic', '3', '--gif']
    for name, extra in (('long', ['--frames', '64', '--rate', '2']), ('plain', [])):
        torch.manual_seed(5)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    with_long, without = _files(str(tmp_path / 'long')), _files(str(tmp_path / 'plain'))
    assert sorted(set(with_long) - set(without)) == sorted(['long.json'] + ['%04d/%s' % (s, n) for s in range(3) for n in ('long.gif', 'long_points.npy')])
    for name, data in without.items():
        assert with_long[name] == data, name                            # every file of the ordinary run, byte for byte
    meta = json.loads(open(str(tmp_path / 'long' / 'long.json')).read())
    assert (meta['frames'], meta['rate'], meta['resample'], meta['n_frames'], meta['fps'], meta['delay_cs'], meta['n_samples']) == (64, 2, 'cubic', 128, 20, 5, 3)
    speed = np.array(meta['speed'], np.float64)
    assert speed.shape == (128,) and np.isfinite(speed).all() and (speed > 0).all()
    assert isinstance(meta['seam_ratio'], float) and np.isfinite(meta['seam_ratio'])
    assert meta['seam_ratio'] == speed[64] / np.delete(speed, 64).mean()
    mean = np.zeros(128, np.float64)
    for s in range(3):
        d = str(tmp_path / 'long' / ('%04d' % s))
        n, durations, size = _gif(os.path.join(d, 'long.gif'))
        assert n == 129 and durations == [50] * 129 and size == (256, 128)          # the input, then 128 frames of pred | points
        pts = np.load(os.path.join(d, 'long_points.npy'))
        assert pts.shape == (128, k, 2) and pts.dtype == np.float32 and np.isfinite(pts).all()
        n32, _, _ = _gif(os.path.join(d, 'pred.gif'))
        assert n32 == 33
    for argv, text in ((['--frames', '64', '--gif-fps', '30', '--rate', '2'], '--gif-fps'), (['--frames', '48'], '--frames'), (['--rate', '65'], '--rate')):
        with pytest.raises(SystemExit):
            evaluate.main(base + argv + ['--save_dir', str(tmp_path / 'none')])
        assert text in capsys.readouterr().err and not os.path.exists(str(tmp_path / 'none'))


def test_animate_writes_longer_and_smoother_grids(tmp_path):
    from PIL import Image
    import animate
    from test_animate_gpu import _checkpoint, _picture, _tiny_config
    cfg, cfg_path = _tiny_config(tmp_path, 5, 3)
    ckpt = _checkpoint(cfg, tmp_path)
    pics = tmp_path / 'pics'
    pics.mkdir()
    Image.fromarray(_picture(200, 150, 1)).save(str(pics / 'a.png'))
    argv = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--images', str(pics), '--actions', '0,2', '--seed', '7']
    animate.main(argv + ['--save_dir', str(tmp_path / 'plain')])
    animate.main(argv + ['--frames', '64', '--rate', '2', '--sheet-frames', '63,127', '--save_dir', str(tmp_path / 'long')])
    n, durations, size = _gif(str(tmp_path / 'plain' / '0000' / 'classes.gif'))
    assert n == 33 and durations == [100] * 33 and size == (256, 128)
    n, durations, size = _gif(str(tmp_path / 'long' / '0000' / 'classes.gif'))
    assert n == 129 and durations == [50] * 129 and size == (256, 128)              # 128 frames at twice the rate
    meta = json.loads(open(str(tmp_path / 'long' / 'animate.json')).read())
    assert meta['frames'] == 129 and meta['fps'] == 20 and meta['rollout'] == {'frames': 64, 'rate': 2, 'resample': 'cubic', 'gif_fps': 10}
    assert meta['sheet_frames'] == [63, 127]
    assert Image.open(str(tmp_path / 'long' / '0000' / 'classes.png')).size == (3 * 128, 2 * 128)
    plain = json.loads(open(str(tmp_path / 'plain' / 'animate.json')).read())
    assert plain['frames'] == 33 and 'rollout' not in plain
