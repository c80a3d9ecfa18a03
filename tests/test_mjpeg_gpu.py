"""GPU: evaluate.py --video -- kpx_jpeg_encode_u8 byte for byte against the restatement (mjpeg_ref.py) on every fixture, packing across
frames and chunks, graph replay, and evaluate.main / animate.main --video end to end on synthetic inputs."""
import io
import json
import os

import numpy as np
import pytest
import torch

import mjpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FIXTURES = R.fixtures()
CASES = [(name, q) for name, (_, qs) in FIXTURES.items() for q in qs]
_want = {}


def _ops():
    from kpx_amd import ops
    return ops


def _ref(name, q):
    """the restatement's scan of a fixture, computed once"""
    if (name, q) not in _want:
        _want[name, q] = R.encode(FIXTURES[name][0], q)
    return _want[name, q]


def _dev(a, off=0):
    """a uint8 on the device, contiguous, its first byte ``off`` bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.uint8)
    buf = torch.empty(a.size + 16, dtype=torch.uint8, device=DEV)
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a).to(DEV))
    assert t.is_contiguous() and t.data_ptr() % 16 == off
    return t


@pytest.mark.parametrize('name,q', CASES)
def test_scan_is_the_restatement(name, q):
    img = FIXTURES[name][0]
    got = _ops().jpeg_encode(_dev(img[None]), q)
    assert len(got) == 1 and isinstance(got[0], bytes)
    assert got[0] == _ref(name, q)


def test_scan_from_an_odd_address_is_the_restatement():
    """a canvas that is not 4-byte aligned is read byte by byte: the same scan"""
    for name, q in (('noise', 75), ('cells', 100)):
        assert _ops().jpeg_encode(_dev(FIXTURES[name][0][None], off=3), q) == [_ref(name, q)]


@pytest.mark.parametrize('q', [50, 100])
def test_mixed_batch_offsets_and_packing(q):
    from kpx_amd._lib import lib
    ops = _ops()
    batch = R.mixed_batch()
    want = [R.encode(f, q) for f in batch]
    assert len(set(want)) == 5
    canvas = _dev(batch)
    assert ops.jpeg_encode(canvas, q) == want
    scans, offsets = ops.jpeg_scans(canvas, q)
    off = offsets.cpu().numpy()
    bound = lib.kpx_jpeg_scan_bound(32, 48)
    assert off.dtype == np.int64 and off[0] == 0 and (np.diff(off) > 0).all() and (np.diff(off) <= bound).all()
    assert scans.numel() == 5 * bound and bound == 6 * 6 * 416 + 2
    host = scans.cpu().numpy().tobytes()
    assert [host[off[i]:off[i + 1]] for i in range(5)] == want
    # through a chunk boundary: a budget of two frames' workspace and scans codes N = 5 as 2 + 2 + 1
    per = lib.kpx_jpeg_workspace_bytes(1, 32, 48) + bound
    calls = []
    inner = ops.jpeg_scans
    from kpx_amd import mjpeg
    try:
        mjpeg.jpeg_scans = lambda c, *a, **k: (calls.append(int(c.shape[0])), inner(c, *a, **k))[1]
        assert ops.jpeg_encode(canvas, q, budget=2 * per + per // 2) == want
    finally:
        mjpeg.jpeg_scans = inner
    assert calls == [2, 2, 1]


def test_wrapper_refuses_what_it_cannot_launch():
    from kpx_amd._lib import KpxError
    ops = _ops()
    canvas = _dev(R.mixed_batch())
    for bad, q in ((canvas[:, :, ::2], 75),                            # not contiguous: the checker's rule is to refuse
                   (canvas[:, :24], 75),                               # H = 24
                   (canvas.view(5, 32, 144), 75),
                   (canvas.cpu(), 75), (canvas.float(), 75), (canvas, 0), (canvas, 101), (canvas, 7.5)):
        with pytest.raises(KpxError):
            ops.jpeg_encode(bad, q)
    with pytest.raises(KpxError):
        ops.jpeg_encode(canvas, 75, budget=0)


def test_graph_replay_is_the_eager_result():
    ops = _ops()
    a, b = R.mixed_batch(), R.mixed_batch()[::-1].copy()
    canvas = _dev(a)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):                                    # the stream's scratch buffer exists before the capture
        scans, offsets = ops.jpeg_scans(canvas, 90)
    stream.synchronize()
    want = {n: ops.jpeg_encode(_dev(d), 90) for n, d in (('a', a), ('b', b))}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        ops.jpeg_scans(canvas, 90, scans, offsets)
    for n, d in (('a', a), ('b', b), ('a', a)):
        canvas.copy_(torch.from_numpy(d).to(DEV))
        scans.fill_(0x55)
        offsets.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        off, host = offsets.cpu().numpy(), scans.cpu().numpy().tobytes()
        assert [host[off[i]:off[i + 1]] for i in range(5)] == want[n], n
    assert want['a'] == [R.encode(f, 90) for f in a]


# ------------------------------------------------------------------------------------------------------------------ the tools
def _decode(jpeg):
    from PIL import Image
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    return np.asarray(im.convert('RGB'))


def _pil_round_trip(rgb, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, 'JPEG', quality=quality, subsampling=2, optimize=False)
    return _decode(buf.getvalue())


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


def test_evaluate_video_on_synthetic_inputs(tmp_path, capsys):
    import evaluate
    from kpx_amd import mjpeg
    from test_gif_gpu import _tiny_config, _checkpoint, _files, _png, _seq
    cfg, cfg_path = _tiny_config(tmp_path, 5, 6, tmp_path / 'none')
    ckpt = _checkpoint(cfg, tmp_path)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--synthetic', '2']
    for name, extra in (('video', ['--video', '--frames', '64', '--rate', '2']), ('plain', [])):
        torch.manual_seed(5)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    ev = str(tmp_path / 'video')
    meta = json.loads(open(os.path.join(ev, 'video.json')).read())
    assert meta['columns'] == ['pred', 'points'] and meta['fps'] == 10 and meta['quality'] == 90 and meta['frames'] == 33
    assert meta['cell'] == [128, 128] and len(meta['bytes']['pred']) == 2 == len(meta['bytes']['compare'])
    worst = 0.0
    for s in range(2):
        d = os.path.join(ev, '%04d' % s)
        for kind, n, w, fps in (('pred', 33, 128, 10), ('compare', 33, 256, 10), ('long', 129, 256, 20)):
            got_fps, h, ww, frames = mjpeg.read_avi(os.path.join(d, kind + '.avi'))
            assert (got_fps, h, ww, len(frames)) == (fps, 128, w, n), kind
            if kind != 'long':
                assert meta['bytes'][kind][s] == os.path.getsize(os.path.join(d, kind + '.avi'))
            decoded = [_decode(f) for f in frames]
            assert all(x.shape == (128, w, 3) for x in decoded)
            if kind == 'pred':                                         # against PIL's own encoder on the PNGs of the same run
                pngs = np.concatenate([_png(os.path.join(d, 'input_im.png'))[None], _seq(os.path.join(d, 'pred_seq'))])
                for png, mine in zip(pngs, decoded):
                    gap = _psnr(_pil_round_trip(png, 90), png) - _psnr(mine, png)
                    worst = max(worst, gap)
                    assert gap <= 0.05, gap
    print('largest PSNR shortfall against PIL on pred.avi: %.4f dB' % worst)
    with_video, without = _files(ev), _files(str(tmp_path / 'plain'))
    extra = sorted(set(with_video) - set(without))
    assert extra == sorted(['video.json', 'long.json'] + ['%04d/%s' % (s, k) for s in range(2)
                                                          for k in ('pred.avi', 'compare.avi', 'long.avi', 'long_points.npy')])
    for name, data in without.items():
        assert with_video[name] == data, name
    with pytest.raises(SystemExit):
        evaluate.main(base + ['--video', '--no-save', '--save_dir', str(tmp_path / 'none')])
    assert '--no-save' in capsys.readouterr().err and not os.path.exists(str(tmp_path / 'none'))


def test_animate_video_on_two_synthetic_stills(tmp_path):
    from PIL import Image
    import animate
    from kpx_amd import mjpeg
    from test_animate_gpu import _tiny_config, _checkpoint, _picture
    cfg, cfg_path = _tiny_config(tmp_path, 5, 3)
    ckpt = _checkpoint(cfg, tmp_path)
    pics = tmp_path / 'pics'
    pics.mkdir()
    for i in range(2):
        Image.fromarray(_picture(160, 140, i + 1)).save(str(pics / ('%d.png' % i)))
    out = str(tmp_path / 'out')
    animate.main(['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--images', str(pics), '--actions', '0,1,2',
                  '--samples', '2', '--overlay', '3', '--video', '--video-fps', '25', '--video-quality', '80', '--save_dir', out])
    meta = json.loads(open(os.path.join(out, 'animate.json')).read())
    assert meta['video']['fps'] == 25 and meta['video']['quality'] == 80 and sorted(meta['video']['bytes']) == ['classes', 'classes_overlay']
    for s in range(2):
        d = os.path.join(out, '%04d' % s)
        assert os.path.exists(os.path.join(d, 'classes.gif')) and os.path.exists(os.path.join(d, 'classes_overlay.gif'))
        for name in ('classes', 'classes_overlay'):
            fps, h, w, frames = mjpeg.read_avi(os.path.join(d, name + '.avi'))
            assert (fps, h, w, len(frames)) == (25, 2 * 128, 3 * 128, 33)
            assert meta['video']['bytes'][name][s] == os.path.getsize(os.path.join(d, name + '.avi'))
            decoded = [_decode(f) for f in frames]
            assert all(x.shape == (256, 384, 3) for x in decoded)
            if name == 'classes':                                      # frame 0 of every cell is the still: against PIL on the same canvas
                still = np.asarray(Image.open(os.path.join(d, 'input_im.png')).convert('RGB'))
                canvas = np.tile(still, (2, 3, 1))
                assert _psnr(decoded[0], canvas) >= _psnr(_pil_round_trip(canvas, 80), canvas) - 0.05
