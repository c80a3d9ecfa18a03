"""GPU: animate.py end to end on the tiny configuration of test_gif_gpu.py -- the class sweep of three stills (the seeded z shared by
stills and classes, classes.gif and classes_overlay.gif against the restated pipeline cells_ref -> gif_ref on the recorded rollouts, the
PNG folders, the sheets, animate.json, and a second run byte for byte) and a driven run (the 33 frames read, the drive dict, driven.gif and
driven_overlay.gif)."""
import json
import os

import numpy as np
import pytest
import torch

import cells_ref as C
import gif_ref as G
import sheet_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
RES, T = 128, 33
SHEET_FRAMES = [3, 7, 11, 15, 19, 23, 27, 31]
KEYS = ('im', 'pred_im_seq', 'mask', 'pred_im_crude', 'current_points', 'future_points', 'first_pt', 'fut_pt_raw')


def _tiny_config(tmp_path, k, n_action):
    import yaml
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    return cfg, cfg_path


def _checkpoint(cfg, tmp_path):
    import kpx_amd
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    return fm.save_checkpoint(None, 0)


def _picture(w, h, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([255.0 * x / max(1, w - 1), 255.0 * y / max(1, h - 1), 127.0 + 127.0 * np.sin(x / 9.0 + seed) * np.cos(y / 7.0)], axis=-1)
    a[h // 4:h // 2, w // 3:w // 2] = rs.randint(0, 256, size=3)
    return np.clip(a + rs.normal(0, 6, size=a.shape), 0, 255).astype(np.uint8)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def _record(monkeypatch):
    """FinalModel.run and FinalModel.detect wrapped: every call's inputs and outputs on the host, while ``log['on']``"""
    import kpx_amd
    log = {'on': True, 'runs': [], 'detects': [], 'colors': None}
    run, detect = kpx_amd.FinalModel.run, kpx_amd.FinalModel.detect
    host = lambda v: v.detach().cpu().numpy().copy() if isinstance(v, torch.Tensor) else v

    def recording_run(self, sess, feed_dict, z=None, drive=None):
        out = run(self, sess, feed_dict, z=z, drive=drive)
        if log['on']:
            log['colors'] = np.asarray(self.colors)
            log['runs'].append({'z': host(z), 'action_code': host(feed_dict.get('action_code')),
                                'drive': None if drive is None else {k: host(v) for k, v in drive.items()},
                                'out': {k: host(out[k]) for k in KEYS}})
        return out

    def recording_detect(self, image):
        pts = detect(self, image)
        if log['on']:
            log['detects'].append((host(image), host(pts)))
        return pts

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    monkeypatch.setattr(kpx_amd.FinalModel, 'detect', recording_detect)
    return log


def _check_gif(path, canvas, delay, dither):
    """the file, decoded by PIL, is palette[idx] of the restated quantiser on the restated canvas -> the palette size"""
    idx, pal = G.quantise(canvas, dither)
    frames, durations, loop = G.decode_gif(path)
    assert frames.shape == canvas.shape and durations == [10 * delay] * T and loop == 0
    assert np.array_equal(frames, pal[idx]), path
    return int(pal.shape[0])


def _marks(out, b):
    k = out['fut_pt_raw'].shape[2]
    return out['first_pt'].reshape(-1, k, 2)[b:b + 1], out['fut_pt_raw'][b:b + 1]


def test_class_sweep_of_three_stills(tmp_path, monkeypatch):
    from PIL import Image
    import animate
    import evaluate
    cfg, cfg_path = _tiny_config(tmp_path, 5, 3)
    ckpt = _checkpoint(cfg, tmp_path)
    pics = tmp_path / 'pics'
    pics.mkdir()
    Image.fromarray(_picture(200, 150, 1)).save(str(pics / 'a.jpg'), quality=90)
    rgba = Image.fromarray(_picture(128, 128, 2))
    rgba.putalpha(Image.fromarray((np.arange(128 * 128).reshape(128, 128) % 256).astype(np.uint8)))
    rgba.save(str(pics / 'b.png'))
    Image.fromarray(_picture(90, 260, 3)).convert('L').save(str(pics / 'c.png'))
    log = _record(monkeypatch)
    actions, samples, seed, fps, radius = [0, 2], 2, 7, 20, 3
    argv = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--images', str(pics), '--actions', '0,2',
            '--samples', str(samples), '--seed', str(seed), '--overlay', str(radius), '--png', '--gif-fps', str(fps)]
    out_dir = str(tmp_path / 'one')
    animate.main(argv + ['--save_dir', out_dir])
    log['on'] = False
    runs, n = log['runs'], 3
    assert len(runs) == samples * len(actions) and not log['detects']
    zs = np.random.RandomState(seed).randn(samples, 8).astype(np.float32)
    for i, r in enumerate(runs):                                       # draw-major, the classes in list order; one z per draw for all
        s, a = divmod(i, len(actions))
        assert r['drive'] is None and np.array_equal(r['z'], np.repeat(zs[s:s + 1], n, axis=0))
        assert np.array_equal(r['action_code'], np.repeat(np.eye(3, dtype=np.float32)[actions[a]][None], n, axis=0))
    colors = C.quantise_colors(log['colors'])
    delay = int(round(100.0 / fps))
    meta = json.loads(open(os.path.join(out_dir, 'animate.json')).read())
    expected = tmp_path / 'expected'
    for b in range(n):
        d = os.path.join(out_dir, '%04d' % b)
        plain = np.full((1, T, samples * RES, len(actions) * RES, 3), 0xA5, np.uint8)
        marked = plain.copy()
        for i, r in enumerate(runs):
            s, a = divmod(i, len(actions))
            o = r['out']
            C.cell_frames(plain, o['im'][b:b + 1], o['pred_im_seq'][b:b + 1], s, a, 'unit')
            C.cell_frames(marked, o['im'][b:b + 1], o['pred_im_seq'][b:b + 1], s, a, 'unit', *_marks(o, b), colors, radius)
            want = str(expected / ('%d_%d' % (b, i)))
            got = os.path.join(d, 'draw_%02d' % s, 'class_%02d' % actions[a])
            for name, key, rescale in (('pred_seq', 'pred_im_seq', True), ('mask', 'mask', False), ('crude', 'pred_im_crude', True),
                                       ('pred_points', 'future_points', False)):
                folder = os.path.join(got, name)
                assert sorted(os.listdir(folder)) == ['%06d.png' % t for t in range(T - 1)]
                pixels = np.stack([np.asarray(Image.open(os.path.join(folder, f))) for f in sorted(os.listdir(folder))])
                q = (S.unit8 if rescale else S.raw8)(o[key][b])                                      # the bytes of _save_img (test_actions_cpu.py)
                assert np.array_equal(pixels, q[..., 0] if q.shape[-1] == 1 else q), (b, i, name)
                if (b, i) == (0, 0):                                                                 # and one rollout file by file
                    evaluate._save_img_sequence(os.path.join(want, name), o[key][b], rescale=rescale)
                    assert _files(folder) == _files(os.path.join(want, name))
            assert sorted(os.listdir(got)) == ['crude', 'mask', 'pred_points', 'pred_seq']
        assert np.array_equal(plain[0, 0, :RES, :RES], plain[0, 0, RES:, RES:])                      # frame 0 is the still in every cell
        assert (marked != plain).any()
        sizes = (_check_gif(os.path.join(d, 'classes.gif'), plain[0], delay, 0), _check_gif(os.path.join(d, 'classes_overlay.gif'), marked[0], delay, 0))
        assert (meta['palette_sizes']['classes'][b], meta['palette_sizes']['classes_overlay'][b]) == sizes
        assert np.array_equal(np.asarray(Image.open(os.path.join(d, 'overlay.png'))), marked[0, 0, :RES, :RES])
        o = runs[0]['out']
        evaluate._save_img(str(expected / 'input_im.png'), o['im'][b], rescale=True)
        evaluate._save_img(str(expected / 'current_points.png'), o['current_points'][b], rescale=False)
        for name in ('input_im.png', 'current_points.png'):
            assert open(os.path.join(d, name), 'rb').read() == open(str(expected / name), 'rb').read()
        sheet = np.zeros((1, len(actions) * RES, 9 * RES, 3), np.uint8)                              # the sheets of evaluate.py --actions, draw 0
        points = np.zeros_like(sheet)
        for a in range(len(actions)):
            o = runs[a]['out']
            S.paste(sheet, o['im'][b:b + 1, None], [0], a, 0, 'unit')
            S.paste(sheet, o['pred_im_seq'][b:b + 1], SHEET_FRAMES, a, 1, 'unit')
            S.paste(points, o['current_points'][b:b + 1, None], [0], a, 0, 'raw')
            S.paste(points, o['future_points'][b:b + 1], SHEET_FRAMES, a, 1, 'raw')
        assert np.array_equal(np.asarray(Image.open(os.path.join(d, 'classes.png'))), sheet[0])
        assert np.array_equal(np.asarray(Image.open(os.path.join(d, 'classes_points.png'))), points[0])
    names = sorted(os.listdir(str(pics)))
    assert [os.path.basename(s['source']) for s in meta['stills']] == names == ['a.jpg', 'b.png', 'c.png']
    assert [s['decoded_size'] for s in meta['stills']] == [[200, 150], [128, 128], [90, 260]] and all(s['box'] is None for s in meta['stills'])
    assert meta['actions'] == actions and meta['draws'] == samples and meta['seed'] == seed and meta['grid'] == [samples, len(actions)]
    assert meta['cell'] == [RES, RES] and meta['frames'] == T and meta['fps'] == fps and meta['delay_cs'] == delay and meta['dither'] == 0
    assert meta['overlay'] == radius and 'driver' not in meta and meta['sheet_frames'] == SHEET_FRAMES
    again = str(tmp_path / 'two')
    animate.main([v for v in argv if v != '--png'] + ['--save_dir', again])                          # the same seed: the same bytes
    first, second = _files(out_dir), _files(again)
    assert second == {name: data for name, data in first.items() if '/draw_' not in name}
    assert len(first) - len(second) == n * samples * len(actions) * 4 * (T - 1)


def test_driven_rollout_from_a_folder_of_frames(tmp_path, monkeypatch):
    from PIL import Image
    import animate
    from kpx_amd import stills
    from kpx_amd.data import _u8_to_unit_numpy
    cfg, cfg_path = _tiny_config(tmp_path, 5, 3)
    ckpt = _checkpoint(cfg, tmp_path)
    video = tmp_path / 'video'
    video.mkdir()
    for i in range(70):
        Image.fromarray(_picture(64, 48, 100 + i)).save(str(video / ('%03d.png' % i)))
    pics = [str(tmp_path / 'a.png'), str(tmp_path / 'b.jpg')]
    Image.fromarray(_picture(140, 128, 4)).save(pics[0])
    Image.fromarray(_picture(128, 131, 5)).save(pics[1], quality=90)
    log = _record(monkeypatch)
    out_dir, fps, dither, radius = str(tmp_path / 'out'), 10, 8, 2
    animate.main(['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--images'] + pics + ['--driver', str(video), '--overlay', str(radius),
                 '--gif-dither', str(dither), '--save_dir', out_dir])
    log['on'] = False
    n = len(pics)
    assert len(log['detects']) == 1 and len(log['runs']) == 1
    frames, pts = log['detects'][0]
    used = [str(video / ('%03d.png' % i)) for i in range(0, 66, 2)]                                  # frames 0, 2, ..., 64 of the 70
    assert np.array_equal(frames, _u8_to_unit_numpy(np.stack([stills.fit(p)[0] for p in used])))     # the loaders' upload, bit for bit
    run = log['runs'][0]
    drive, o = run['drive'], run['out']
    assert drive['mode'] == 'relative' and drive['shift'] == 0 and drive['scaled'] is False and run['z'] is None
    assert np.array_equal(drive['first'], np.repeat(pts[:1], n, axis=0)) and np.array_equal(drive['seq'], np.repeat(pts[None, 1:], n, axis=0))
    colors = C.quantise_colors(log['colors'])
    meta = json.loads(open(os.path.join(out_dir, 'animate.json')).read())
    for b in range(n):
        d = os.path.join(out_dir, '%04d' % b)
        plain = np.full((1, T, RES, 2 * RES, 3), 0xA5, np.uint8)
        C.cell_frames(plain, frames[:1], frames[None, 1:], 0, 0, 'unit')
        C.cell_frames(plain, o['im'][b:b + 1], o['pred_im_seq'][b:b + 1], 0, 1, 'unit')
        marked = plain.copy()
        C.cell_frames(marked, frames[:1], frames[None, 1:], 0, 0, 'unit', pts[:1], pts[None, 1:], colors, radius)
        C.cell_frames(marked, o['im'][b:b + 1], o['pred_im_seq'][b:b + 1], 0, 1, 'unit', *_marks(o, b), colors, radius)
        sizes = (_check_gif(os.path.join(d, 'driven.gif'), plain[0], 10, dither), _check_gif(os.path.join(d, 'driven_overlay.gif'), marked[0], 10, dither))
        assert (meta['palette_sizes']['driven'][b], meta['palette_sizes']['driven_overlay'][b]) == sizes
        assert sorted(os.listdir(d)) == ['current_points.png', 'driven.gif', 'driven_overlay.gif', 'input_im.png']
    assert meta['driver']['frames'] == list(range(0, 66, 2)) and meta['driver']['n_found'] == 70 and meta['driver']['mode'] == 'relative'
    assert meta['driver']['scaled'] is False and 'actions' not in meta and meta['dither'] == dither
