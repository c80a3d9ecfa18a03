"""GPU: evaluate.py --gif -- kpx_color_hist_add_u32 and kpx_palette_map_u8 bit for bit against the restatement (gif_ref.py), graph replay,
the wrappers' argument errors, and evaluate.main --gif end to end on synthetic inputs and on the fixture videos."""
import json
import os

import numpy as np
import pytest
import torch

import gif_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _ops():
    from kpx_amd import ops
    return ops


def _dev_u8(a, off=0):
    """a uint8 on the device, contiguous, its first byte ``off`` bytes past a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.uint8)
    buf = torch.empty(a.size + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a).to(DEV))
    assert t.is_contiguous() and t.data_ptr() % 16 == off
    return t


def _pixels(g, n, seed):
    """a key-point-like mix: a long black run, a few flat colours in runs, noise"""
    rs = np.random.RandomState(seed)
    rgb = rs.randint(0, 256, size=(g, n, 3)).astype(np.uint8)
    rgb[:, :n // 2] = 0
    flat = rs.randint(0, 256, size=(5, 3)).astype(np.uint8)
    rgb[:, n // 2:3 * n // 4] = flat[rs.randint(0, 5, size=(g, 3 * n // 4 - n // 2)) if n < 256 else (np.arange(3 * n // 4 - n // 2) // 96) % 5]
    return rgb


def _hist(rgb, off=0, hist=None):
    ops = _ops()
    g = rgb.shape[0]
    if hist is None:
        hist = torch.zeros((g, 32768, 4), dtype=torch.int32, device=DEV)
    ops.color_hist_add(_dev_u8(rgb, off), hist)
    return hist


def _host(hist):
    return hist.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('g,n,off', [(1, 1, 0), (2, 35, 0), (3, 33 * 16 * 16, 0), (3, 33 * 16 * 16, 1), (2, 70001, 3)])
def test_color_hist_is_the_restatement(g, n, off):
    rgb = _pixels(g, n, seed=n)
    want = R.hist_add(np.zeros((g, 32768, 4), np.uint32), rgb)
    assert np.array_equal(_host(_hist(rgb, off)), want)


def test_color_hist_hot_cell_counts_past_16_bits():
    n = 65539
    rgb = np.empty((1, n, 3), np.uint8)
    rgb[:] = (200, 9, 77)
    got = _host(_hist(rgb))
    want = np.zeros((1, 32768, 4), np.uint32)
    want[0, (25 << 10) | (1 << 5) | 9] = (n, 200 * n, 9 * n, 77 * n)
    assert np.array_equal(got, want)
    assert np.array_equal(want, R.hist_add(np.zeros((1, 32768, 4), np.uint32), rgb))


def test_color_hist_adds_in_place_two_halves_are_the_whole():
    rgb = _pixels(2, 9000, seed=4)
    whole = _host(_hist(rgb))
    hist = _hist(rgb[:, :4321])
    halves = _host(_hist(rgb[:, 4321:], off=1, hist=hist))
    assert np.array_equal(halves, whole)


def test_color_hist_sums_are_exact_at_the_largest_size():
    """n = 2^24 - 1 pixels of (255, 255, 255): the largest sums a call can make, 255 (2^24 - 1) < 2^32"""
    ops = _ops()
    n = (1 << 24) - 1
    rgb = torch.full((1, n, 3), 255, dtype=torch.uint8, device=DEV)
    hist = torch.zeros((1, 32768, 4), dtype=torch.int32, device=DEV)
    ops.color_hist_add(rgb, hist)
    got = _host(hist)
    want = np.zeros((1, 32768, 4), np.uint32)
    want[0, 32767] = (n, 255 * n, 255 * n, 255 * n)
    assert np.array_equal(got, want)
    with pytest.raises(ops._lib.KpxError):
        ops.color_hist_add(torch.zeros((1, n + 2, 3), dtype=torch.uint8, device=DEV), hist)


def _map(rgb, pals, sizes, amp=0, off=0, out_off=None):
    """ops.palette_map on host arrays (pals: list of [P, 3]) -> host indices"""
    ops = _ops()
    g = rgb.shape[0]
    pal = np.zeros((g, 256, 3), np.uint8)
    for i, p in enumerate(pals):
        pal[i, :len(p)] = p
        pal[i, len(p):] = pals[i][0]                                   # entries past the size are never chosen, whatever they hold
    out = None
    if out_off is not None:
        out = _dev_u8(np.full(rgb.shape[:4], 255, np.uint8), out_off)
    got = ops.palette_map(_dev_u8(rgb, off), _dev_u8(pal), torch.tensor(sizes, dtype=torch.int32, device=DEV), dither=amp, out=out)
    return got.cpu().numpy()


def _palette(p, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(p, 3)).astype(np.uint8)


@pytest.mark.parametrize('p', [1, 2, 3, 17, 255, 256])
@pytest.mark.parametrize('t,h,w', [(3, 5, 7), (2, 16, 16), (1, 33, 17)])
def test_palette_map_is_the_restatement(p, t, h, w):
    rs = np.random.RandomState(p + h)
    rgb = rs.randint(0, 256, size=(1, t, h, w, 3)).astype(np.uint8)
    pal = _palette(p, p)
    rgb[0, 0, 0, :min(w, p)] = pal[:min(w, p)]                         # exact hits
    for off, out_off in ((0, None), (1, 3)):                           # a base that is not 4-byte aligned, in and out
        got = _map(rgb, [pal], [p], off=off, out_off=out_off)
        assert np.array_equal(got[0], R.palette_map(rgb[0], pal)), (off, out_off)


def test_palette_map_groups_have_their_own_palettes_and_sizes():
    rs = np.random.RandomState(1)
    rgb = rs.randint(0, 256, size=(2, 2, 16, 16, 3)).astype(np.uint8)
    pals = [_palette(5, 10), _palette(200, 11)]
    got = _map(rgb, pals, [5, 200])
    for g in range(2):
        assert np.array_equal(got[g], R.palette_map(rgb[g], pals[g]))
    assert got[0].max() < 5 and got[1].max() >= 5


def test_palette_map_at_the_rollout_width_with_dither():
    """(1, 128, 384): more than one workgroup tile, whole and partial; A = 0 is the undithered call"""
    rs = np.random.RandomState(2)
    rgb = rs.randint(0, 256, size=(1, 1, 128, 384, 3)).astype(np.uint8)
    rgb[0, 0, :, 256:] = 0
    rgb[0, 0, 40:60, 300:320] = (255, 0, 0)
    pal = _palette(256, 12)
    plain = _map(rgb, [pal], [256])
    assert np.array_equal(plain[0], R.palette_map(rgb[0], pal))
    assert np.array_equal(_map(rgb, [pal], [256], amp=0), plain)
    got = _map(rgb, [pal], [256], amp=8)
    assert np.array_equal(got[0], R.palette_map(rgb[0], pal, 8)) and not np.array_equal(got, plain)


def test_palette_map_ties_go_to_the_lowest_index():
    pal = np.array([[0, 0, 0], [2, 0, 0], [9, 9, 9], [9, 9, 9], [0, 0, 0]], np.uint8)
    rgb = np.array([[1, 0, 0], [9, 9, 9], [0, 0, 0], [2, 0, 0], [5, 5, 5]], np.uint8).reshape(1, 1, 1, 5, 3)
    got = _map(rgb, [pal], [5])
    assert got.reshape(-1).tolist() == [0, 2, 0, 1, 2]
    assert np.array_equal(got[0], R.palette_map(rgb[0], pal))
    white = np.full((1, 1, 3, 3, 3), 255, np.uint8)                    # the largest distance, 195 075
    assert not _map(white, [np.zeros((1, 3), np.uint8)], [1]).any()
    assert not _map(white, [np.zeros((3, 3), np.uint8)], [3]).any()


@pytest.mark.parametrize('amp', [0, 8, 64])
def test_palette_map_dither_clamps_at_both_ends(amp):
    rs = np.random.RandomState(amp)
    rgb = (rs.randint(0, 2, size=(1, 2, 9, 11, 3)) * 255).astype(np.uint8)          # every value 0 or 255: both clamps act
    rgb[0, 1, :4] = rs.randint(0, 256, size=(4, 11, 3))
    pal = _palette(17, 3)
    pal[0], pal[1] = (0, 0, 0), (255, 255, 255)
    got = _map(rgb, [pal], [17], amp=amp, off=1)
    assert np.array_equal(got[0], R.palette_map(rgb[0], pal, amp))
    d = R.dithered(rgb[0], amp)
    assert d.min() == 0 and d.max() == 255 and (amp == 0 or len(np.unique(d[0])) > 2)


def test_graph_replay_of_memset_histogram_and_map_is_the_eager_result():
    ops = _ops()
    rs = np.random.RandomState(6)
    a = _pixels(2, 3 * 16 * 20, seed=8).reshape(2, 3, 16, 20, 3)
    b = rs.randint(0, 256, size=a.shape).astype(np.uint8)
    rgb = _dev_u8(a)
    pal = _dev_u8(np.stack([_palette(256, 1), _palette(256, 2)]))
    sizes = torch.tensor([256, 31], dtype=torch.int32, device=DEV)
    hist = torch.zeros((2, 32768, 4), dtype=torch.int32, device=DEV)
    idx = torch.empty((2, 3, 16, 20), dtype=torch.uint8, device=DEV)

    def step():
        hist.zero_()
        ops.color_hist_add(rgb.view(2, -1, 3), hist)
        ops.palette_map(rgb, pal, sizes, dither=4, out=idx)

    step()                                                             # eager first: the one-time kernel attribute is set outside the capture
    eager = {name: (hist.cpu().numpy().copy(), idx.cpu().numpy().copy()) for name in ('a',)}
    rgb.copy_(torch.from_numpy(b).to(DEV))
    step()
    eager['b'] = (hist.cpu().numpy().copy(), idx.cpu().numpy().copy())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for name, data in (('a', a), ('b', b), ('a', a)):
        rgb.copy_(torch.from_numpy(data).to(DEV))
        hist.fill_(7)                                                  # the memset node zeroes it
        idx.fill_(255)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(hist.cpu().numpy(), eager[name][0]) and np.array_equal(idx.cpu().numpy(), eager[name][1]), name
    assert np.array_equal(eager['a'][0].view(np.uint32), R.hist_add(np.zeros((2, 32768, 4), np.uint32), a.reshape(2, -1, 3)))


def test_wrappers_refuse_what_they_cannot_launch():
    ops = _ops()
    from kpx_amd._lib import KpxError, abi_calls
    rgb = torch.zeros((1, 2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    pal = torch.zeros((1, 256, 3), dtype=torch.uint8, device=DEV)
    sizes = torch.ones((1,), dtype=torch.int32, device=DEV)
    hist = torch.zeros((1, 32768, 4), dtype=torch.int32, device=DEV)
    before = abi_calls[0]
    bad_hist = [(rgb.cpu().view(1, -1, 3), hist), (rgb.view(1, -1, 3), hist.cpu()), (rgb.view(1, -1, 3).float(), hist),
                (rgb.view(1, -1, 3), hist.float()), (rgb.view(1, -1, 3)[:, ::2], hist), (rgb.view(1, -1, 3), hist[:, ::2]),
                (rgb, hist), (rgb.view(1, -1, 3), hist[:, :100])]
    for args in bad_hist:
        with pytest.raises(KpxError):
            ops.color_hist_add(*args)
    bad_map = [dict(rgb=rgb.cpu()), dict(palette=pal.cpu()), dict(sizes=sizes.cpu()), dict(rgb=rgb.float()), dict(palette=pal.int()),
               dict(sizes=sizes.long()), dict(rgb=rgb[:, :, :, ::2]), dict(palette=pal[:, :, :2]), dict(sizes=torch.ones((2,), dtype=torch.int32, device=DEV)),
               dict(dither=65), dict(dither=-1), dict(dither=1.5), dict(pmax=0), dict(pmax=257), dict(out=torch.zeros((1, 2, 4, 4), dtype=torch.uint8)),
               dict(out=torch.zeros((1, 2, 4, 5), dtype=torch.uint8, device=DEV))]
    for kw in bad_map:
        args = dict(rgb=rgb, palette=pal, sizes=sizes)
        args.update(kw)
        with pytest.raises(KpxError):
            ops.palette_map(**args)
    with pytest.raises(KpxError):
        ops.gif_indices(rgb.cpu())
    assert abi_calls[0] == before                                      # nothing was launched
    idx, palettes, psizes = ops.gif_indices(rgb)
    assert idx.shape == (1, 2, 4, 4) and not idx.any().item() and palettes.shape == (1, 256, 3) and psizes.tolist() == [1]


def test_gif_indices_is_the_restatements_pipeline():
    ops = _ops()
    rs = np.random.RandomState(12)
    canvas = rs.randint(0, 256, size=(2, 3, 20, 24, 3)).astype(np.uint8)
    canvas[1] = (canvas[1] // 64) * 64                                 # 64 colours: a palette smaller than 256
    canvas[:, :, :, 12:] = 0
    for amp in (0, 16):
        idx, palettes, sizes = ops.gif_indices(_dev_u8(canvas, 1), amp)
        idx = idx.cpu().numpy()
        for g in range(2):
            hist = R.hist_add(np.zeros((1, 32768, 4), np.uint32), canvas[g].reshape(1, -1, 3))[0]
            pal, _ = R.median_cut(hist)
            assert sizes[g] == pal.shape[0] and np.array_equal(palettes[g, :sizes[g]], pal) and not palettes[g, sizes[g]:].any()
            assert np.array_equal(idx[g], R.palette_map(canvas[g], pal, amp))
        assert sizes[0] == 256 and sizes[1] <= 65


# ---- evaluate.py --gif end to end

def _png(path):
    from PIL import Image
    a = np.array(Image.open(path).convert('RGB'))
    return a


def _seq(folder):
    return np.stack([_png(os.path.join(folder, n)) for n in sorted(os.listdir(folder))])


def _files(root):
    """every file of a run by relative path -> its bytes (an .npz: its arrays, since a zip member carries the time it was written)"""
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            if n.endswith('.npz'):
                z = np.load(p)
                out[os.path.relpath(p, root)] = [(k, z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in sorted(z.files)]
            else:
                out[os.path.relpath(p, root)] = open(p, 'rb').read()
    return out


def _check_run(ev, plain, columns, n_samples, fps, dither, pred_folder='pred_seq', points=None):
    """the GIFs of a run against the restatement's pipeline on the PNGs of the same run; every other file against the run without --gif.
    ``points``: per sample the 8-bit key-point maps [33, H, W, 3] where the run writes no PNGs of them (--drive-only)"""
    res, t = 128, 33
    meta = json.loads(open(os.path.join(ev, 'gif.json')).read())
    delay = int(round(100.0 / fps))
    assert meta['columns'] == columns and meta['fps'] == fps and meta['delay_cs'] == delay and meta['dither'] == dither
    assert meta['frames'] == t and meta['cell'] == [res, res]
    assert len(meta['palette_sizes']['pred']) == n_samples == len(meta['palette_sizes']['compare'])
    for s in range(n_samples):
        d = os.path.join(ev, '%04d' % s)
        cells = {'pred': np.concatenate([_png(os.path.join(d, 'input_im.png'))[None], _seq(os.path.join(d, pred_folder))])}
        if 'real' in columns:
            cells['real'] = np.concatenate([cells['pred'][:1], _seq(os.path.join(d, 'real_seq'))])
        if points is None:
            cells['points'] = np.concatenate([_png(os.path.join(d, 'current_points.png'))[None], _seq(os.path.join(d, 'pred_points'))])
        else:
            cells['points'] = points[s]
        for kind, cols in (('pred', ['pred']), ('compare', columns)):
            canvas = np.concatenate([cells[c] for c in cols], axis=2)
            assert canvas.shape == (t, res, len(cols) * res, 3)
            idx, pal = R.quantise(canvas, dither)
            frames, durations, loop = R.decode_gif(os.path.join(d, kind + '.gif'))
            assert frames.shape == canvas.shape and durations == [10 * delay] * t and loop == 0
            assert meta['palette_sizes'][kind][s] == pal.shape[0]
            assert np.array_equal(frames, pal[idx]), (s, kind)
            if dither == 0 and pal.shape[0] < 256:                     # fewer cells than entries: one entry per cell
                assert np.abs(frames.astype(np.int64) - canvas).max() < 8
    with_gif, without = _files(ev), _files(plain)
    extra = sorted(set(with_gif) - set(without))
    assert extra == sorted(['gif.json'] + ['%04d/%s.gif' % (s, k) for s in range(n_samples) for k in ('pred', 'compare')])
    assert set(without) <= set(with_gif)
    for name, data in without.items():
        assert with_gif[name] == data, name


def _tiny_config(tmp_path, k, n_action, data_dir):
    import yaml
    cfg = {'paths': {'data_dir': str(data_dir), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
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


def test_evaluate_gif_on_synthetic_inputs(tmp_path, capsys):
    import evaluate
    cfg, cfg_path = _tiny_config(tmp_path, 5, 6, tmp_path / 'none')
    ckpt = _checkpoint(cfg, tmp_path)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--synthetic', '3']
    for name, extra in (('gif', ['--gif']), ('plain', [])):
        torch.manual_seed(5)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    _check_run(str(tmp_path / 'gif'), str(tmp_path / 'plain'), ['pred', 'points'], 3, 10, 0)
    with pytest.raises(SystemExit):
        evaluate.main(base + ['--gif', '--no-save', '--save_dir', str(tmp_path / 'none')])
    assert '--no-save' in capsys.readouterr().err and not os.path.exists(str(tmp_path / 'none'))


def test_evaluate_gif_drive_only_shows_the_first_driven_mode(tmp_path, monkeypatch):
    """--drive-only writes no PNGs of the key-point maps: the points column is restated from the maps the driven run returned"""
    import evaluate
    import kpx_amd
    import sheet_ref
    cfg, cfg_path = _tiny_config(tmp_path, 5, 6, tmp_path / 'none')
    ckpt = _checkpoint(cfg, tmp_path)
    maps = {'gif': [], 'plain': []}
    run = kpx_amd.FinalModel.run

    def recording_run(self, sess, feed_dict, z=None, drive=None):
        out = run(self, sess, feed_dict, z=z, drive=drive)
        first, seq = out['current_points'].cpu().numpy(), out['future_points'].cpu().numpy()
        maps[name].extend(sheet_ref.raw8(np.concatenate([first[:, None], seq], axis=1)))
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--batch', '2', '--synthetic', '3', '--drive', 'hold', '--drive-only']
    for name, extra in (('gif', ['--gif', '--gif-fps', '25', '--gif-dither', '8']), ('plain', [])):
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    assert len(maps['gif']) == 3 and maps['gif'][0].shape == (33, 128, 128, 3)
    _check_run(str(tmp_path / 'gif'), str(tmp_path / 'plain'), ['pred', 'points'], 3, 25, 8, pred_folder='drive_hold', points=maps['gif'])


def test_evaluate_gif_on_the_fixture_videos(tmp_path):
    import evaluate
    import make_pseudo_labels
    from test_data_gpu import _fixture_dataset
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    cfg, cfg_path = _tiny_config(tmp_path, int(golden['n_points']), int(golden['n_action']), data)
    ckpt = _checkpoint(cfg, tmp_path)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt])
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics', '--samples', '2']
    for name, extra in (('gif', ['--gif', '--gif-fps', '12']), ('plain', [])):
        torch.manual_seed(5)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    _check_run(str(tmp_path / 'gif'), str(tmp_path / 'plain'), ['real', 'pred', 'points'], 3, 12, 0)
