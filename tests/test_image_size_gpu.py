"""GPU: the resident augmentation at an image size S of its own (kpx_augment_geometry_sq_u8 / kpx_augment_filter_sq_f32, kpx_amd.resident)
against ImagePairDataLoader.render at that S, i.e. the PIL installed here; the new entries against the old ones at 128; and the four
command lines with --image-size.  Every comparison of pixels is exact: torch.equal / np.array_equal, no tolerance."""
import json
import os
import random

import numpy as np
import pytest
import torch

import image_size_ref as isr
import resident_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = [(80, 60), (60, 80), (40, 56)]           # landscape, portrait, and one that upscales even at 48
FRAMES = 12


@pytest.fixture(scope='module')
def dev():
    import kpx_amd  # noqa: F401
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def small(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('image_size_small'))
    return root, ref.write_dataset(root, SMALL, frames=FRAMES, subsets=('train', 'test'))


def _loader(root, random_order=True, randomness=True, seed=5, **kw):
    from kpx_amd.data import ImagePairDataLoader
    return ImagePairDataLoader(root, 'train', random_order=random_order, randomness=randomness, rng=random.Random(seed),
                               np_rng=np.random.RandomState(seed), **kw)


def _fixture_dataset(root):
    golden = np.load(os.path.join(HERE, 'golden', 'image_pair_ref.npz'))
    for k, rel in enumerate(str(n) for n in golden['file_names']):
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(golden['file_%03d' % k].tobytes())
    for subset in ('train', 'test'):
        (root / (subset + '_set.txt')).write_bytes(golden['listing'].tobytes())
    return golden


def _cases(store, root, names, sizes, side, frames):
    """The enumerated rows of every video, then its centre-crop rows -> (checked int32 rows, the tiles before the filter and the tiles
    after it as Pillow makes them, uint8 [n, S, S, 3] each, in row order)"""
    from kpx_amd import resident as R
    rows, plain, final = [], [], []
    for randomness in (True, False):
        loader = _loader(root, random_order=False, randomness=randomness, image_size=side)
        if randomness:
            plans = [p for name, (w, h) in zip(names, sizes) for p in isr.enumerated_plans(name, w, h, side, frames)]
        else:
            plans = [p._replace(fu_idx=p.fu_idx % frames) for p in loader.plans()]       # frames 0 and 10 of the video, or of a shorter one 0 and 10 % n
        rows.append(store.rows_for_plans(plans, randomness))
        pairs = [loader.render(p) for p in plans]
        for which in (0, 1):                                          # rows_for_plans: every plan's image, then every plan's future_image
            for p, pair in zip(plans, pairs):
                path = R.frame_path(root, p.video, (p.im_idx, p.fu_idx)[which])
                plain.append(np.asarray(isr.pillow_tile(path, p, side, randomness)))
                final.append(pair[which])
    rows = store.check_rows(np.concatenate(rows))
    isr.assert_full_coverage(rows)
    return rows, np.stack(plain), np.stack(final)


def _launch(store, rows):
    """The two launches through the wrappers of ops.py -> (tiles, lsum, out) on the device"""
    from kpx_amd import ops
    rows_dev = torch.from_numpy(rows).to(store.device)
    n, s = rows.shape[0], store.image_size
    tiles, lsum = ops.augment_geometry(store.frames, store.frame_off, rows_dev, n, store.resize_tabs, store.band_rows_cap, s)
    out = ops.augment_filter(tiles, lsum, rows_dev, n, store.kernels, s)
    torch.cuda.synchronize()
    return tiles, lsum, out


def _assert_equal_render(store, rows, plain, final):
    from kpx_amd.data import _u8_to_unit_numpy
    s = store.image_size
    tiles, lsum, out = _launch(store, rows)
    assert tiles.dtype == torch.uint8 and tuple(tiles.shape) == (len(rows), s, s, 3)
    assert lsum.dtype == torch.int32 and tuple(lsum.shape) == (len(rows), s // 16)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(rows), s, s, 3)
    got_tiles, got_lsum, got_out = tiles.cpu().numpy(), lsum.cpu().numpy(), out.cpu().numpy()
    want_out = _u8_to_unit_numpy(final)
    bad = [k for k in range(len(rows)) if not np.array_equal(got_tiles[k], plain[k])]
    assert not bad, ('tiles', s, bad[:8], rows[bad[0]].tolist())
    bad = [k for k in range(len(rows)) if not np.array_equal(got_lsum[k], isr.band_luminance(plain[k]))]
    assert not bad, ('lsum', s, bad[:8])
    bad = [k for k in range(len(rows)) if not np.array_equal(got_out[k], want_out[k])]
    assert not bad, ('out', s, bad[:8], rows[bad[0]].tolist())
    assert torch.equal(store.augment_rows(rows), out)                 # the store's own call is these two launches


# ---------------------------------------------------------------------------------------------- every stage at S = 32 and 48
@pytest.mark.parametrize('side', [32, 48])
def test_every_stage_equals_render_at_small_sides(dev, small, side):
    """2 and 3 bands; 48 is no power of two, so a surviving shift or mask, or a contrast mean divided by 2^14, shows here."""
    from kpx_amd.resident import ResidentFrames
    root, names = small
    store = ResidentFrames(root, ['%s 0' % n for n in names], dev, image_size=side)
    assert store.image_size == side and store.bands == side // 16
    rows, plain, final = _cases(store, root, names, SMALL, side, FRAMES)
    _assert_equal_render(store, rows, plain, final)


# ---------------------------------------------------------------------------------------------- S = 256, and the LDS opt-in
def test_side_256_with_a_band_above_64_kb_of_lds(dev, tmp_path):
    from kpx_amd import resident as R
    sizes = [(320, 270), (1700, 1300)]
    root = str(tmp_path / 'big')
    os.makedirs(root)
    names = ref.write_dataset(root, sizes, frames=2)
    xmin, cnt, _ = R.resize_table(1300, 256)
    need = R.band_rows(xmin, cnt)
    assert need > 85 and need * 256 * 3 > 64 * 1024 and need * 256 * 3 <= R.LDS_BYTES      # the launch has to opt in
    store = R.ResidentFrames(root, ['%s 0' % n for n in names], dev, image_size=256)
    assert store.band_rows_cap == need
    rows, plain, final = _cases(store, root, names, sizes, 256, 2)
    _assert_equal_render(store, rows, plain, final)


# ---------------------------------------------------------------------------------------------- S = 128: the old entries
def test_new_and_old_entries_agree_bit_for_bit_at_128(dev, small):
    from kpx_amd import resident as R
    from kpx_amd._lib import lib
    root, names = small
    store = R.ResidentFrames(root, ['%s 0' % n for n in names], dev)
    assert store.image_size == 128
    rows, plain, final = _cases(store, root, names, SMALL, 128, FRAMES)
    tiles, lsum, out = _launch(store, rows)
    n = len(rows)
    rows_dev = torch.from_numpy(rows).to(dev)
    tiles0 = torch.full((n, 128, 128, 3), 0x5A, dtype=torch.uint8, device=dev)
    lsum0 = torch.full((n, R.BANDS), -7, dtype=torch.int32, device=dev)
    out0 = torch.full((n, 128, 128, 3), 7.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert lib.kpx_augment_geometry_u8(store.frames.data_ptr(), store.frame_off.data_ptr(), rows_dev.data_ptr(), n, store.resize_tabs.data_ptr(),
                                       store.band_rows_cap, tiles0.data_ptr(), lsum0.data_ptr(), stream) == 0
    assert lib.kpx_augment_filter_f32(tiles0.data_ptr(), lsum0.data_ptr(), rows_dev.data_ptr(), n, store.kernels.data_ptr(), out0.data_ptr(),
                                      stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(tiles, tiles0) and torch.equal(lsum, lsum0) and torch.equal(out, out0)
    assert np.array_equal(tiles0.cpu().numpy(), plain)               # and both are render's


# ---------------------------------------------------------------------------------------------- batches at S = 48
def test_resident_batches_equal_host_batches_at_48(dev, small):
    root = small[0]
    a, b = _loader(root, image_size=48), _loader(root, image_size=48)
    it_d, it_h = iter(a.batches(4, dev, resident=True)), iter(b.batches(4, 'cpu'))
    for _ in range(6):                                                # random order, all augmentations
        bd, bh = next(it_d), next(it_h)
        for key in ('image', 'future_image'):
            assert bd[key].device.type == 'cuda' and bd[key].dtype == torch.float32 and tuple(bd[key].shape) == (4, 48, 48, 3)
            assert torch.equal(bd[key].cpu(), bh[key])
    a, b = (_loader(root, random_order=False, randomness=False, image_size=48) for _ in range(2))
    got = list(a.batches(2, dev, repeat=False, resident=True))        # three listed videos: the last batch is short
    want = list(b.batches(2, 'cpu', repeat=False))
    assert [tuple(g['image'].shape) for g in got] == [tuple(w['image'].shape) for w in want] == [(2, 48, 48, 3), (1, 48, 48, 3)]
    for g, w in zip(got, want):
        assert torch.equal(g['image'].cpu(), w['image']) and torch.equal(g['future_image'].cpu(), w['future_image'])


def test_graph_replay_equals_direct_launches_at_48(dev, small):
    root = small[0]
    loader = _loader(root, seed=21, image_size=48)
    store = loader.resident_frames(dev)
    n = 4
    plans = [p for _ in range(4) for p in loader.plans()]            # three per pass: twelve
    batches = [store.check_rows(store.rows_for_plans(plans[i * n:(i + 1) * n], True)) for i in range(3)]
    direct = [store.augment_rows(rows).clone() for rows in batches]
    rows_dev = torch.from_numpy(batches[0]).to(dev)
    out = torch.empty((2 * n, 48, 48, 3), dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        store.augment(rows_dev, 2 * n, out=out)                      # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        store.augment(rows_dev, 2 * n, out=out)
    for rows, want in zip(batches[1:] + batches[:1], direct[1:] + direct[:1]):
        rows_dev.copy_(torch.from_numpy(rows))
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------- refusals: nothing is launched
def test_refused_calls_leave_the_outputs_untouched(dev, small):
    from kpx_amd import ops, resident as R
    from kpx_amd._lib import KpxError, lib
    root, names = small
    store = R.ResidentFrames(root, ['%s 0' % n for n in names], dev, image_size=48)
    rows = store.check_rows(store.rows_for_plans(list(_loader(root, image_size=48).plans())[:2], True))
    rows_dev, n = torch.from_numpy(rows).to(dev), len(rows)
    tiles = torch.full((n, 48, 48, 3), 0x5A, dtype=torch.uint8, device=dev)
    lsum = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
    out = torch.full((n, 48, 48, 3), 7.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def geometry(side=48, cap=store.band_rows_cap, frames=store.frames.data_ptr()):
        return lib.kpx_augment_geometry_sq_u8(frames, store.frame_off.data_ptr(), rows_dev.data_ptr(), n, store.resize_tabs.data_ptr(), cap, side,
                                              tiles.data_ptr(), lsum.data_ptr(), stream)

    def filt(side=48, kernels=store.kernels.data_ptr()):
        return lib.kpx_augment_filter_sq_f32(tiles.data_ptr(), lsum.data_ptr(), rows_dev.data_ptr(), n, kernels, side, out.data_ptr(), stream)
    assert geometry(side=40) == -1 and geometry(side=272) == -1 and geometry(frames=None) == -1
    assert geometry(cap=R.LDS_BYTES // (48 * 3) + 1) == -1            # one row more than the LDS of a workgroup holds
    assert filt(side=40) == -1 and filt(side=272) == -1 and filt(kernels=None) == -1
    for bad in (lambda: ops.augment_geometry(store.frames, store.frame_off, rows_dev, n, store.resize_tabs, store.band_rows_cap, 40, tiles, lsum),
                lambda: ops.augment_geometry(store.frames, store.frame_off, rows_dev, n, store.resize_tabs, R.LDS_BYTES // (48 * 3) + 1, 48, tiles, lsum),
                lambda: ops.augment_geometry(store.frames, store.frame_off, rows_dev.long(), n, store.resize_tabs, store.band_rows_cap, 48, tiles, lsum),
                lambda: ops.augment_geometry(store.frames, store.frame_off, rows_dev, n + 1, store.resize_tabs, store.band_rows_cap, 48),
                lambda: ops.augment_filter(tiles, lsum, rows_dev, n, store.kernels, 272, out),
                lambda: ops.augment_filter(tiles, lsum[:, :2].contiguous(), rows_dev, n, store.kernels, 48, out),
                lambda: ops.augment_filter(tiles.cpu(), lsum.cpu(), rows_dev.cpu(), n, store.kernels.cpu(), 48)):
        with pytest.raises(KpxError):
            bad()
    torch.cuda.synchronize()
    assert bool((tiles == 0x5A).all()) and bool((lsum == -7).all()) and bool((out == 7.0).all())
    assert geometry() == 0 and filt() == 0                            # the same buffers, the right arguments
    torch.cuda.synchronize()
    assert torch.equal(out, store.augment_rows(rows))


# ---------------------------------------------------------------------------------------------- the model at a side that is no power of two
def test_train_step_at_48_matches_the_oracle(dev):
    """The checker admits every multiple of 16: one tiny detector_translator step at 48 against the CPU oracle, with smoke()'s bounds."""
    import kpx_amd
    from oracle import restatement as O
    res, k, b = 48, 3, 2
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': b},
           'model': {'n_pts': k}, 'paths': {'log_dir': '/tmp/kpx_image_size', 'vggnet': None}}
    vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(seed=19, width_div=8), device=dev)
    model = kpx_amd.DetectorTranslatorModel(cfg, device=dev, vgg=vgg, image_size=res)
    model.build()
    im, fut = O.synthetic_pair(b, res=res)
    model.train_step(None, {'image': torch.from_numpy(im).to(dev), 'future_image': torch.from_numpy(fut).to(dev)}, 0, b)
    got = model.loss_values()
    want = O.train_step(O.TrainState(O.init_variables(k, res=res, seed=1234), O.synthetic_vgg(seed=19, width_div=8)), im, fut)
    for key in ('loss_D', 'loss_G'):
        assert abs(got[key] - want[key]) <= 1e-4 * max(1.0, abs(want[key])), (key, got[key], want[key])
    frame = model.last['fwd']['final_output'].cpu().numpy()
    rel = np.linalg.norm(frame - want['final_output'].numpy()) / np.linalg.norm(want['final_output'].numpy())
    assert rel < 1e-4, rel


# ---------------------------------------------------------------------------------------------- the command lines
def _tiny_config(data, log_dir, k=5, n_action=9, **model):
    return {'paths': {'data_dir': str(data), 'vggnet': str(log_dir) + '.none.npy', 'log_dir': str(log_dir)},
            'training': {'n_steps': 3, 'summary_interval': 500, 'test_interval': 1, 'checkpoint_interval': 1, 'log_interval': 1,
                         'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
            'model': dict({'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8}, **model)}


def test_train_py_at_32_trains_the_same_parameters_from_resident_frames(dev, tmp_path):
    """train.py --image-size 32 --resident-data --steps 3 on the fixture tree ends with the parameters, bit for bit, of the same run on the
    host loader (test_resident_gpu.py's claim at 128)."""
    import yaml
    import train
    data = tmp_path / 'penn'
    _fixture_dataset(data)
    ckpts = {}
    for tag, extra in (('cpu', []), ('resident', ['--resident-data'])):
        cfg_path = tmp_path / (tag + '.yaml')
        cfg_path.write_text(yaml.safe_dump(_tiny_config(data, tmp_path / tag)))
        train.main(['--mode', 'detector_translator', '--config', str(cfg_path), '--image-size', '32', '--synthetic-vgg', '--steps', '3'] + extra)
        path = tmp_path / tag / 'detector_translator' / 'model.ckpt-2.npz'
        assert path.exists()
        ckpts[tag] = np.load(str(path))
    assert sorted(ckpts['cpu'].files) == sorted(ckpts['resident'].files) and len(ckpts['cpu'].files) > 10
    for name in ckpts['cpu'].files:
        assert np.array_equal(ckpts['cpu'][name], ckpts['resident'][name]), name


def _png_sizes(root):
    from PIL import Image
    out = {}
    for d, _, names in os.walk(str(root)):
        for n in names:
            if n.endswith('.png'):
                with Image.open(os.path.join(d, n)) as im:
                    out[os.path.relpath(os.path.join(d, n), str(root))] = im.size
    return out


def test_labels_and_evaluation_at_64(dev, tmp_path):
    """make_pseudo_labels.py then evaluate.py with --image-size 64 on the JPEG fixture, from a checkpoint written at 128."""
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k = int(golden['n_points'])
    cfg = _tiny_config(data, tmp_path / 'results', k=k, n_action=int(golden['n_action']), image_size=32)      # the command line beats the YAML
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=dev)                          # a checkpoint carries no size: written at 128, read at 64
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt, '--image-size', '64'])
    for vid, n in zip(golden['kp_idx'], golden['kp_len']):
        pts = np.load(str(data / 'pseudo_labels' / ('%04d.npy' % int(vid))))
        assert pts.shape == (int(n), k, 2) and np.isfinite(pts).all() and np.abs(pts).max() <= 1.0
    ev = tmp_path / 'eval'
    evaluate.main(['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--save_dir', str(ev), '--batch', '2',
                   '--image-size', '64', '--metrics', '--samples', '1', '--actions', '0,1'])
    assert json.loads((ev / 'metrics.json').read_text())['n_samples'] == 3
    sizes = _png_sizes(ev)
    sheets = {'classes.png': (9 * 64, 3 * 64), 'classes_points.png': (9 * 64, 2 * 64)}       # 1 + 8 columns; the real row + two classes
    assert len(sizes) > 3 * 5 * 32
    for rel, size in sizes.items():
        assert size == sheets.get(os.path.basename(rel), (64, 64)), (rel, size)
    assert sum(os.path.basename(rel) in sheets for rel in sizes) == 6


def test_animate_py_at_64_writes_64_pixel_cells(dev, tmp_path):
    import yaml
    from PIL import Image
    import animate
    import kpx_amd
    cfg = _tiny_config(tmp_path / 'none', tmp_path / 'results', k=5, n_action=3)
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=dev)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    still = tmp_path / 'still.jpg'
    ref.jpeg_frame(200, 150, 6).save(str(still), format='JPEG', quality=90)
    out = tmp_path / 'out'
    animate.main(['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--images', str(still), '--actions', '0,2',
                  '--samples', '2', '--image-size', '64', '--png', '--save_dir', str(out)])
    meta = json.loads((out / 'animate.json').read_text())
    assert meta['cell'] == [64, 64] and meta['stills'][0]['resized_size'] == [85, 64]
    with Image.open(str(out / '0000' / 'classes.gif')) as gif:
        assert gif.size == (2 * 64, 2 * 64) and gif.n_frames == 33                # two classes wide, two draws high
    with Image.open(str(out / '0000' / 'input_im.png')) as im:
        assert im.size == (64, 64)
    frames = {rel: s for rel, s in _png_sizes(out).items() if os.sep + 'pred_seq' + os.sep in rel}
    assert len(frames) == 2 * 2 * 32 and set(frames.values()) == {(64, 64)}
