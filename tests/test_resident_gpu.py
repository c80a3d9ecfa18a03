"""GPU: HBM-resident frames + the augmentation kernels (kpx_augment_geometry_u8 / kpx_augment_filter_f32, kpx_amd.resident) against
ImagePairDataLoader.render, i.e. the PIL installed here.  Every comparison is exact: torch.equal / np.array_equal, no tolerance."""
import os
import random

import numpy as np
import pytest
import torch

import resident_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(480, 270), (270, 480), (320, 240), (486, 360), (128, 128), (641, 359), (129, 128)]


@pytest.fixture(scope='module')
def dev():
    import kpx_amd  # noqa: F401
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def synthetic(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('resident_synthetic'))
    return root, ref.write_dataset(root, SIZES, frames=12, subsets=('train', 'test'))


def _fixture_dataset(root):
    golden = np.load(os.path.join(HERE, 'golden', 'image_pair_ref.npz'))
    for k, rel in enumerate(str(n) for n in golden['file_names']):
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(golden['file_%03d' % k].tobytes())
    for subset in ('train', 'test'):
        (root / (subset + '_set.txt')).write_bytes(golden['listing'].tobytes())
    return str(root)


def _loader(root, random_order=True, randomness=True, seed=5):
    from kpx_amd.data import ImagePairDataLoader
    return ImagePairDataLoader(root, 'train', random_order=random_order, randomness=randomness, rng=random.Random(seed),
                               np_rng=np.random.RandomState(seed))


def _want(loader, plans):
    """render (PIL) on the plans -> float32 [2 * len(plans), 128, 128, 3], images first, like the rows of rows_for_plans."""
    from kpx_amd.data import _u8_to_unit_numpy
    pairs = [loader.render(p) for p in plans]
    return torch.from_numpy(_u8_to_unit_numpy(np.stack([p[0] for p in pairs] + [p[1] for p in pairs])))


def _stage_plans(loader, video, w, h):
    """Hand-made decisions covering every stage: each angle, the crop origins 0 / max / between, both flips, every filter id, the
    enhancers at both ends of their ranges and at 9, 10 (factor 1.0) and 11."""
    from kpx_amd.data import PairPlan, _ENHANCERS, _resized_size
    rw, rh, _ = _resized_size(w, h)
    cmax = int((rw if w > h else rh) - 128)
    crops = [0, cmax, cmax // 2]
    filters = [(f, None) for f in range(6)] + [(f, v) for f, (_, lo, hi) in sorted(_ENHANCERS.items()) for v in (lo, hi, 9, 10, 11)]
    plans, k = [], 0

    def add(angle, crop, flip, fv):
        plans.append(PairPlan(video, len(plans) % 12, (len(plans) + 9) % 12, angle, crop, flip, fv[0], fv[1]))
    for angle in range(-10, 11):
        add(angle, crops[k % 3], k % 2, filters[k % len(filters)]); k += 1
    for fv in filters:
        add((k * 7) % 21 - 10, crops[k % 3], (k // 3) % 2, fv); k += 1
    for crop in crops:
        for flip in (0, 1):
            add(0, crop, flip, filters[k % 6]); k += 1
    return plans


def test_every_stage_equals_render(dev, synthetic):
    from kpx_amd.resident import ResidentFrames
    root, names = synthetic
    loader = _loader(root)
    store = ResidentFrames(root, ['%s 0' % n for n in names], dev)
    assert store.frames.dtype == torch.uint8 and store.frames.numel() == store.index.total_bytes and store.frames.is_cuda
    assert store.frame_off.dtype == torch.int64 and np.array_equal(store.frame_off.cpu().numpy(), store.index.offsets)
    assert store.video_table.cpu().tolist() == [[w, h, 12 * v, 12] for v, (w, h) in enumerate(SIZES)]
    for name, (w, h) in zip(names, SIZES):
        plans = _stage_plans(loader, name, w, h)
        rows = store.rows_for_plans(plans, True)
        got = store.augment_rows(rows)
        want = _want(loader, plans)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2 * len(plans), 128, 128, 3)
        bad = [k for k in range(len(rows)) if not torch.equal(got[k].cpu(), want[k])]
        assert not bad, ((w, h), [plans[k % len(plans)] for k in bad[:4]])
    # the store holds the decoded frames themselves
    from PIL import Image
    k = store.index.frame_number(names[3], 7)
    o = int(store.index.offsets[k])
    frame = np.asarray(Image.open(os.path.join(root, names[3], '000008.jpg')))
    assert np.array_equal(store.frames[o:o + frame.size].cpu().numpy().reshape(frame.shape), frame)


def test_centre_crop_rows_equal_render(dev, synthetic):
    """randomness off: no rotation, the centre box of render's else branch, no filter -- on every frame size."""
    root, names = synthetic
    loader = _loader(root, random_order=False, randomness=False)
    store = loader.resident_frames(dev)
    plans = list(loader.plans())
    got = store.augment_rows(store.rows_for_plans(plans, False))
    assert torch.equal(got.cpu(), _want(loader, plans))


def _compare_batches(root, dev, batch, n_batches, **kw):
    a, b = _loader(root, **kw), _loader(root, **kw)
    it_d, it_h = iter(a.batches(batch, dev, resident=True)), iter(b.batches(batch, 'cpu'))
    for _ in range(n_batches):
        bd, bh = next(it_d), next(it_h)
        for key in ('image', 'future_image'):
            assert bd[key].device.type == 'cuda' and bd[key].dtype == torch.float32 and tuple(bd[key].shape) == (batch, 128, 128, 3)
            assert torch.equal(bd[key].cpu(), bh[key])


def test_resident_batches_equal_host_batches_on_the_fixture(dev, tmp_path):
    _compare_batches(_fixture_dataset(tmp_path), dev, 8, 25)                 # 200 pairs, random order, all augmentations


def test_resident_batches_equal_host_batches_on_synthetic_frames(dev, synthetic):
    _compare_batches(synthetic[0], dev, 8, 25)


def test_shuffled_sequential_batches_equal_host_batches(dev, synthetic):
    """random_order off + shuffle: the plan-level shuffle buffer draws from rng in both iterators alike."""
    a, b = (_loader(synthetic[0], random_order=False, randomness=True, seed=3) for _ in range(2))
    it_d, it_h = iter(a.batches(4, dev, shuffle=True, resident=True)), iter(b.batches(4, 'cpu', shuffle=True))
    for _ in range(6):
        bd, bh = next(it_d), next(it_h)
        assert torch.equal(bd['image'].cpu(), bh['image']) and torch.equal(bd['future_image'].cpu(), bh['future_image'])


@pytest.mark.parametrize('which', ['fixture', 'synthetic'])
def test_one_sequential_pass_ends_with_a_short_batch(dev, synthetic, tmp_path, which):
    root = _fixture_dataset(tmp_path) if which == 'fixture' else synthetic[0]
    batch = 2 if which == 'fixture' else 4                                   # 3 and 7 listed videos: the last batch is short
    a, b = (_loader(root, random_order=False, randomness=False) for _ in range(2))
    got = list(a.batches(batch, dev, repeat=False, resident=True))
    want = list(b.batches(batch, 'cpu', repeat=False))
    assert [tuple(g['image'].shape) for g in got] == [tuple(w['image'].shape) for w in want]
    assert got[-1]['image'].shape[0] == a.length() % batch
    for g, w in zip(got, want):
        assert torch.equal(g['image'].cpu(), w['image']) and torch.equal(g['future_image'].cpu(), w['future_image'])


def test_a_second_iterator_reuses_the_store(dev, synthetic):
    root = synthetic[0]
    a = _loader(root, seed=3)
    first = iter(a.batches(4, dev, resident=True))
    for _ in range(3):
        next(first)
    store = a.resident_frames(dev)
    a._rng, a._np_rng = random.Random(9), np.random.RandomState(9)
    second = iter(a.batches(4, dev, resident=True))
    assert a.resident_frames(dev) is store and second.store is store         # built once
    fresh_loader = _loader(root, seed=9)
    fresh = iter(fresh_loader.batches(4, dev, resident=True))
    assert fresh.store is not store                                          # built anew
    for _ in range(5):
        x, y = next(second), next(fresh)
        assert torch.equal(x['image'], y['image']) and torch.equal(x['future_image'], y['future_image'])


def test_graph_replay_equals_direct_launches(dev, synthetic):
    """The two launches captured in a HIP graph whose input is the device table: new rows in the same buffer, replayed, give the bytes
    of direct launches on those rows."""
    root, names = synthetic
    loader = _loader(root, seed=21)
    store = loader.resident_frames(dev)
    n = 8
    plans = _endless(loader)
    batches = [store.check_rows(store.rows_for_plans([next(plans) for _ in range(n)], True)) for _ in range(3)]
    direct = [store.augment_rows(rows).clone() for rows in batches]
    rows_dev = torch.from_numpy(batches[0]).to(dev)
    out = torch.empty((2 * n, 128, 128, 3), dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        store.augment(rows_dev, 2 * n, out=out)                              # warm-up outside the capture
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


def _endless(loader):
    while True:
        for p in loader.plans():
            yield p


def test_invalid_rows_never_reach_the_device(dev, synthetic):
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError
    loader = _loader(synthetic[0])
    store = loader.resident_frames(dev)
    rows = store.rows_for_plans(list(loader.plans())[:2], True)
    for col, value in ((R.R_FRAME, len(store.index.offsets)), (R.R_X0, 4000), (R.R_FILT, 10)):
        bad = rows.copy()
        bad[1, col] = value
        with pytest.raises(KpxError):
            store.augment_rows(bad)
    with pytest.raises(KpxError, match='max_bytes'):
        _loader(synthetic[0]).batches(4, dev, resident=True, max_resident_bytes=1 << 20)


def test_train_py_with_resident_data_trains_the_same_parameters(dev, tmp_path):
    """train.py --resident-data --steps 2 on the fixture dataset: checkpoints written, and every variable equals, bit for bit, the one
    of the run without the flag (equal inputs under the same seeds, deterministic step)."""
    import yaml
    import train
    data = _fixture_dataset(tmp_path / 'penn')
    ckpts = {}
    for tag, extra in (('cpu', []), ('resident', ['--resident-data'])):
        cfg = {'paths': {'data_dir': data, 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / tag)},
               'training': {'n_steps': 2, 'summary_interval': 500, 'test_interval': 1, 'checkpoint_interval': 1, 'log_interval': 1,
                            'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
               'model': {'n_pts': 5, 'n_action': 9, 'cell_info': [32, 32], 'vae_dim': 8}}
        cfg_path = tmp_path / (tag + '.yaml')
        cfg_path.write_text(yaml.safe_dump(cfg))
        train.main(['--mode', 'detector_translator', '--config', str(cfg_path), '--synthetic-vgg', '--steps', '2'] + extra)
        path = tmp_path / tag / 'detector_translator' / 'model.ckpt-1.npz'
        assert path.exists()
        ckpts[tag] = np.load(str(path))
    assert sorted(ckpts['cpu'].files) == sorted(ckpts['resident'].files) and len(ckpts['cpu'].files) > 10
    for name in ckpts['cpu'].files:
        assert np.array_equal(ckpts['cpu'][name], ckpts['resident'][name]), name
