"""GPU: stage 2's resident key-point labels (csrc/augment_seq.hip, kpx_amd.resident) against ``SequenceDataLoader.render`` -- the kernel,
the iterator and train.py --resident-labels.  Every comparison is on bit patterns, so -0.0 and +0.0 are told apart."""
import os

import numpy as np
import pytest
import torch

import resident_seq_ref as ref

pytestmark = pytest.mark.gpu
KEYS = ('keypoints', 'real_seq', 'action_code')


@pytest.fixture(scope='module')
def dev():
    import kpx_amd  # noqa: F401
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp('seq')
    ref.write_dataset(root)
    return root


def _same(got, want, what=''):
    for key in KEYS:
        g = got[key]
        assert g.dtype == torch.float32 and g.device.type == 'cuda' and tuple(g.shape) == tuple(want[key].shape), (what, key)
        assert np.array_equal(ref.bits(g), ref.bits(want[key])), (what, key)


def test_kernel_equals_render_on_hand_made_plans(dev, dataset):
    """Every angle, both flips, scales 0.70 / 1.00 / 1.20, the first and last legal start of every video, both forms, with and without
    ``randomness``: a few hundred rows in ONE launch at K = 5."""
    rows, want = [], []
    for randomness in (True, False):
        ld = ref.loader(dataset, False, randomness)
        store = ld.resident_labels(dev)
        plans = ref.hand_plans(randomness)
        rows.append(store.rows_for_plans(plans))
        want.append(ref.collated(ld, plans))
    rows = np.concatenate(rows)
    assert 300 <= rows.shape[0] <= 1000
    want = {key: np.concatenate([w[key] for w in want]) for key in KEYS}
    z = ref.bits(want['real_seq'])[want['real_seq'] == 0]
    assert (z == 0).any() and (z != 0).any()                      # zeros of both signs are among the expected values
    _same(store.augment_rows(rows), want)


def test_kernel_equals_render_at_forty_points(dev, tmp_path):
    """One launch at the reference's K = 40 with the plans a seeded loader draws (more than one workgroup per sample)."""
    ref.write_dataset(tmp_path, frames=(70, 40, 20), k=40, w=64, h=48, seed=1)
    ld = ref.loader(tmp_path, True, True, seed=9, k=40)
    plans = [p for _ in range(12) for p in ld.plans()]
    assert len(plans) == 48 and {int(p.n_files / 33) for p in plans} == {0, 1, 2}
    store = ld.resident_labels(dev)
    _same(store.augment_rows(store.rows_for_plans(plans)), ref.collated(ld, plans))


@pytest.mark.parametrize('random_order,randomness,repeat', [(True, True, True), (False, False, False)])
def test_resident_iterator_equals_host_iterator(dev, dataset, random_order, randomness, repeat):
    """Equal seeds, equal batches: the listing has 7 lines, so a pass is a batch of 4 and a short batch of 3."""
    ld = ref.loader(dataset, random_order, randomness, seed=5)
    it_r = ld.batches(4, dev, repeat=repeat, resident=True)
    it_h = ref.loader(dataset, random_order, randomness, seed=5).batches(4, dev, repeat=repeat)
    sizes = []
    for _ in range(6 if repeat else 2):          # with repeat: more batches than pinned slots, the ring is reused
        br, bh = next(it_r), next(it_h)
        assert sorted(br) == sorted(KEYS) and 'image' in bh
        _same(br, {key: bh[key].cpu().numpy() for key in KEYS})
        im = it_r.start_images(2)
        assert im.dtype == torch.float32 and im.device.type == 'cuda' and tuple(im.shape) == (2, 128, 128, 3)
        assert torch.equal(im, bh['image'][:2])
        sizes.append(br['keypoints'].shape[0])
    assert sizes == ([4, 3] * 3 if repeat else [4, 3])
    if not repeat:
        with pytest.raises(StopIteration):
            next(it_r)
        with pytest.raises(StopIteration):
            next(it_h)
    # a second iterator on the same loader reuses the store
    store = it_r.store
    assert ld.batches(2, dev, resident=True).store is store and ld.resident_labels(dev) is store


def test_resident_iterator_refuses_future_frames(dev, dataset):
    from kpx_amd._lib import KpxError
    from kpx_amd.data import SequenceDataLoader
    ld = SequenceDataLoader(str(dataset), 'train', ref.K, ref.N_ACTION, with_image_seq=True, random_order=False, randomness=False)
    with pytest.raises(KpxError):
        ld.batches(2, dev, resident=True)


def test_invalid_rows_raise_before_any_launch(dev, dataset):
    from kpx_amd import _lib, resident as R
    store = ref.loader(dataset, False, True).resident_labels(dev)
    good = store.rows_for_plans(ref.hand_plans(True)[:8])
    store.augment_rows(good)
    calls = _lib.abi_calls[0]
    for col, value in ((R.S_VIDEO, len(ref.FRAMES)), (R.S_IM_IDX, 1 << 20), (R.S_GAP, 1 << 10), (R.S_ANGLE, R.SEQ_ANGLES), (R.S_ACTION, ref.N_ACTION)):
        rows = good.copy()
        rows[3, col] = value
        with pytest.raises(_lib.KpxError):
            store.augment_rows(rows)
    with pytest.raises(_lib.KpxError):
        store.augment_rows(np.repeat(good, R.SEQ_MAX_ROWS // 8 + 1, axis=0))
    assert _lib.abi_calls[0] == calls            # nothing was launched


def _train(tmp_path, data, name, flag):
    import yaml
    import train
    cfg = {'paths': {'data_dir': str(data), 'vggnet': None, 'log_dir': str(tmp_path / name)},
           'training': {'n_steps': 2, 'summary_interval': 1, 'test_interval': 1, 'checkpoint_interval': 1, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': ref.K, 'n_action': ref.N_ACTION, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / (name + '.yaml')
    cfg_path.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(0)
    train.main(['--mode', 'motion_generator', '--config', str(cfg_path), '--steps', '2'] + (['--resident-labels'] if flag else []))
    from kpx_amd import summary
    out = tmp_path / name / 'motion_generator'
    events = {}
    for sub in ('train', 'test'):
        values = []
        for path in summary.event_files(str(out / sub)):
            for e in summary.read_events(path):
                for v in e['values']:
                    payload = v['image']['encoded_image_string'] if 'image' in v else np.float32(v['simple_value']).tobytes()
                    values.append((e['step'], v['tag'], 'image' in v, payload))
        events[sub] = values
    with np.load(str(out / 'model.ckpt-1.npz')) as z:
        ckpt = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
    return events, ckpt


def test_train_py_resident_labels_equals_the_host_path(dev, dataset, tmp_path):
    """train.py --mode motion_generator, two steps with a summary, a test pass and a checkpoint at each: with --resident-labels the event
    files hold the same tags, scalars and image bytes and the checkpoint the same arrays as without -- after two runs WITHOUT the flag have
    been seen to agree with each other (the stage-2 step is run-to-run deterministic)."""
    ev_a, ck_a = _train(tmp_path, dataset, 'host_a', False)
    ev_b, ck_b = _train(tmp_path, dataset, 'host_b', False)
    assert ev_a == ev_b and ck_a == ck_b, 'two runs of the host path differ: the step is not deterministic'
    ev_r, ck_r = _train(tmp_path, dataset, 'resident', True)
    for sub in ('train', 'test'):
        tags = [t for _, t, _, _ in ev_a[sub]]
        assert 'im/image/0' in tags and 'im/image/1' in tags and 'real_pose_sequence/image/1' in tags and 'D_real' in tags, tags
        assert len(ev_a[sub]) == len(ev_r[sub])
        for a, r in zip(ev_a[sub], ev_r[sub]):
            assert a == r, (sub, a[:3], r[:3])
    assert sorted(ck_a) == sorted(ck_r) and len(ck_a) > 10
    for k in ck_a:
        assert ck_a[k] == ck_r[k], k
