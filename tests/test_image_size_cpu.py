"""CPU: one image size S from the YAML to the pixels -- the checker and its command-line override, the host loaders at a size of their
own (``render`` against the Pillow calls it stands for, written out in image_size_ref.py), the default left byte for byte as it was, and
the row tables of kpx_amd.resident at S applied in numpy against ``render``.  Every comparison is exact.  Nothing here needs a device."""
import os
import random

import numpy as np
import pytest
from PIL import Image

import image_size_ref as isr
import resident_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
VIDEOS = [(80, 60), (60, 80)]                    # a landscape and a portrait video; both upscale at 256
FRAMES = 12


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('image_size'))
    return root, ref.write_dataset(root, VIDEOS, frames=FRAMES)


def _loader(root, random_order=True, randomness=True, seed=5, **kw):
    from kpx_amd.data import ImagePairDataLoader
    return ImagePairDataLoader(root, 'train', random_order=random_order, randomness=randomness, rng=random.Random(seed),
                               np_rng=np.random.RandomState(seed), **kw)


def _index(names):
    from kpx_amd import resident as R
    return R.FrameIndex(names, VIDEOS, [FRAMES] * len(VIDEOS))


# ---------------------------------------------------------------------------------------------- configuration
def test_checker_accepts_multiples_of_16_from_32_to_256_and_names_key_and_value():
    from kpx_amd.data import check_image_size
    from kpx_amd._lib import KpxError
    for good in (32, 48, 128, 256):
        assert check_image_size(good) == good
    for bad in (0, 16, 40, 264, 272, '128', 128.0, None, True):
        with pytest.raises(KpxError) as e:
            check_image_size(bad)
        assert 'model.image_size' in str(e.value) and repr(bad) in str(e.value)


def test_command_line_override_beats_the_yaml_and_the_default_is_128():
    import yaml
    import train
    from kpx_amd._lib import KpxError
    penn = yaml.safe_load(open(os.path.join(os.path.dirname(HERE), 'configs', 'penn.yaml')))
    penn256 = yaml.safe_load(open(os.path.join(os.path.dirname(HERE), 'configs', 'penn256.yaml')))
    assert 'image_size' not in penn['model']                                         # the key is optional: configs/penn.yaml stays as it is
    assert penn256['model'].pop('image_size') == 256 and penn256 == penn             # penn256.yaml is penn.yaml plus the key
    assert train.config_image_size(penn) == 128
    assert train.config_image_size({'model': {'image_size': 256}}) == 256
    assert train.config_image_size({'model': {'image_size': 256}}, 48) == 48         # --image-size wins
    assert train.config_image_size({'model': {'image_size': 40}}, 64) == 64          # ... even over a YAML value the checker would refuse
    with pytest.raises(KpxError, match=r'model\.image_size = 40'):
        train.config_image_size({'model': {'image_size': 40}})
    with pytest.raises(KpxError, match=r'--image-size = 272'):
        train.config_image_size(penn, 272)
    for script in ('train', 'evaluate', 'make_pseudo_labels', 'animate'):            # the flag is on all four command lines
        assert "'--image-size'" in open(os.path.join(os.path.dirname(HERE), script + '.py')).read(), script
    assert train.parse_args(['--mode', 'detector_translator', '--config', 'c.yaml', '--image-size', '64']).image_size == 64
    assert train.parse_args(['--mode', 'detector_translator', '--config', 'c.yaml']).image_size is None


def test_loaders_and_the_still_fitter_refuse_a_bad_size(tree):
    from kpx_amd import stills
    from kpx_amd.data import KeypointDataLoader, SequenceDataLoader
    from kpx_amd._lib import KpxError
    root, _ = tree
    with pytest.raises(KpxError):
        _loader(root, image_size=40)
    with pytest.raises(KpxError):
        KeypointDataLoader(root, 'train', image_size=272)
    with pytest.raises(KpxError):
        SequenceDataLoader(root, 'train', 3, 2, image_size=16)
    with pytest.raises(KpxError):
        stills.fit_image(Image.new('RGB', (90, 70)), image_size=0)


# ---------------------------------------------------------------------------------------------- the default is what it was
@pytest.mark.parametrize('randomness', [True, False])
@pytest.mark.parametrize('random_order', [True, False])
def test_default_size_leaves_plans_and_bytes_unchanged(tree, randomness, random_order):
    root, _ = tree
    a, b = _loader(root, random_order, randomness, 7), _loader(root, random_order, randomness, 7, image_size=128)
    assert a.image_size == b.image_size == 128 and a.get_sample_shape() == b.get_sample_shape() == {'image': [128, 128, 3], 'future_image': [128, 128, 3]}
    want = [p for _ in range(3) for p in a.plans()]
    got = [p for _ in range(3) for p in b.plans()]
    assert got == want and a._rng.random() == b._rng.random() and a._np_rng.randint(1 << 30) == b._np_rng.randint(1 << 30)
    for p in want:
        for x, y in zip(a.render(p), b.render(p)):
            assert x.shape == (128, 128, 3) and x.dtype == np.uint8 and np.array_equal(x, y)


def test_default_size_of_the_other_loaders_and_the_still_fitter(tree):
    from kpx_amd import stills
    from kpx_amd.data import KeypointDataLoader, SequenceDataLoader
    root, _ = tree
    a, b = KeypointDataLoader(root, 'train'), KeypointDataLoader(root, 'train', image_size=128)
    fa, fb = a.render_video(1), b.render_video(1)
    assert fa[0].shape == (FRAMES, 128, 128, 3) and np.array_equal(fa[0], fb[0]) and fa[1:] == fb[1:]
    assert a.get_sample_shape()['image'] == [663, 128, 128, 3]
    small = KeypointDataLoader(root, 'train', image_size=48)
    assert small.render_video(0)[0].shape == (FRAMES, 48, 48, 3) and small.get_sample_shape()['image'] == [663, 48, 48, 3]
    assert next(small.sample_generator())['image'].shape == (663, 48, 48, 3)
    sa, sb = SequenceDataLoader(root, 'train', 3, 2), SequenceDataLoader(root, 'train', 3, 2, image_size=128)
    plan = sa.plan(0)
    assert np.array_equal(sa.render_start_image(plan), sb.render_start_image(plan)) and sa.get_sample_shape() == sb.get_sample_shape()
    s64 = SequenceDataLoader(root, 'train', 3, 2, with_image_seq=True, image_size=64)
    assert s64.render_start_image(plan).shape == (64, 64, 3) and s64.get_sample_shape()['real_im_seq'] == [32, 64, 64, 3]
    picture = ref.jpeg_frame(200, 150, 4)
    (ua, ia), (ub, ib) = stills.fit_image(picture), stills.fit_image(picture, image_size=128)
    assert np.array_equal(ua, ub) and ia == ib and ua.shape == (128, 128, 3)
    u64, i64 = stills.fit_image(picture, image_size=64)
    assert u64.shape == (64, 64, 3) and i64['resized_size'] == [85, 64]
    assert np.array_equal(u64, np.asarray(picture.resize([85, 64]).crop((85 / 2.0 - 32, 0, 85 / 2.0 + 32, 64))))


# ---------------------------------------------------------------------------------------------- render at S against Pillow, written out
@pytest.mark.parametrize('side', isr.SIDES)
def test_render_equals_the_restated_pillow_calls(tree, side):
    from kpx_amd import resident as R
    root, names = tree
    for randomness in (True, False):
        loader = _loader(root, random_order=False, randomness=randomness, image_size=side)
        assert loader.get_sample_shape() == {'image': [side, side, 3], 'future_image': [side, side, 3]}
        drawn = [p for _ in range(2) for p in loader.plans()]                        # the crop range int(side / ratio - S) is drawn from, too
        plans = drawn + ([p for name, (w, h) in zip(names, VIDEOS) for p in isr.enumerated_plans(name, w, h, side, FRAMES)] if randomness else [])
        for name, (w, h) in zip(names, VIDEOS):
            assert any(p.video == name for p in plans)
        for p in plans:
            got = loader.render(p)
            for g, idx in zip(got, (p.im_idx, p.fu_idx)):
                assert g.shape == (side, side, 3) and g.dtype == np.uint8
                assert np.array_equal(g, isr.pillow_render(R.frame_path(root, p.video, idx), p, side, randomness)), (side, randomness, p)
        if randomness:
            ratio = 60 / float(side)
            assert all(0 <= p.crop <= int(int(80 / ratio) - side) for p in drawn)


# ---------------------------------------------------------------------------------------------- the row tables at S
@pytest.mark.parametrize('side', isr.SIDES)
def test_row_tables_applied_in_numpy_reproduce_render(tree, side):
    from kpx_amd import resident as R
    root, names = tree
    planner = R.AugmentPlanner(_index(names), side)
    assert planner.image_size == side and planner.bands == side // R.BAND
    tabs, kernels = planner.tables.buffer(), R.filter_kernels()
    everything = []
    for randomness in (True, False):
        loader = _loader(root, random_order=False, randomness=randomness, image_size=side)
        if randomness:
            plans = [p for name, (w, h) in zip(names, VIDEOS) for p in isr.enumerated_plans(name, w, h, side, FRAMES)]
        else:
            plans = list(loader.plans())
        rows = planner.check_rows(planner.rows_for_plans(plans, randomness))
        assert rows.shape == (2 * len(plans), R.ROW_INTS)
        everything.append(rows)
        for k, plan in enumerate(plans):
            want = loader.render(plan)
            for which, idx in ((0, plan.im_idx), (1, plan.fu_idx)):
                frame = np.asarray(Image.open(R.frame_path(root, plan.video, idx)))
                tile, plain = isr.render_row(frame, rows[which * len(plans) + k], tabs, kernels, side)
                assert np.array_equal(tile, want[which]), (side, randomness, which, plan)
                assert np.array_equal(plain, np.asarray(isr.pillow_tile(R.frame_path(root, plan.video, idx), plan, side, randomness)))
    isr.assert_full_coverage(np.concatenate(everything))


def test_contrast_grey_is_pillows_rounded_mean_at_every_side():
    """(2 * sum + S^2) / (2 * S^2) in integers against int(mean + 0.5) in Python floats, on tiles whose mean sits on and beside a tie."""
    from PIL import ImageStat
    rs = np.random.RandomState(3)
    for side in (32, 48, 80, 128, 208, 256):
        for case in range(6):
            tile = np.full((side, side, 3), 37 + case, np.uint8)
            n = (side * side // 2 + (case - 2)) if case < 5 else 0               # half of the pixels one brighter: the mean is x.5 (+- a few pixels)
            flat = tile.reshape(-1, 3)
            flat[rs.permutation(side * side)[:max(n, 0)]] += 1
            want = int(ImageStat.Stat(Image.fromarray(tile).convert('L')).mean[0] + 0.5)
            assert isr.contrast_grey(tile) == want, (side, case)


# ---------------------------------------------------------------------------------------------- what the kernels cannot take
def test_check_rows_refuses_a_band_beyond_the_lds_limit_and_names_the_video():
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError
    index = R.FrameIndex(['small', 'big'], [(320, 270), (1700, 1300)], [2, 2])
    xmin, cnt, _ = R.resize_table(1300, 256)
    need = R.band_rows(xmin, cnt)
    assert need > 85 and 64 * 1024 < need * 256 * 3 <= R.LDS_BYTES                  # more than the default 64 KB of a workgroup, within the limit
    full = R.AugmentPlanner(index, 256)
    rows = np.array([full.row('small', 0), full.row('big', 1, x0=3)], np.int32)
    assert full.check_rows(rows) is rows and full.band_rows_cap == need
    tight = R.AugmentPlanner(index, 256, lds_bytes=64 * 1024)
    assert tight.band_rows_cap < need and tight.band_rows_cap * 256 * 3 <= 64 * 1024   # the launches' LDS follows the videos that fit
    assert tight.check_rows(rows[:1]) is not None
    with pytest.raises(KpxError, match=r'big.*%d bytes of LDS' % (need * 256 * 3)):
        tight.check_rows(rows)
    with pytest.raises(KpxError, match='crop window'):
        full.check_rows(np.array([full.row('small', 0, x0=60)], np.int32))           # 320 x 270 -> 303 x 256: x0 <= 47


def test_square_entries_refuse_bad_sizes_before_any_device_call():
    from kpx_amd import ops, resident as R
    from kpx_amd._lib import lib
    a = 1 << 20                                                                     # an aligned fake address: nothing may read it
    geometry = lambda side=48, cap=32, n=2, frames=a: lib.kpx_augment_geometry_sq_u8(frames, a, a, n, a, cap, side, a, a, None)
    filt = lambda side=48, n=2, kernels=a: lib.kpx_augment_filter_sq_f32(a, a, a, n, kernels, side, a, None)
    for side in (0, 16, 40, 264, 272, -48):
        assert geometry(side=side) == -1 and filt(side=side) == -1
    assert geometry(frames=None) == -1 and filt(kernels=None) == -1
    assert geometry(cap=R.BAND - 1) == -1 and geometry(n=R.MAX_ROWS + 1) == -1 and filt(n=-1) == -1
    for side in (32, 48, 128, 256):
        assert geometry(side=side, cap=R.LDS_BYTES // (side * 3) + 1) == -1           # one row more than the LDS of a workgroup holds
    assert geometry(n=0) == 0 and filt(n=0) == 0
    assert (ops.AUG_TILE_MIN, ops.AUG_TILE_MAX, ops.AUG_LDS_BYTES) == (R.TILE_MIN, R.TILE_MAX, R.LDS_BYTES)
    import re
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'kpx.h')).read()
    for name, value in (('TILE_MIN', R.TILE_MIN), ('TILE_MAX', R.TILE_MAX), ('LDS_BYTES', R.LDS_BYTES)):
        assert int(re.search(r'#define\s+KPX_AUG_%s\s+(\d+)' % name, src).group(1)) == value, name
    assert R.MAX_BAND_ROWS * R.TILE_MAX * 3 == R.LDS_BYTES
