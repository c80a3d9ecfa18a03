"""CPU: the host side of the resident-frame input path (kpx_amd.resident) -- the integer / float32 tables the augmentation kernels are
driven by, applied in numpy (resident_ref.py) and compared with PIL itself, every byte equal; the plan stream drawn from a frame table
instead of the files; the store's bookkeeping and the validation of table rows.  Nothing here needs a device."""
import os
import random
import re

import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageFilter

import resident_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(480, 270), (270, 480), (320, 240), (486, 360), (128, 128), (641, 359), (129, 128)]


jpeg_frame = ref.jpeg_frame


def resized_tile(w, h, seed):
    from kpx_amd.data import _resized_size
    rw, rh, _ = _resized_size(w, h)
    return jpeg_frame(w, h, seed).resize([rw, rh]).crop((0, 0, 128, 128))


def test_constants_mirror_the_header():
    from kpx_amd import resident as R
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'kpx.h')).read()
    for name, value in (('ROW_INTS', R.ROW_INTS), ('FLIP', R.FLIP), ('ROTATE', R.ROTATE), ('IDENTITY', R.IDENTITY), ('BAND', R.BAND),
                        ('BANDS', R.BANDS), ('KERNEL_FLOATS', R.KERNEL_FLOATS), ('MAX_SIDE', R.MAX_SIDE), ('MAX_TAPS', R.MAX_TAPS),
                        ('MAX_BAND_ROWS', R.MAX_BAND_ROWS), ('MAX_ROWS', R.MAX_ROWS)):
        assert int(re.search(r'#define\s+KPX_AUG_%s\s+(\d+)' % name, src).group(1)) == value, name
    assert R.BAND * R.BANDS == 128 and R.MAX_BAND_ROWS * 128 * 3 <= 64 * 1024          # the default LDS limit of a workgroup


@pytest.mark.parametrize('w,h', SIZES)
def test_resize_tables_equal_pil(w, h):
    from kpx_amd import resident as R
    from kpx_amd.data import _resized_size
    im = jpeg_frame(w, h, 1)
    rw, rh, _ = _resized_size(w, h)
    got = ref.resize(np.asarray(im), R.resize_table(w, rw), R.resize_table(h, rh))
    assert np.array_equal(got, np.asarray(im.resize([rw, rh])))
    for n_in, n_out in ((w, rw), (h, rh)):
        xmin, cnt, k = R.resize_table(n_in, n_out)
        assert k.shape[1] <= R.MAX_TAPS and (xmin >= 0).all() and (xmin + cnt <= n_in).all() and (cnt >= 1).all()
        assert 255 * int(np.abs(k.astype(np.int64)).sum(1).max()) < 1 << 31             # the kernels' 32-bit sums
        assert R.band_rows(xmin, cnt) <= R.MAX_BAND_ROWS


@pytest.mark.parametrize('w,h', SIZES)
def test_rotate_constants_equal_pil(w, h):
    from kpx_amd import resident as R
    im = jpeg_frame(w, h, 2)
    a = np.asarray(im)
    for angle in range(-10, 11):
        c = R.rotate_constants(w, h, angle)
        assert (c is None) == (angle == 0)
        assert np.array_equal(ref.rotate(a, c), np.asarray(im.rotate(angle))), angle
        if c is not None:                                                               # |a1*y + a0*x + a2| stays far inside 32 bits
            assert max(abs(c[0]), abs(c[1]), abs(c[3]), abs(c[4])) <= 65536 and max(abs(c[2]), abs(c[5])) < 1 << 29


@pytest.mark.parametrize('w,h', SIZES)
def test_kernel_coefficients_equal_pil(w, h):
    from kpx_amd import resident as R
    from kpx_amd.data import _KERNEL_FILTERS
    tile = resized_tile(w, h, 3)
    kernels = R.filter_kernels()
    for i, f in enumerate(_KERNEL_FILTERS):
        assert np.array_equal(ref.kernel_filter(np.asarray(tile), kernels[i]), np.asarray(tile.filter(f))), f.name


@pytest.mark.parametrize('w,h', SIZES)
def test_enhancer_blends_equal_pil(w, h):
    from kpx_amd import resident as R
    from kpx_amd.data import _ENHANCERS
    tile = resized_tile(w, h, 4)
    a = np.asarray(tile)
    kernels = R.filter_kernels()
    assert _ENHANCERS[6][0] is ImageEnhance.Sharpness and _ENHANCERS[9][0] is ImageEnhance.Contrast
    for filt, (enhancer, lo, hi) in _ENHANCERS.items():
        for val in (lo, hi, 9, 10, 11):
            f = val * 0.1
            got = ref.enhance(a, filt, np.float32(f), f == 1.0, kernels)
            assert np.array_equal(got, np.asarray(enhancer(tile).enhance(f))), (filt, val)


# ---------------------------------------------------------------------------------------------- the whole composition, rows from plans
def _fixture_dataset(root):
    golden = np.load(os.path.join(HERE, 'golden', 'image_pair_ref.npz'))
    for k, rel in enumerate(str(n) for n in golden['file_names']):
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(golden['file_%03d' % k].tobytes())
    (root / 'train_set.txt').write_bytes(golden['listing'].tobytes())
    return [line.split()[0] for line in golden['listing'].tobytes().decode().splitlines()]


def _loader(root, random_order, randomness, seed):
    from kpx_amd.data import ImagePairDataLoader
    return ImagePairDataLoader(str(root), 'train', random_order=random_order, randomness=randomness, rng=random.Random(seed),
                               np_rng=np.random.RandomState(seed))


def _table_index(root, names):
    """A FrameIndex written down from what the files say -- then used WITHOUT the files."""
    from kpx_amd import resident as R
    sizes, counts, seen = [], [], []
    for v in names:
        if v in seen:
            continue
        seen.append(v)
        files = sorted(os.listdir(str(root / v)))
        counts.append(len(files))
        with Image.open(str(root / v / files[0])) as im:
            sizes.append(im.size)
    return R.FrameIndex(seen, sizes, counts)


@pytest.mark.parametrize('randomness', [True, False])
@pytest.mark.parametrize('random_order', [True, False])
@pytest.mark.parametrize('seed', [5, 11])
def test_plans_from_a_frame_table_equal_plans_from_the_files(tmp_path, randomness, random_order, seed):
    names = _fixture_dataset(tmp_path / 'data')
    bare = tmp_path / 'bare'                     # the listing only: a plan() that looked at a frame file would fail here
    bare.mkdir()
    (bare / 'train_set.txt').write_bytes((tmp_path / 'data' / 'train_set.txt').read_bytes())
    a = _loader(tmp_path / 'data', random_order, randomness, seed)
    b = _loader(bare, random_order, randomness, seed)
    b.attach_frames(_table_index(tmp_path / 'data', names))
    want = [p for _ in range(3) for p in a.plans()]
    got = [p for _ in range(3) for p in b.plans()]
    assert got == want and len(got) == 3 * a.length()
    assert a._rng.random() == b._rng.random() and a._np_rng.randint(1 << 30) == b._np_rng.randint(1 << 30)      # both streams consumed alike


def test_resident_iterator_shares_the_plan_stream_code():
    from kpx_amd.data import _DeviceBatcher
    from kpx_amd.resident import ResidentBatcher
    assert ResidentBatcher._plan_stream is _DeviceBatcher._plan_stream and ResidentBatcher.SHUFFLE_BUFFER == _DeviceBatcher.SHUFFLE_BUFFER


@pytest.mark.parametrize('randomness', [True, False])
def test_rows_from_plans_reproduce_render(tmp_path, randomness):
    """rows_for_plans + the numpy restatement of the kernels == ImagePairDataLoader.render (PIL) on the fixture videos."""
    from kpx_amd import resident as R
    names = _fixture_dataset(tmp_path)
    loader = _loader(tmp_path, True, randomness, 7)
    planner = R.AugmentPlanner(_table_index(tmp_path, names))
    tabs, kernels = planner.tables.buffer(), R.filter_kernels()
    plans = [p for _ in range(4) for p in loader.plans()]
    rows = planner.check_rows(planner.rows_for_plans(plans, randomness))
    assert rows.shape == (24, R.ROW_INTS) and rows.dtype == np.int32
    for k, plan in enumerate(plans):
        want = loader.render(plan)
        for which, idx in ((0, plan.im_idx), (1, plan.fu_idx)):
            frame = np.asarray(Image.open(R.frame_path(str(tmp_path), plan.video, idx)))
            assert np.array_equal(ref.render_row(frame, rows[which * len(plans) + k], tabs, kernels), want[which]), (k, which, plan)


# ---------------------------------------------------------------------------------------------- bookkeeping and validation
def test_store_layout_is_aligned_and_in_listing_order():
    from kpx_amd import resident as R
    offsets, first, total = R.store_layout([(480, 270, 3), (129, 128, 2), (5, 7, 4)])
    assert first.tolist() == [0, 3, 5] and len(offsets) == 9 and offsets.dtype == np.int64
    assert (offsets % 16 == 0).all() and (np.diff(offsets) > 0).all() and offsets[0] == 0
    sizes = [480 * 270 * 3] * 3 + [129 * 128 * 3] * 2 + [105] * 4
    assert all(offsets[i] + sizes[i] <= (offsets[i + 1] if i + 1 < 9 else total) for i in range(9))
    assert all(offsets[i + 1] - (offsets[i] + sizes[i]) < 16 for i in range(8))        # no more padding than the alignment needs
    idx = R.FrameIndex(['a', 'b'], [(480, 270), (270, 480)], [3, 2])
    assert idx.frame_number('b', 1) == 4 and idx.count('a') == 3 and idx.size('b') == (270, 480) and idx.total_bytes == 5 * 480 * 270 * 3


def test_a_store_that_does_not_fit_raises_before_allocating(tmp_path):
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError
    with pytest.raises(KpxError, match=str(5 * 480 * 270 * 3)):
        R.FrameIndex(['a', 'b'], [(480, 270), (270, 480)], [3, 2], max_bytes=5 * 480 * 270 * 3 - 1)
    names = _fixture_dataset(tmp_path)
    with pytest.raises(KpxError, match='max_bytes'):
        R.FrameIndex.scan(str(tmp_path), names, max_bytes=1000)                          # the scan is host work: no device is touched


def _write_video(root, name, frames):
    os.makedirs(os.path.join(str(root), name))
    for i, im in enumerate(frames):
        im.save(os.path.join(str(root), name, '%06d.jpg' % (i + 1)), format='JPEG', quality=90)


def test_grey_frames_and_mixed_sizes_raise_with_the_file_name(tmp_path):
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError
    rgb = lambda w, h: Image.fromarray(np.full((h, w, 3), 90, np.uint8))
    _write_video(tmp_path / 'g', 'v0', [rgb(160, 140), rgb(160, 140).convert('L'), rgb(160, 140)])
    with pytest.raises(KpxError, match=r'v0.000002\.jpg'):
        R.FrameIndex.scan(str(tmp_path / 'g'), ['v0 0'])
    _write_video(tmp_path / 's', 'v0', [rgb(160, 140), rgb(160, 140)])
    _write_video(tmp_path / 's', 'v1', [rgb(160, 140), rgb(160, 140), rgb(140, 160)])
    with pytest.raises(KpxError, match=r'v1.000003\.jpg'):
        R.FrameIndex.scan(str(tmp_path / 's'), ['v0 0', 'v1 1'])
    idx = R.FrameIndex.scan(str(tmp_path / 's'), ['v0 0', 'v0 3'])                       # a video listed twice is stored once
    assert idx.names == ['v0'] and idx.n_frames.tolist() == [2]


def test_resident_data_flag_is_an_error_outside_the_frame_pipeline(capsys):
    import train
    for extra in (['--mode', 'motion_generator'], ['--mode', 'detector_translator', '--synthetic']):
        with pytest.raises(SystemExit):
            train.main(extra + ['--config', 'unused.yaml', '--resident-data'])
        assert '--resident-data keeps JPEG frames in HBM' in capsys.readouterr().err      # the flag is known; the combination is refused


def test_resident_batches_refuse_a_cpu_device(tmp_path):
    from kpx_amd._lib import KpxError
    _fixture_dataset(tmp_path)
    with pytest.raises(KpxError):
        _loader(tmp_path, True, True, 1).batches(2, 'cpu', resident=True)


def test_rows_the_kernels_cannot_take_are_rejected_on_the_host():
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError, lib
    planner = R.AugmentPlanner(R.FrameIndex(['a', 'b'], [(480, 270), (270, 480)], [3, 2]))
    good = np.array([planner.row('a', 2, angle=-7, x0=99, flip=1, filt=9, filt_val=30), planner.row('b', 0, y0=40, filt=3)], np.int32)
    assert planner.check_rows(good) is good
    assert good[0, R.R_FLAGS] == R.FLIP | R.ROTATE and good[1, R.R_FLAGS] == 0
    assert planner.row('a', 0, filt=7, filt_val=10)[R.R_FLAGS] == R.IDENTITY
    assert np.array([planner.row('a', 0, filt=8, filt_val=9)[R.R_FVAL]], np.int32).view(np.float32)[0] == np.float32(9 * 0.1)

    def bad(col, value, r=0):
        rows = good.copy()
        rows[r, col] = value
        with pytest.raises(KpxError):
            planner.check_rows(rows)
    bad(R.R_FRAME, 5); bad(R.R_FRAME, -1)                  # outside the store
    bad(R.R_FRAME, 3)                                      # a frame of the other video: the size no longer fits
    bad(R.R_X0, 100); bad(R.R_X0, -1); bad(R.R_Y0, 1)      # 480 x 270 resizes to 227 x 128: x0 <= 99, y0 = 0
    bad(R.R_Y0, 100, r=1)                                  # 270 x 480 resizes to 128 x 227
    bad(R.R_FILT, 10); bad(R.R_FILT, -2)
    bad(R.R_FLAGS, 8)
    bad(R.R_HTAB, good[1, R.R_HTAB]); bad(R.R_VSTRIDE, 3); bad(R.R_W, 481)
    bad(R.R_A0, 65537); bad(R.R_A2, 1 << 29)
    with pytest.raises(KpxError):
        planner.check_rows(good.astype(np.int64))
    with pytest.raises(KpxError):
        planner.row('a', 3)                                # 'a' has three frames
    with pytest.raises(KpxError):
        R.FrameIndex(['big'], [(4096, 128)], [1])          # a side above KPX_AUG_MAX_SIDE
    with pytest.raises(KpxError):
        R.AugmentPlanner(R.FrameIndex(['fine'], [(2048, 1100)], [1]))    # 1100 -> 128 rows: more than KPX_AUG_MAX_TAPS taps
    # the C entries refuse null pointers and sizes outside the header's bounds before any device call
    a = 1 << 20
    assert lib.kpx_augment_geometry_u8(None, a, a, 2, a, 64, a, a, None) == -1
    assert lib.kpx_augment_geometry_u8(a, a, a, 2, a, R.MAX_BAND_ROWS + 1, a, a, None) == -1
    assert lib.kpx_augment_geometry_u8(a, a, a, R.MAX_ROWS + 1, a, 64, a, a, None) == -1
    assert lib.kpx_augment_filter_f32(a, a, a, 2, None, a, None) == -1
    assert lib.kpx_augment_filter_f32(a, a, a, -1, a, a, None) == -1
    assert lib.kpx_augment_geometry_u8(a, a, a, 0, a, 64, a, a, None) == 0 and lib.kpx_augment_filter_f32(a, a, a, 0, a, a, None) == 0
