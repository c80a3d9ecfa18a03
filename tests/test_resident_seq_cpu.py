"""CPU: the host side of stage 2's resident key-point labels (kpx_amd.resident, second half) -- the numpy restatement of
csrc/augment_seq.hip (resident_seq_ref.py) against ``SequenceDataLoader.render`` itself, bit pattern for bit pattern; table rows from
plans; the label store's refusals; the validation of rows; the command line.  Nothing here needs a device."""
import os
import re

import numpy as np
import pytest

import resident_seq_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp('seq')
    return root, ref.write_dataset(root)


def _planner(root, subset='train'):
    from kpx_amd import resident as R
    with open(os.path.join(str(root), subset + '_set.txt')) as f:
        listing = f.read().splitlines()
    return R.SequencePlanner(R.LabelIndex.scan(str(root), listing, ref.K), ref.N_ACTION)


def test_constants_mirror_the_header():
    from kpx_amd import resident as R
    from kpx_amd.data import N_SEQUENCE_LEN
    src = open(os.path.join(os.path.dirname(HERE), 'include', 'kpx.h')).read()
    for name, value in (('ROW_INTS', R.SEQ_ROW_INTS), ('ROTATE', R.SEQ_ROTATE), ('FLIP', R.SEQ_FLIP), ('SCALE', R.SEQ_SCALE),
                        ('LEN', R.SEQ_LEN), ('ANGLES', R.SEQ_ANGLES), ('MAX_ROWS', R.SEQ_MAX_ROWS), ('MAX_POINTS', R.SEQ_MAX_POINTS),
                        ('MAX_ACTIONS', R.SEQ_MAX_ACTIONS)):
        assert int(re.search(r'#define\s+KPX_SEQ_%s\s+(\d+)' % name, src).group(1)) == value, name
    assert R.SEQ_LEN == N_SEQUENCE_LEN and R.SEQ_SHORT == 17 and R.SEQ_ANGLE_MIN + R.SEQ_ANGLES == 16
    assert R.SEQ_MAX_ROWS * (R.SEQ_LEN * R.SEQ_MAX_POINTS + R.SEQ_MAX_ACTIONS) < 1 << 31          # the kernel's 32-bit thread index
    assert R.seq_trig().shape == (R.SEQ_ANGLES, 2) and R.seq_trig().dtype == np.float64


def test_dataset_covers_both_forms_and_signed_zeros(dataset):
    root, labels = dataset
    assert [int(n / 33) for n in ref.FRAMES] == [3, 2, 1, 1, 0, 0] and ref.last_im_idx(17) == 0 and ref.last_im_idx(33) == 0
    for a in labels.values():
        z = ref.bits(a)[a == 0]
        assert (z == 0).any() and (z != 0).any()                                                  # +0.0 and -0.0


@pytest.mark.parametrize('randomness', [True, False])
def test_restatement_equals_render(dataset, randomness):
    """rows_for_plans + the numpy restatement of the kernel == render + _collate on the hand-made plans, every bit."""
    from kpx_amd import resident as R
    root, _ = dataset
    ld = ref.loader(root, False, randomness)
    planner = _planner(root)
    plans = ref.hand_plans(randomness)
    if randomness:
        for v in set(p.video for p in plans):
            mine = [p for p in plans if p.video == v]
            assert set(p.angle for p in mine) == set(range(-15, 16)) and set(p.flip for p in mine) == {0, 1}
            assert set(p.scale for p in mine) == {0.7, 1.0, 1.2}
            assert set(p.im_idx for p in mine) == {0, ref.last_im_idx(mine[0].n_files)}
    rows = planner.check_rows(planner.rows_for_plans(plans))
    assert rows.shape == (len(plans), R.SEQ_ROW_INTS) and rows.dtype == np.int32
    assert set(rows[:, R.S_GAP].tolist()) == {0, 1, 2, 3}
    assert set(rows[:, R.S_FLAGS].tolist()) == ({R.SEQ_ROTATE | R.SEQ_SCALE, R.SEQ_ROTATE | R.SEQ_SCALE | R.SEQ_FLIP} if randomness else {0})
    want, got = ref.collated(ld, plans), ref.restate(planner, rows)
    for key in ('keypoints', 'real_seq', 'action_code'):
        assert got[key].shape == want[key].shape
        assert np.array_equal(ref.bits(got[key]), ref.bits(want[key])), key
    if randomness:                           # the comparison told the zeros' signs apart: both signs occur among the outputs
        z = ref.bits(want['real_seq'])[want['real_seq'] == 0]
        assert (z == 0).any() and (z != 0).any()


def test_a_fused_product_would_be_seen(dataset):
    """The check has teeth: the float32 rotation with c*x folded into the subtraction (one rounding less) differs from render."""
    root, labels = dataset
    a = labels[ref.video_name(1)].astype(np.float64)
    c, s = np.float64(np.float32(np.cos(np.radians(7.0)))), np.float64(np.float32(np.sin(np.radians(7.0))))
    sy = (s * a[..., 1]).astype(np.float32).astype(np.float64)
    plain = ((c * a[..., 0]).astype(np.float32).astype(np.float64) - sy).astype(np.float32)
    fused = (c * a[..., 0] - sy).astype(np.float32)          # exact in float64: 24 x 24 bit product minus a float32
    assert 0.05 < np.mean(plain != fused) < 0.5


def test_rows_round_trip_the_plan(dataset):
    from kpx_amd import resident as R
    root, _ = dataset
    planner = _planner(root)
    plans = ref.hand_plans(True) + ref.hand_plans(False)
    rows = planner.rows_for_plans(plans)
    with open(os.path.join(str(root), 'train_set.txt')) as f:
        listing = f.read().splitlines()
    for p, r in zip(plans, rows):
        assert planner.index.names[r[R.S_VIDEO]] == p.video and r[R.S_IM_IDX] == p.im_idx and r[R.S_GAP] == int(p.n_files / 33)
        assert r[R.S_ACTION] == int(listing[p.index].split()[1])
        if p.angle is None:
            assert r[R.S_FLAGS] == 0
        else:
            assert r[R.S_FLAGS] == R.SEQ_ROTATE | R.SEQ_SCALE | (R.SEQ_FLIP if p.flip else 0)
            assert r[R.S_ANGLE] + R.SEQ_ANGLE_MIN == p.angle
            assert np.array([r[R.S_SCALE_LO], r[R.S_SCALE_HI]], np.int32).view(np.float64)[0] == p.scale
    assert planner.index.names == [ref.video_name(v) for v in range(len(ref.FRAMES))]             # the video listed twice is stored once
    assert planner.index.n_frames.tolist() == list(ref.FRAMES)


@pytest.mark.parametrize('random_order,randomness', [(True, True), (False, False)])
def test_plans_from_the_store_equal_plans_from_the_files(dataset, random_order, randomness):
    root, _ = dataset
    a, b = ref.loader(root, random_order, randomness, seed=3), ref.loader(root, random_order, randomness, seed=3)
    b._labels = _planner(root).index
    b._data_dir = os.path.join(str(root), 'nowhere')         # a plan() that listed a directory would fail here
    want = [p for _ in range(3) for p in a.plans()]
    assert [p for _ in range(3) for p in b.plans()] == want and len(want) == 3 * a.length()
    assert a._rng.random() == b._rng.random() and a._np_rng.randint(1 << 30) == b._np_rng.randint(1 << 30)


def test_rows_the_kernel_cannot_take_are_rejected_on_the_host(dataset):
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError, lib
    root, _ = dataset
    planner = _planner(root)
    v = ref.video_name
    good = np.array([planner.row(v(0), 1, 3, 4, angle=-15, flip=1, scale=0.7),      # 100 frames: 1 + 32 * 3 = 97
                     planner.row(v(4), 15, 0, 8),                                   # 32 frames, short form: 15 + 16 = 31
                     planner.row(v(3), 0, 1, 0, angle=15, scale=1.2)], np.int32)    # 33 frames: 0 + 32
    assert planner.check_rows(good) is good

    def bad(col, value, r=0):
        rows = good.copy()
        rows[r, col] = value
        with pytest.raises(KpxError):
            planner.check_rows(rows)
    bad(R.S_VIDEO, len(ref.FRAMES)); bad(R.S_VIDEO, -1)                      # outside the store
    bad(R.S_IM_IDX, 4); bad(R.S_IM_IDX, -1); bad(R.S_GAP, 4); bad(R.S_GAP, -1)     # 4 + 96 = 100; 1 + 32 * 4
    bad(R.S_IM_IDX, 16, r=1); bad(R.S_GAP, 1, r=1)                           # short form: 16 + 16 = 32; gap 1 would read row 47
    bad(R.S_IM_IDX, 1, r=2); bad(R.S_VIDEO, 5, r=2)                          # 33 frames; the 17-frame video has no 33 rows
    bad(R.S_ANGLE, R.SEQ_ANGLES); bad(R.S_ANGLE, -1)
    bad(R.S_ACTION, ref.N_ACTION); bad(R.S_ACTION, -1)
    bad(R.S_FLAGS, 8)
    with pytest.raises(KpxError):
        planner.check_rows(good.astype(np.int64))
    with pytest.raises(KpxError):
        planner.check_rows(np.repeat(good, R.SEQ_MAX_ROWS // 3 + 1, axis=0))      # more rows than the stated cap
    with pytest.raises(KpxError):
        planner.check_rows(good[:0])
    # the C entry refuses null pointers and sizes outside the header's bounds before any device call
    a = 1 << 20
    f = lib.kpx_keypoint_seq_augment_f32
    assert f(None, a, a, 2, 5, 9, a, a, a, a, None) == -1 and f(a, a, a, 2, 5, 9, a, a, a, None, None) == -1
    assert f(a, a, a, R.SEQ_MAX_ROWS + 1, 5, 9, a, a, a, a, None) == -1 and f(a, a, a, -1, 5, 9, a, a, a, a, None) == -1
    assert f(a, a, a, 2, R.SEQ_MAX_POINTS + 1, 9, a, a, a, a, None) == -1 and f(a, a, a, 2, 5, 0, a, a, a, a, None) == -1
    assert f(a, a, a, 0, 5, 9, a, a, a, a, None) == 0


def test_the_store_refuses_wrong_label_files(tmp_path):
    from kpx_amd import resident as R
    from kpx_amd._lib import KpxError
    ref.write_dataset(tmp_path / 'd', frames=(40, 17))
    listing = ['%s 0' % ref.video_name(0), '%s 1' % ref.video_name(1)]
    R.LabelIndex.scan(str(tmp_path / 'd'), listing, ref.K)
    p = str(tmp_path / 'd' / 'pseudo_labels' / '0002.npy')
    a = np.load(p)
    np.save(p, a.astype(np.float64))
    with pytest.raises(KpxError, match=r'frames/0002.*float64'):
        R.LabelIndex.scan(str(tmp_path / 'd'), listing, ref.K)
    np.save(p, a[:16])
    with pytest.raises(KpxError, match=r'frames/0002.*16 label rows for 17 frame files'):
        R.LabelIndex.scan(str(tmp_path / 'd'), listing, ref.K)
    np.save(p, a)
    with pytest.raises(KpxError, match=r'frames/0001'):
        R.LabelIndex.scan(str(tmp_path / 'd'), listing, ref.K + 1)               # not [len, n_points, 2]
    np.save(p, np.concatenate([a, a]))                                           # more label rows than frames: fine
    idx = R.LabelIndex.scan(str(tmp_path / 'd'), listing, ref.K)
    assert idx.label_rows.tolist() == [40, 34] and idx.n_frames.tolist() == [40, 17] and idx.offsets.tolist() == [0, 40 * ref.K * 2]
    assert np.array_equal(idx.array(ref.video_name(1)), np.concatenate([a, a]))


def test_resident_labels_flag_is_an_error_outside_stage_two(capsys):
    import train
    for extra in (['--mode', 'detector_translator'], ['--mode', 'motion_generator', '--synthetic']):
        with pytest.raises(SystemExit):
            train.main(extra + ['--config', 'unused.yaml', '--resident-labels'])
        assert '--resident-labels keeps pseudo labels in HBM' in capsys.readouterr().err      # the flag is known; the combination is refused
    with pytest.raises(SystemExit):
        train.main(['--mode', 'motion_generator', '--config', 'unused.yaml', '--resident-data'])
    assert '--resident-data keeps JPEG frames in HBM' in capsys.readouterr().err


def test_resident_batches_refuse_a_cpu_device(dataset):
    from kpx_amd._lib import KpxError
    root, _ = dataset
    with pytest.raises(KpxError):
        ref.loader(root, True, True).batches(2, 'cpu', resident=True)
