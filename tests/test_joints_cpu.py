"""CPU: the host side of the landmark regression (kpx_amd/joints.py, make_pseudo_labels.py --joints) -- the coordinate map against the
loader's own rendering, the label reader, the solver on a planted linear problem, the summary, the script's argument rules and the three
entries' refusals.  Nothing here needs a GPU; the kernels are held to tests/joints_ref.py in test_joints_gpu.py."""
import json
import math

import numpy as np
import pytest

import joints_ref as R


def _J():
    from kpx_amd import joints
    return joints


# ------------------------------------------------------------------------------------------------ crop_map against the loader
# A black frame with one white 9 x 9 square, written as JPEG, rendered by KeypointDataLoader.render_video; the intensity centroid of the
# crop, in normalised units, against crop_map applied to the square's centre.  Measured with the loader here (Pillow 12.2, bicubic resize),
# the largest deviation over the two axes, in normalised units (one pixel of the crop is 2 / 127 = 0.01575):
#
#     frame      correct map   no pixel-centre term in the resize   unrounded crop box
#     320 x 240  0.000078      0.003614                             0.000078  (the box has whole edges: the same map)
#     240 x 320  0.000122      0.003797                             0.000122  (alike)
#     321 x 241  0.000289      0.003993                             0.000289  (alike: int(321 / (241 / 128)) = 170 is even)
#     323 x 241  0.000007      0.003704                             0.007873  (resized width 171: the box starts at 21.5, PIL crops at 22)
#
# 321 x 241 does not give an odd resized width, so the fourth frame is there for the case the third was meant to be.  The smallest deviation
# a wrong convention produces is 0.003614; the bound is half of it, six times the correct map's largest.
CROP_BOUND = 0.003614 / 2
CROP_CASES = ((320, 240, 170, 90), (240, 320, 100, 180), (321, 241, 150, 131), (323, 241, 181, 77))      # w, h, the square's corner


def _wrong_maps(w, h, res=128):
    from kpx_amd.data import center_crop_box
    box, ratio = center_crop_box(w, h, res)
    rw, rh = int(w / ratio), int(h / ratio)
    sx, sy, g = rw / float(w), rh / float(h), 2.0 / (res - 1.0)
    left, top = int(round(box[0])), int(round(box[1]))
    no_centre = np.array([sx * g, -left * g - 1.0, sy * g, -top * g - 1.0])
    unrounded = np.array([sx * g, (0.5 * sx - 0.5 - box[0]) * g - 1.0, sy * g, (0.5 * sy - 0.5 - box[1]) * g - 1.0])
    return no_centre, unrounded, (box[0] != left or box[1] != top)


@pytest.mark.parametrize('case', CROP_CASES, ids=lambda c: '%dx%d' % c[:2])
def test_crop_map_follows_the_loader(case, tmp_path):
    from PIL import Image
    from kpx_amd.data import KeypointDataLoader
    w, h, x0, y0 = case
    frames = tmp_path / 'frames' / '0001'
    frames.mkdir(parents=True)
    im = np.zeros((h, w, 3), np.uint8)
    im[y0:y0 + 9, x0:x0 + 9] = 255
    for i in range(2):
        Image.fromarray(im).save(str(frames / ('%06d.jpg' % (i + 1))), quality=95)
    (tmp_path / 'train_set.txt').write_text('frames/0001 0\n')
    loader = KeypointDataLoader(str(tmp_path), 'train')
    assert loader.frame_size(0) == (w, h) and loader.video_ids() == [1]
    crop, n, vid = loader.render_video(0)
    assert crop.shape == (2, 128, 128, 3) and n == 2 and vid == 1
    a = crop[0].astype(np.float64).sum(axis=-1)
    ys, xs = np.mgrid[0:128, 0:128]
    centroid = -1.0 + 2.0 * np.array([(a * xs).sum(), (a * ys).sum()]) / a.sum() / 127.0
    centre = np.array([x0 + 4.0, y0 + 4.0])                                  # 0-based pixel positions

    def deviation(m):
        return float(np.abs(np.array([m[0] * centre[0] + m[1], m[2] * centre[1] + m[3]]) - centroid).max())

    good = deviation(_J().crop_map(w, h))
    no_centre, unrounded, fractional = _wrong_maps(w, h)
    print('crop_map %dx%d: correct %.6f, no pixel centre %.6f, unrounded box %.6f' % (w, h, good, deviation(no_centre), deviation(unrounded)))
    assert good <= CROP_BOUND
    assert deviation(no_centre) > CROP_BOUND                                 # the bound tells the conventions apart
    assert fractional == ((w, h) == (323, 241))
    if fractional:
        assert deviation(unrounded) > CROP_BOUND


def test_crop_map_by_hand_and_refusals():
    J = _J()
    # 256 x 128: ratio 1, no resize, the crop starts at column 64: x -> -1 + 2 (x - 64) / 127, y -> -1 + 2 y / 127
    assert np.allclose(J.crop_map(256, 128), [2 / 127.0, -1 - 128 / 127.0, 2 / 127.0, -1.0], rtol=0, atol=1e-15)
    a = J.crop_map(320, 240)
    b = J.crop_map(240, 320)
    assert np.array_equal(a[[2, 3, 0, 1]], b) and a.dtype == np.float64
    assert a[0] != a[2]                                                      # int() truncates the longer side: the axis scales differ
    with pytest.raises(ValueError):
        J.crop_map(0, 10)
    assert '0-BASED' in J.crop_map.__doc__


# ------------------------------------------------------------------------------------------------ read_labels
def _penn_fields(f, j=13, seed=0):
    rs = np.random.RandomState(seed)
    return {'x': rs.uniform(0, 300, size=(f, j)), 'y': rs.uniform(0, 200, size=(f, j)), 'visibility': (rs.uniform(size=(f, j)) < 0.8).astype(np.uint8),
            'bbox': np.sort(rs.uniform(0, 300, size=(f, 4)), axis=1)[:, [0, 1, 2, 3]], 'nframes': np.array([[f]]), 'action': 'jump',
            'dimensions': np.array([[240, 320, f]])}


def test_read_labels_round_trip(tmp_path):
    from scipy.io import savemat
    J = _J()
    fields = _penn_fields(7)
    savemat(str(tmp_path / '0001.mat'), fields)
    np.savez(str(tmp_path / '0002.npz'), **{k: fields[k] for k in J.LABEL_FIELDS})
    for name in ('0001.mat', '0002.npz'):
        got = J.read_labels(str(tmp_path / name), n_frames=7)
        assert got['nframes'] == 7 and got['x'].dtype == np.float64 and got['visibility'].dtype == bool
        for key in ('x', 'y', 'bbox'):
            assert np.array_equal(got[key], fields[key]), (name, key)
        assert np.array_equal(got['visibility'], fields['visibility'] != 0)
        assert J.read_labels(str(tmp_path / name))['nframes'] == 7          # the frame count is optional
        with pytest.raises(ValueError, match='the video has 8'):
            J.read_labels(str(tmp_path / name), n_frames=8)
    assert J.find_label_file(str(tmp_path), 1).endswith('0001.mat') and J.find_label_file(str(tmp_path), 2).endswith('0002.npz')
    assert J.find_label_file(str(tmp_path), 3) is None
    bad = dict(fields, bbox=fields['bbox'][:6])                              # one box short of nframes
    savemat(str(tmp_path / '0003.mat'), bad)
    with pytest.raises(ValueError, match='bbox'):
        J.read_labels(str(tmp_path / '0003.mat'))
    np.savez(str(tmp_path / '0004.npz'), x=fields['x'], y=fields['y'])
    with pytest.raises(ValueError, match='no field visibility, bbox, nframes'):
        J.read_labels(str(tmp_path / '0004.npz'))


# ------------------------------------------------------------------------------------------------ the planted linear problem
F, K, NJ, SIGMA = 400, 15, 13, 0.01
D = 2 * K + 1
SPREAD = 0.8                                                                 # key points uniform in [-SPREAD, SPREAD]


def _planted(seed, a=None, f=F):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-SPREAD, SPREAD, size=(f, K, 2)).astype(np.float32)
    if a is None:
        a = rs.uniform(-0.3, 0.3, size=(NJ, D, 2)) / math.sqrt(D)
    phi, _ = R.features(pts)
    target = (np.einsum('fd,jdc->fjc', phi, a) + SIGMA * rs.standard_normal((f, NJ, 2))).astype(np.float32)
    return pts, target, a


def _zero():
    return np.zeros((NJ, D, D)), np.zeros((NJ, D, 2)), np.zeros(NJ, np.int64)


def test_solve_recovers_a_planted_map_and_scores_at_the_noise_level():
    """Least squares on F frames with independent features: a coefficient of a feature of standard deviation s has standard error sigma /
    (sqrt(F) s), times sqrt(F / (F - D)) for the D fitted coefficients; the features are uniform in +-0.8 (s = 0.8 / sqrt(3)), the bias has
    s = 1.  The tolerance is six such errors for the smaller s, 6 * 0.01 / (20 * 0.462) * 1.04 = 0.0068: the float32 rounding of the targets
    (6e-8) and the default ridge (1e-6 of the coefficients) do not show at that scale.
    The error of an entry of a fresh split is the length of a 2-vector whose components are the noise (sigma) plus the fit's own error
    (variance sigma^2 D / F on average): a Rayleigh mean between sigma sqrt(pi / 2) and sigma sqrt(pi / 2) sqrt(1 + D / F), each widened by five
    standard errors of a mean over F * J entries, 5 sqrt((4 - pi) / pi) / sqrt(F J) = 3.6 %."""
    J = _J()
    pts, target, a = _planted(1)
    mask = np.ones((F, NJ), np.uint8)
    mask[:, 3] = 0                                                           # a joint that is never annotated
    G, Bm, n = R.moments_add(pts, target, mask, *_zero())
    assert n.tolist() == [0 if j == 3 else F for j in range(NJ)]
    W = J.solve(G, Bm, n)
    assert W.shape == (NJ, D, 2) and np.isnan(W[3]).all() and np.isfinite(np.delete(W, 3, axis=0)).all()
    tol = 6.0 * SIGMA / (math.sqrt(F) * SPREAD / math.sqrt(3.0)) * math.sqrt(F / float(F - D))
    worst = np.abs(np.delete(W - a, 3, axis=0)).max()
    print('planted map: worst coefficient error %.5f (tolerance %.5f)' % (worst, tol))
    assert worst <= tol
    # a fresh split, scored by the restatement and reduced by summarise
    pts2, target2, _ = _planted(2, a)
    mask2 = np.ones((F, NJ), np.uint8)
    norm2 = np.full(F, 2.0, np.float32)
    alphas = [0.005, 0.05]
    _, _, _, sum_err, count, pck_count, hit_count, _, _ = R.joint_scores(pts2, target2, mask2, norm2, W, alphas)
    assert np.isnan(sum_err[3]) and count[3] == F
    rec = J.video_record('test', 5, F, sum_err, count, pck_count, hit_count)
    s = J.summarise([rec], NJ, alphas, 128, solved=np.isfinite(W).all(axis=(1, 2)))
    o = s['subsets']['test']
    rayleigh, rel = SIGMA * math.sqrt(math.pi / 2.0), 5.0 * math.sqrt((4.0 - math.pi) / math.pi) / math.sqrt(F * (NJ - 1))
    lo, hi = rayleigh * (1.0 - rel), rayleigh * math.sqrt(1.0 + D / float(F)) * (1.0 + rel)
    print('planted map: test error %.6f in [%.6f, %.6f]' % (o['err'], lo, hi))
    assert lo <= o['err'] <= hi and o['scored_joints'] == NJ - 1
    assert o['err_px'] == o['err'] * 63.5
    assert math.isnan(o['per_joint']['err'][3]) and math.isnan(o['per_joint']['pck'][3][0]) and all(math.isfinite(v) for v in o['per_joint']['err'][:3])
    assert o['pck'][1] == 1.0 and 0.0 < o['pck'][0] < 1.0                      # 0.1 of the frame: every entry; 0.01 = sigma: some
    json.dumps(J.jsonable(s), allow_nan=False)


def test_the_ridge_leaves_the_bias_alone():
    """(G + R) e_D = G e_D because R's last row and column are 0, and Bm for targets t + c is Bm + c G e_D: the solution moves by c e_D
    whatever the ridge.  The targets are float32, so t + c is rounded again (3e-8 per entry): the bound is 1e-6."""
    J = _J()
    pts, target, _ = _planted(3, f=100)
    mask = np.ones((100, NJ), np.uint8)
    c = 0.25
    for ridge in (0.0, 1e-6, 0.1):
        W0 = J.solve(*R.moments_add(pts, target, mask, *_zero()), ridge=ridge)
        W1 = J.solve(*R.moments_add(pts, (target.astype(np.float64) + c).astype(np.float32), mask, *_zero()), ridge=ridge)
        assert np.abs((W1 - W0)[:, :-1]).max() <= 1e-6 and np.abs((W1 - W0)[:, -1] - c).max() <= 1e-6, ridge
    shrunk, free = J.solve(*R.moments_add(pts, target, mask, *_zero()), ridge=10.0), J.solve(*R.moments_add(pts, target, mask, *_zero()), ridge=0.0)
    assert np.abs(shrunk[:, :-1]).sum() < 0.5 * np.abs(free[:, :-1]).sum()  # the ridge does act on the other rows
    with pytest.raises(ValueError):
        J.solve(*R.moments_add(pts, target, mask, *_zero()), ridge=-1.0)
    # a singular system without a ridge: NaN, no exception
    G, Bm, n = _zero()
    n[:] = 5
    assert np.isnan(J.solve(G, Bm, n, ridge=0.0)).all()
    assert 'judgement' in J.solve.__doc__


# ------------------------------------------------------------------------------------------------ summarise / jsonable
def test_summarise_means_are_over_valid_entries_only():
    J = _J()
    alphas = [0.1, 0.2]
    # two joints; video a (train): joint 0 has 4 valid entries of error sum 2.0, joint 1 none; video b (test): 2 and 6 valid entries
    a = J.video_record('train', 1, 10, [2.0, 0.0], [4, 0], [4, 0], [[1, 2], [0, 0]])
    b = J.video_record('test', 2, 5, [1.0, 3.0], [2, 6], [1, 6], [[1, 1], [3, 6]])
    s = J.summarise([a, b], 2, alphas, 128, protocol={'ridge': 1e-6})
    assert list(s['subsets']) == ['train', 'test'] and s['alphas'] == alphas and s['protocol'] == {'ridge': 1e-6} and s['note'] == J.NOTE
    tr, te, al = s['subsets']['train'], s['subsets']['test'], s['overall']
    assert tr['err'] == 0.5 and tr['valid_entries'] == 4 and tr['entries'] == 20 and tr['valid_fraction'] == 0.2 and tr['pck'] == [0.25, 0.5]
    assert tr['per_joint']['err'][0] == 0.5 and math.isnan(tr['per_joint']['err'][1]) and math.isnan(tr['per_joint']['pck'][1][0])
    assert te['err'] == 0.5 and te['pck'] == [4 / 7.0, 1.0] and te['pck_entries'] == 7 and te['per_joint']['pck'][0] == [1.0, 1.0]
    assert al['err'] == 6.0 / 12 and al['videos'] == 2 and al['frames'] == 15 and al['err_px'] == 0.5 * 63.5
    js = J.jsonable(s)
    assert js['subsets']['train']['per_joint']['err'][1] is None and js['subsets']['train']['per_joint']['pck'][1] == [None, None]
    json.dumps(js, allow_nan=False)
    # a joint without a regressor: its figures are NaN and the overall means leave it out
    u = J.summarise([b], 2, alphas, 128, solved=[True, False])['overall']
    assert u['err'] == 0.5 and u['pck'] == [1.0, 1.0] and u['scored_joints'] == 1 and math.isnan(u['per_joint']['err'][1])
    assert u['valid_entries'] == 8 and u['scored_entries'] == 2 and u['pck_entries'] == 7 and u['scored_pck_entries'] == 1
    assert al['scored_entries'] == al['valid_entries'] == 12 and al['scored_pck_entries'] == al['pck_entries'] == 11
    arr = J.per_video_arrays([a, b])
    assert arr['subset'].tolist() == ['train', 'test'] and arr['idx'].tolist() == [1, 2] and arr['err'].tolist() == [0.5, 0.5]
    assert arr['count'].tolist() == [4, 8] and arr['pck_count'].tolist() == [4, 7] and arr['frames'].tolist() == [10, 5]
    assert math.isnan(J.summarise([], 2, alphas, 128)['overall']['err'])
    for word in ('landmark regression', "this project's", 'published'):
        assert word in J.NOTE
    for bad in ([], [0.0], [1.5], [0.1] * 9, ['x']):
        with pytest.raises(ValueError):
            J.check_alphas(bad)
    assert J.check_alphas((0.05, 1)) == [0.05, 1.0]


def test_planted_labels_are_a_function_of_the_seed():
    J = _J()
    a, b, c = J.planted_labels([0, 3], 9, 13, (128, 128)), J.planted_labels([0, 3], 9, 13, (128, 128)), J.planted_labels([0, 4], 9, 13, (128, 128))
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a['x'], c['x'])
    assert a['x'].shape == (9, 13) and a['bbox'].shape == (9, 4) and a['nframes'] == 9 and (a['bbox'][:, 2] > a['bbox'][:, 0]).all()


# ------------------------------------------------------------------------------------------------ the script and the entries
def test_parser_errors_of_the_new_flags(tmp_path, capsys):
    import make_pseudo_labels
    assert make_pseudo_labels.JOINTS_DEFAULT_RIDGE == _J().DEFAULT_RIDGE                      # the script's copies of the defaults
    assert [float(v) for v in make_pseudo_labels.JOINTS_DEFAULT_PCK.split(',')] == list(_J().DEFAULT_ALPHAS)
    base = ['--config', str(tmp_path / 'none.yaml'), '--checkpoint', str(tmp_path / 'none.npz')]
    belong = 'belong to --joints'
    for extra, text in ((['--joints-dir', 'x'], belong), (['--joints-ridge', '0.1'], belong), (['--joints-pck', '0.1'], belong),
                        (['--joints-norm', 'image'], belong), (['--joints-sheets'], belong),
                        (['--joints', '--joints-pck', '0,0.1'], 'must lie in (0, 1]'), (['--joints', '--joints-pck', '0.1,1.5'], 'must lie in (0, 1]'),
                        (['--joints', '--joints-pck', '0.1,-0.2'], 'must lie in (0, 1]'), (['--joints', '--joints-pck', '0.1,nan'], 'must lie in (0, 1]'),
                        (['--joints', '--joints-pck', ','.join(['0.1'] * 9)], 'at most 8'), (['--joints', '--joints-pck', '0.1,x'], 'comma-separated'),
                        (['--joints', '--joints-pck', ''], 'comma-separated'), (['--joints', '--joints-ridge', '-0.001'], 'must be >= 0'),
                        (['--joints', '--joints-ridge', 'nan'], 'must be >= 0'), (['--joints', '--joints-norm', 'torso'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            make_pseudo_labels.main(base + extra)
        assert e.value.code == 2, extra
        assert text in capsys.readouterr().err, extra


def test_entries_refuse_bad_arguments_without_a_device_call():
    from kpx_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION >= 19 and lib.kpx_abi_version() == _lib.ABI_VERSION
    a = 1 << 20                                                              # an aligned fake address: nothing is dereferenced

    def targets(xy=a, vis=a, bbox=a, cmap=a, f=4, j=13, target=a, mask=a, norm=a):
        return lib.kpx_joint_targets_f32(xy, vis, bbox, cmap, f, j, target, mask, norm, None)

    for bad in (dict(xy=None), dict(vis=None), dict(bbox=None), dict(cmap=None), dict(target=None), dict(mask=None), dict(norm=None), dict(f=0),
                dict(f=(1 << 20) + 1), dict(j=0), dict(j=33), dict(xy=a + 2), dict(bbox=a + 1), dict(cmap=a + 4), dict(target=a + 2), dict(norm=a + 2)):
        assert targets(**bad) == -1, bad

    def moments(pts=a, target=a, mask=a, f=4, k=15, j=13, g=a, bm=a, n=a):
        return lib.kpx_joint_moments_add_f64(pts, target, mask, f, k, j, g, bm, n, None)

    for bad in (dict(pts=None), dict(target=None), dict(mask=None), dict(g=None), dict(bm=None), dict(n=None), dict(f=0), dict(f=(1 << 20) + 1),
                dict(k=0), dict(k=65), dict(j=0), dict(j=33), dict(pts=a + 2), dict(target=a + 1), dict(g=a + 4), dict(bm=a + 4), dict(n=a + 4)):
        assert moments(**bad) == -1, bad

    def scores(pts=a, target=a, mask=a, norm=a, w=a, alpha=a, f=4, k=15, j=13, na=3, pred=a, err=a, hits=a, sum_err=a, count=a, pck=a, hit=a):
        return lib.kpx_joint_scores_f32(pts, target, mask, norm, w, alpha, f, k, j, na, pred, err, hits, sum_err, count, pck, hit, None)

    for bad in (dict(pts=None), dict(target=None), dict(mask=None), dict(norm=None), dict(w=None), dict(alpha=None), dict(pred=None), dict(err=None),
                dict(hits=None), dict(sum_err=None), dict(count=None), dict(pck=None), dict(hit=None), dict(f=0), dict(f=(1 << 20) + 1), dict(k=0),
                dict(k=65), dict(j=0), dict(j=33), dict(na=0), dict(na=9), dict(pts=a + 2), dict(norm=a + 1), dict(w=a + 4), dict(alpha=a + 4),
                dict(pred=a + 2), dict(err=a + 2), dict(sum_err=a + 4), dict(count=a + 4), dict(pck=a + 4), dict(hit=a + 4)):
        assert scores(**bad) == -1, bad


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    f, k, j = 3, 2, 4
    pts, target, mask = torch.zeros((f, k, 2)), torch.zeros((f, j, 2)), torch.zeros((f, j), dtype=torch.uint8)
    with pytest.raises(KpxError):
        ops.joint_targets(torch.zeros((f, j, 2)), mask, torch.zeros((f, 4)), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(KpxError):
        ops.joint_moments_add(pts, target, mask, torch.zeros((j, 5, 5), dtype=torch.float64), torch.zeros((j, 5, 2), dtype=torch.float64),
                              torch.zeros(j, dtype=torch.int64))
    with pytest.raises(KpxError):
        ops.joint_scores(pts, target, mask, torch.zeros(f), torch.zeros((j, 5, 2), dtype=torch.float64), torch.zeros(2, dtype=torch.float64))


def test_restatement_of_the_moments_on_a_case_known_by_hand():
    """A check of the test oracle alone (tests/joints_ref.py), which passes with or without the feature: a hand-worked anchor for the
    restatement the GPU tests hold the kernels to.  Two frames, one key point, one joint: phi = (x, y, 1).  The second frame has a NaN
    coordinate and adds nothing."""
    pts = np.array([[[0.5, -0.25]], [[np.nan, 0.0]]], np.float32)
    target = np.array([[[0.125, 2.0]], [[1.0, 1.0]]], np.float32)
    G, Bm, n = R.moments_add(pts, target, np.ones((2, 1), np.uint8), np.zeros((1, 3, 3)), np.zeros((1, 3, 2)), np.zeros(1, np.int64))
    assert np.array_equal(G[0], np.outer([0.5, -0.25, 1.0], [0.5, -0.25, 1.0])) and n.tolist() == [1]
    assert np.array_equal(Bm[0], np.outer([0.5, -0.25, 1.0], [0.125, 2.0]))
    absG, absB = R.moments_abs(pts, target, np.ones((2, 1), np.uint8))
    assert np.array_equal(absG[0], np.abs(G[0])) and np.array_equal(absB[0], np.abs(Bm[0]))
    if R.HAVE_FMA:
        G2, Bm2, _ = R.moments_add(pts, target, np.ones((2, 1), np.uint8), np.zeros((1, 3, 3)), np.zeros((1, 3, 2)), np.zeros(1, np.int64), fused=True)
        assert np.array_equal(G2, G) and np.array_equal(Bm2, Bm)           # exact products: fused or not
