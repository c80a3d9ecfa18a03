"""GPU: the landmark regression -- the three kernels of csrc/joints.hip against the numpy float64 restatement (joints_ref.py) at the smallest
shapes that can go wrong (D = 3, 31, 81: below, beside and beyond one 32 x 32 tile; F = 1, 63, 65, 130: below, beside and beyond one staged
run of 32 and 64 frames), JointRegression end to end on a planted problem, and make_pseudo_labels.py --joints on the fixture videos and on
synthetic ones."""
import json
import math
import os

import numpy as np
import pytest
import torch

import joints_ref as R
from motion_metrics_ref import within_one_ulp

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KS, JS, FS = (1, 15, 40), (1, 13), (1, 63, 65, 130)
EPS = 2.0 ** -52


def _ops():
    from kpx_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    """bit for bit, any NaN standing for any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


# ------------------------------------------------------------------------------------------------ 1. targets
def _target_case(f, j, seed):
    from kpx_amd import joints
    rs = np.random.RandomState(seed)
    cmap = joints.crop_map(320, 240)
    ax, bx, ay, by = cmap
    want = rs.uniform(-1.3, 1.3, size=(f, j, 2))                             # where the joints should land, some outside the crop
    flat = want.reshape(-1, 2)
    specials = [(1 - 1e-4, 0.0), (1 + 1e-4, 0.0), (0.0, -1 + 1e-4), (0.0, -1 - 1e-4), (-1 + 1e-4, 1 - 1e-4), (-1 - 1e-4, 0.3)]
    for i, s in enumerate(specials):                                         # just inside and just outside the crop's edge
        flat[(3 * i + 1) % len(flat)] = s
    xy = np.stack([(want[..., 0] - bx) / ax, (want[..., 1] - by) / ay], axis=-1).astype(np.float32)
    vis = (rs.uniform(size=(f, j)) < 0.8).astype(np.uint8) * rs.randint(1, 4, size=(f, j)).astype(np.uint8)   # any non-zero value is visible
    xy.reshape(-1, 2)[(len(flat) // 2) % len(flat), 0] = np.nan
    xy.reshape(-1, 2)[(len(flat) // 3) % len(flat), 1] = np.inf
    x0, y0 = rs.uniform(0, 200, size=f), rs.uniform(0, 150, size=f)
    bbox = np.stack([x0, y0, x0 + rs.uniform(5, 120, size=f), y0 + rs.uniform(5, 90, size=f)], axis=1).astype(np.float32)
    for i, bad in enumerate(((10, 10, 10, 50), (10, 10, 50, 5), (np.nan, 0, 10, 10), (0, 0, np.inf, 10), (30, 20, 29, 40))):   # degenerate boxes
        if f > 2 * i + 1:
            bbox[2 * i + 1] = bad
    return xy, vis, bbox, cmap


@pytest.mark.parametrize('f', FS)
@pytest.mark.parametrize('j', JS)
def test_targets_equal_the_restatement_bit_for_bit(j, f):
    ops = _ops()
    xy, vis, bbox, cmap = _target_case(f, j, 100 + f + j)
    want_t, want_m, want_n = R.joint_targets(xy, vis, bbox, cmap)
    fin = np.isfinite(want_t)
    assert (np.abs(np.abs(want_t[fin]) - 1.0) > 1e-6).all()                  # no target within 1e-6 of the crop's edge
    target, mask, norm = ops.joint_targets(_dev(xy), _dev(vis), _dev(bbox), _dev(cmap))
    with np.errstate(over='ignore', invalid='ignore'):
        assert _same(target.cpu().numpy(), want_t.astype(np.float32))
        assert _same(norm.cpu().numpy(), want_n.astype(np.float32))
    assert np.array_equal(mask.cpu().numpy(), want_m) and mask.dtype == torch.uint8
    if f * j >= 13:                                                          # the case does hold what it is meant to hold
        assert want_m.any() and not want_m.all() and (vis == 0).any()
    if f >= 63:
        assert np.isnan(want_n).sum() == 5 and np.isfinite(want_n).sum() == f - 5


# ------------------------------------------------------------------------------------------------ 2. moments
def _moment_case(f, k, j, seed):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-1, 1, size=(f, k, 2)).astype(np.float32)
    target = rs.uniform(-1, 1, size=(f, j, 2)).astype(np.float32)
    mask = (rs.uniform(size=(f, j)) < 0.7).astype(np.uint8)
    if j > 1:
        mask[:, 1] = 0                                                       # a joint that never counts
    if f > 2:
        pts[f // 2, k - 1, 1] = np.nan                                       # the last coordinate: a column only the last tiles stage
        mask[f // 2] = 1
    return pts, target, mask


def _start(k, j, seed):
    rs = np.random.RandomState(seed)
    d = 2 * k + 1
    g = rs.uniform(-3, 3, size=(j, d, d))
    return g + np.transpose(g, (0, 2, 1)), rs.uniform(-3, 3, size=(j, d, 2)), rs.randint(0, 1000, size=j).astype(np.int64)


def _moments(pts, target, mask, start, cuts=()):
    """the accumulators after the frames, fed in consecutive calls cut at ``cuts``"""
    ops = _ops()
    g, bm, n = (_dev(a.copy()) for a in start)
    p, t, m = _dev(pts), _dev(target), _dev(mask)
    edges = [0] + list(cuts) + [pts.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        ops.joint_moments_add(p[a:b].contiguous(), t[a:b].contiguous(), m[a:b].contiguous(), g, bm, n)
    return g.cpu().numpy(), bm.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize('f', FS)
@pytest.mark.parametrize('j', JS)
@pytest.mark.parametrize('k', KS)
def test_moments_match_the_restatement_and_do_not_depend_on_the_split(k, j, f):
    pts, target, mask = _moment_case(f, k, j, 200 + 7 * k + 3 * j + f)
    d = 2 * k + 1
    zero = (np.zeros((j, d, d)), np.zeros((j, d, 2)), np.zeros(j, np.int64))
    # from zero, against the restatement: |G - G_ref| <= F 2^-52 sum_f |use phi_a phi_b| per element, alike for Bm; n exact
    g, bm, n = _moments(pts, target, mask, zero)
    fused = R.HAVE_FMA and k <= 15 and f <= 65
    want_g, want_bm, want_n = R.moments_add(pts, target, mask, *zero, fused=fused)
    abs_g, abs_bm = R.moments_abs(pts, target, mask)
    assert np.array_equal(n, want_n) and np.isfinite(g).all() and np.isfinite(bm).all()
    print('moments K=%d J=%d F=%d: worst |G - ref| / bound %.3g, |Bm - ref| / bound %.3g'
          % (k, j, f, (np.abs(g - want_g) / np.maximum(f * EPS * abs_g, 1e-300)).max(), (np.abs(bm - want_bm) / np.maximum(f * EPS * abs_bm, 1e-300)).max()))
    assert (np.abs(g - want_g) <= f * EPS * abs_g).all() and (np.abs(bm - want_bm) <= f * EPS * abs_bm).all()
    # the key points and the targets are float32 values: their products are exact in float64, so the fused and the unfused sum round the
    # same number and the restatement gives the kernel's bits either way
    assert np.array_equal(g, want_g) and np.array_equal(bm, want_bm)
    assert np.array_equal(g, np.transpose(g, (0, 2, 1)))                     # bitwise symmetric
    if j > 1:
        assert not g[1].any() and not bm[1].any() and n[1] == 0
    # the frame with the NaN key point changes nothing: the same bits as without it
    if f > 2:
        keep = np.arange(f) != f // 2
        g2, bm2, n2 = _moments(pts[keep], target[keep], mask[keep], zero)
        assert np.array_equal(g, g2) and np.array_equal(bm, bm2) and np.array_equal(n, n2)
    # from accumulators that are not zero: one call, two calls and three calls give the same bits
    start = _start(k, j, 300 + k + j)
    one = _moments(pts, target, mask, start)
    assert np.array_equal(one[0], np.transpose(one[0], (0, 2, 1)))
    assert np.array_equal(one[2], start[2] + want_n)
    splits = [(c,) for c in (1, 64, f - 1) if 0 < c < f]
    if f > 2:
        splits.append((1, f - 1))
    if f > 65:
        splits.append((1, 64))
        splits.append((64, f - 1))
    for cuts in sorted(set(splits)):
        got = _moments(pts, target, mask, start, cuts)
        assert all(np.array_equal(a, b) for a, b in zip(one, got)), cuts


# ------------------------------------------------------------------------------------------------ 3. scores
def _score_case(f, k, j, a, seed):
    rs = np.random.RandomState(seed)
    d = 2 * k + 1
    pts = rs.uniform(-1, 1, size=(f, k, 2)).astype(np.float32)
    w = rs.uniform(-1, 1, size=(j, d, 2)) / math.sqrt(d)
    phi, _ = R.features(pts)
    target = (np.einsum('fd,jdc->fjc', phi, w) + rs.uniform(-0.12, 0.12, size=(f, j, 2))).astype(np.float32)   # errors around the thresholds
    mask = (rs.uniform(size=(f, j)) < 0.8).astype(np.uint8)
    norm = rs.uniform(0.5, 1.5, size=f).astype(np.float32)
    if j > 1:
        mask[:, j - 1] = 0                                                   # a joint without a valid frame
    if f > 2:
        norm[1] = np.nan                                                     # counted for the error, left out of PCK
        mask[1, 0] = 1
        pts[f - 1, 0, 0] = np.nan                                            # a frame that is not valid for any joint
        mask[f - 1] = 1
    alpha = np.array([0.05, 0.1, 0.2, 0.01, 0.15, 0.3, 0.5, 1.0][:a])
    return pts, target, mask, norm, w, alpha


@pytest.mark.parametrize('f', FS)
@pytest.mark.parametrize('j', JS)
@pytest.mark.parametrize('k', KS)
def test_scores_match_the_restatement(k, j, f):
    ops = _ops()
    a = 8 if (k, j) == (15, 13) else 3
    pts, target, mask, norm, w, alpha = _score_case(f, k, j, a, 400 + 5 * k + 3 * j + f)
    pred, err, hits, sum_err, count, pck_count, hit_count, valid, pck = R.joint_scores(pts, target, mask, norm, w, alpha)
    # no valid error within a relative 1e-9 of a threshold: then no hit may differ
    thr = alpha[None, None, :] * norm.astype(np.float64)[:, None, None]
    with np.errstate(invalid='ignore'):
        close = np.abs(err[..., None] - thr) <= 1e-9 * thr
    assert not (close & pck[..., None]).any()
    got = ops.joint_scores(_dev(pts), _dev(target), _dev(mask), _dev(norm), _dev(w), _dev(alpha))
    g_pred, g_err, g_hits, g_sum, g_count, g_pck, g_hit = (t.cpu().numpy() for t in got)
    assert within_one_ulp(g_pred, pred) and within_one_ulp(g_err, err)
    assert np.array_equal(g_hits, hits) and g_hits.dtype == np.uint8
    assert np.array_equal(g_count, count) and np.array_equal(g_pck, pck_count) and np.array_equal(g_hit, hit_count) and g_hit.shape == (j, a)
    bound = f * EPS * np.where(valid, err, 0.0).sum(axis=0)
    print('scores K=%d J=%d F=%d: worst |sum_err - ref| / bound %.3g' % (k, j, f, (np.abs(g_sum - sum_err) / np.maximum(bound, 1e-300)).max()))
    assert (np.abs(g_sum - sum_err) <= bound).all()
    if j > 1:
        assert g_count[j - 1] == 0 and g_sum[j - 1] == 0.0 and not g_hits[:, j - 1].any()      # the caller's mean is 0 / 0 = NaN
    if f > 2:
        assert not valid[f - 1].any() and np.isnan(g_pred[f - 1]).all() and not g_hits[f - 1].any()
        assert valid[1, 0] and not pck[1, 0] and g_hits[1, 0] == 0 and g_count[0] == g_pck[0] + (valid[:, 0] & ~pck[:, 0]).sum()
    if f >= 63:
        assert hit_count[:, 0].sum() > 0 and (hit_count[:, 0] < pck_count).any()               # the thresholds do cut through the errors


def test_ops_refuse_bad_arguments_before_any_launch():
    from kpx_amd._lib import KpxError
    ops = _ops()
    f, k, j = 4, 2, 3
    d = 2 * k + 1
    pts, target, mask = torch.zeros((f, k, 2), device=DEV), torch.zeros((f, j, 2), device=DEV), torch.zeros((f, j), dtype=torch.uint8, device=DEV)
    g, bm, n = (torch.zeros(s, dtype=t, device=DEV) for s, t in (((j, d, d), torch.float64), ((j, d, 2), torch.float64), ((j,), torch.int64)))
    norm, w = torch.ones(f, device=DEV), torch.zeros((j, d, 2), dtype=torch.float64, device=DEV)
    alpha = torch.tensor([0.1], dtype=torch.float64, device=DEV)
    ops.joint_moments_add(pts, target, mask, g, bm, n)
    ops.joint_scores(pts, target, mask, norm, w, alpha)
    for bad in (lambda: ops.joint_moments_add(pts, target, mask, g[:, :4, :4].contiguous(), bm, n),
                lambda: ops.joint_moments_add(pts, target, mask, g.float(), bm, n),
                lambda: ops.joint_moments_add(pts, target, mask, g, bm, n.int()),
                lambda: ops.joint_moments_add(pts, target[:3], mask, g, bm, n),
                lambda: ops.joint_moments_add(pts.transpose(0, 1), target, mask, g, bm, n),
                lambda: ops.joint_moments_add(torch.zeros((f, 65, 2), device=DEV), target, mask, torch.zeros((j, 131, 131), dtype=torch.float64, device=DEV),
                                              torch.zeros((j, 131, 2), dtype=torch.float64, device=DEV), n),
                lambda: ops.joint_scores(pts, target, mask, norm, w, torch.zeros(9, dtype=torch.float64, device=DEV)),
                lambda: ops.joint_scores(pts, target, mask, norm, w, alpha.float()),
                lambda: ops.joint_scores(pts, target, mask, norm[:3], w, alpha),
                lambda: ops.joint_scores(pts, target, mask.bool(), norm, w, alpha),
                lambda: ops.joint_targets(target, mask, torch.zeros((f, 3), device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)),
                lambda: ops.joint_targets(torch.zeros((f, 33, 2), device=DEV), torch.zeros((f, 33), dtype=torch.uint8, device=DEV),
                                          torch.zeros((f, 4), device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV))):
        with pytest.raises(KpxError):
            bad()


# ------------------------------------------------------------------------------------------------ 4. JointRegression
def _planted_videos(k=15, j=13, sigma=0.02, size=(320, 240)):
    """6 videos of 40 .. 70 frames, train and test in turn: the joints are a planted linear map of the points plus noise, written as pixel
    annotations of a 320 x 240 frame."""
    from kpx_amd import joints
    rs = np.random.RandomState(7)
    d = 2 * k + 1
    a = rs.uniform(-0.5, 0.5, size=(j, d, 2)) / math.sqrt(d)
    ax, bx, ay, by = joints.crop_map(*size)
    videos = []
    for v, f in enumerate((40, 70, 55, 64, 47, 65)):
        pts = rs.uniform(-0.9, 0.9, size=(f, k, 2)).astype(np.float32)
        phi, _ = R.features(pts)
        t = np.einsum('fd,jdc->fjc', phi, a) + sigma * rs.standard_normal((f, j, 2))
        x0, y0 = rs.uniform(0, 100, size=f), rs.uniform(0, 80, size=f)
        labels = {'x': (t[..., 0] - bx) / ax, 'y': (t[..., 1] - by) / ay, 'visibility': rs.uniform(size=(f, j)) < 0.9,
                  'bbox': np.stack([x0, y0, x0 + rs.uniform(60, 200, size=f), y0 + rs.uniform(60, 150, size=f)], axis=1), 'nframes': f}
        labels['visibility'][:, 4] = v % 2 == 1                                # joint 4 is never annotated in the train videos
        videos.append(('test' if v % 2 else 'train', 10 + v, pts, labels))
    return videos, size


def test_joint_regression_end_to_end_equals_the_restatement():
    """The summary against joints_ref.py.  The targets are bit-equal to the restatement's and the moments too (products of float32 values are
    exact in float64), so G, Bm and n are the restatement's bits and the one host ``solve`` gives the same W, bit for bit.  Only the device's
    float64 square root may then differ from numpy's, so counts and PCK are exact (no error of the restatement lies within a relative 1e-6
    of a threshold, asserted) and every mean is held to the bound of the per-call sums: sum_v F_v 2^-52 sum |err|_v over the entries it
    averages, divided by their number.
    What the class guarantees about order: W is a function of the train videos in the order they were added, bit for bit, whatever comes
    in between -- not that another order of the train videos gives the same bits."""
    from kpx_amd import joints
    videos, size = _planted_videos()
    k, j, alphas, ridge = 15, 13, [0.02, 0.05, 0.1], 1e-6
    reg = joints.JointRegression(k, j, alphas=alphas, ridge=ridge, device=DEV)
    for subset, idx, pts, labels in videos:
        reg.add(subset, idx, _dev(pts), labels, size)
    out = reg.finish()
    # the restatement of the same run
    cmap = joints.crop_map(*size)
    d = 2 * k + 1
    acc = (np.zeros((j, d, d)), np.zeros((j, d, 2)), np.zeros(j, np.int64))
    kept = []
    for subset, idx, pts, labels in videos:
        xy = np.stack([labels['x'], labels['y']], axis=-1).astype(np.float32)
        t, m, nrm = R.joint_targets(xy, labels['visibility'].astype(np.uint8), labels['bbox'].astype(np.float32), cmap)
        t, nrm = t.astype(np.float32), nrm.astype(np.float32)
        if subset == 'train':
            acc = R.moments_add(pts, t, m, *acc)
        kept.append((subset, idx, pts, t, m, nrm))
    assert np.array_equal(out['n'], acc[2]) and out['n'][4] == 0 and out['n'].max() <= 142
    assert np.array_equal(out['G'], acc[0]) and np.array_equal(out['Bm'], acc[1]) and np.array_equal(out['G'], np.transpose(out['G'], (0, 2, 1)))
    W = joints.solve(*acc, ridge=ridge)
    assert np.isnan(W[4]).all() and np.isfinite(np.delete(W, 4, 0)).all() and _same(out['W'], W)
    solved = np.isfinite(W).all(axis=(1, 2))
    records, slack = [], {'train': np.zeros(j), 'test': np.zeros(j)}         # per subset and joint: sum_v F_v 2^-52 sum_f |err|
    for subset, idx, pts, t, m, nrm in kept:
        _, err, _, sum_err, count, pck_count, hit_count, valid, pck = R.joint_scores(pts, t, m, nrm, W, alphas)
        thr = np.array(alphas)[None, None, :] * nrm.astype(np.float64)[:, None, None]
        with np.errstate(invalid='ignore'):
            assert not ((np.abs(err[..., None] - thr) <= 1e-6 * thr) & pck[..., None]).any()
        records.append(joints.video_record(subset, idx, pts.shape[0], sum_err, count, pck_count, hit_count))
        slack[subset] += pts.shape[0] * EPS * np.where(valid & solved[None, :], err, 0.0).sum(axis=0)
    want = joints.summarise(records, j, alphas, 128, solved=solved)
    got = out['summary']
    assert list(got['subsets']) == ['train', 'test'] and got['protocol']['norm'] == 'bbox' and got['protocol']['train_frames_per_joint'] == acc[2].tolist()
    for name in ('train', 'test'):
        g, w = got['subsets'][name], want['subsets'][name]
        for key in ('videos', 'frames', 'entries', 'valid_entries', 'pck_entries', 'valid_fraction', 'scored_joints', 'scored_entries', 'scored_pck_entries', 'pck'):
            assert g[key] == w[key], (name, key)
        assert g['per_joint']['count'] == w['per_joint']['count'] and g['per_joint']['pck_count'] == w['per_joint']['pck_count']
        assert np.array_equal(np.array(g['per_joint']['pck']), np.array(w['per_joint']['pck']), equal_nan=True)
        count = np.array(w['per_joint']['count'], np.float64)
        bound = slack[name].sum() / count[solved].sum()
        print('regression %s: |err - ref| / bound %.3g' % (name, abs(g['err'] - w['err']) / bound))
        assert abs(g['err'] - w['err']) <= bound and abs(g['err_px'] - w['err_px']) <= bound * 63.5
        for jj in range(j):
            if solved[jj]:
                assert abs(g['per_joint']['err'][jj] - w['per_joint']['err'][jj]) <= slack[name][jj] / count[jj], (name, jj)
                assert abs(g['per_joint']['err_px'][jj] - w['per_joint']['err_px'][jj]) <= slack[name][jj] / count[jj] * 63.5, (name, jj)
        assert math.isnan(g['per_joint']['err'][4]) and math.isnan(w['per_joint']['err'][4]) and g['scored_joints'] == j - 1
    # the planted map is found: the test error is at the noise's Rayleigh mean (sigma sqrt(pi / 2) = 0.0251), PCK@0.1 of boxes of 0.5 .. 1.7 is 1
    te = got['subsets']['test']
    assert 0.9 * 0.02 * math.sqrt(math.pi / 2) < te['err'] < 1.5 * 0.02 * math.sqrt(math.pi / 2) and te['pck'][2] > 0.9
    # the same train videos in the same order, the test videos first: the same W, bit for bit
    reg2 = joints.JointRegression(k, j, alphas=alphas, ridge=ridge, device=DEV)
    for subset, idx, pts, labels in [v for v in videos if v[0] == 'test'] + [v for v in videos if v[0] == 'train']:
        reg2.add(subset, idx, _dev(pts), labels, size)
    out2 = reg2.finish()
    assert np.array_equal(out2['G'], out['G']) and np.array_equal(out2['Bm'], out['Bm']) and _same(out2['W'], out['W'])
    assert joints.jsonable(out2['summary']['subsets']) == joints.jsonable(got['subsets'])
    # norm = 'image': the side of the crop, 2, for every frame
    reg3 = joints.JointRegression(k, j, alphas=alphas, norm='image', device=DEV)
    reg3.add('train', 1, _dev(videos[0][2]), videos[0][3], size)
    assert bool((reg3.kept[0]['norm'] == 2.0).all())
    with pytest.raises(ValueError):
        reg3.add('train', 2, _dev(videos[0][2][:5]), videos[0][3], size)     # 5 frames of points, 40 of labels
    with pytest.raises(ValueError):
        joints.JointRegression(k, j, norm='torso', device=DEV)


# ------------------------------------------------------------------------------------------------ 5. the script
def _strict_json(text):
    def refuse(name):
        raise ValueError('not standard JSON: %s' % name)
    return json.loads(text, parse_constant=refuse)


def test_make_pseudo_labels_joints_end_to_end(tmp_path, capsys):
    """The labels are the same bytes with and without --joints, on the fixture videos (label files written here: .mat, one .npz, one missing)
    and on synthetic ones; the report, the arrays and the sheets are there and the JSON is standard."""
    import yaml
    import kpx_amd
    from PIL import Image
    from scipy.io import savemat
    from kpx_amd import joints
    from test_data_gpu import _fixture_dataset
    from sheet_ref import unit8
    import make_pseudo_labels
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k = int(golden['n_points'])
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': int(golden['n_action']), 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    del fm
    base = ['--config', str(cfg_path), '--checkpoint', ckpt]
    labels = data / 'pseudo_labels'
    out_dir = tmp_path / 'results' / 'joints'

    def label_bytes():
        return {name: (labels / name).read_bytes() for name in sorted(os.listdir(str(labels)))}

    # no label file at all: an error before the first video (the fixture ships pseudo labels: they are not rewritten)
    before = {name: (os.stat(str(labels / name)).st_mtime_ns, (labels / name).read_bytes()) for name in sorted(os.listdir(str(labels)))}
    with pytest.raises(Exception, match='no label file'):
        make_pseudo_labels.main(base + ['--joints'])
    assert {name: (os.stat(str(labels / name)).st_mtime_ns, (labels / name).read_bytes()) for name in sorted(os.listdir(str(labels)))} == before
    make_pseudo_labels.main(base)
    plain = label_bytes()
    assert plain and (not out_dir.exists() or not os.listdir(str(out_dir)))
    # Penn's fields for every video but the last; the first as .npz
    loader = kpx_amd.data.KeypointDataLoader(str(data), 'train')
    ids, lens = [int(v) for v in golden['kp_idx']], [int(n) for n in golden['kp_len']]
    assert loader.video_ids() == ids and len(ids) >= 2
    (data / 'labels').mkdir()
    rs = np.random.RandomState(11)
    for pos, (vid, n) in enumerate(zip(ids[:-1], lens[:-1])):
        w, h = loader.frame_size(pos)
        x, y = rs.uniform(0.3 * w, 0.7 * w, size=(n, 13)), rs.uniform(0.2 * h, 0.8 * h, size=(n, 13))
        fields = {'x': x, 'y': y, 'visibility': (rs.uniform(size=(n, 13)) < 0.9).astype(np.uint8), 'nframes': np.array([[n]]),
                  'bbox': np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], axis=1)}
        if pos == 0:
            np.savez(str(data / 'labels' / ('%04d.npz' % vid)), **fields)
        else:
            savemat(str(data / 'labels' / ('%04d.mat' % vid)), fields)
    capsys.readouterr()
    make_pseudo_labels.main(base + ['--joints', '--joints-sheets', '--joints-pck', '0.1,0.5', '--colors_seed', '1'])
    assert label_bytes() == plain                                            # the same bytes, and nothing else in there
    assert 'joints (landmark regression' in capsys.readouterr().out
    assert sorted(os.listdir(str(out_dir))) == ['joints.json', 'joints.npz', 'sheets']
    rep = _strict_json((out_dir / 'joints.json').read_text())
    scored = ids[:-1]
    assert rep['missing'] == [ids[-1]] and rep['synthetic'] is False and rep['note'] == joints.NOTE and rep['alphas'] == [0.1, 0.5]
    assert list(rep['subsets']) == ['train', 'test'] and rep['overall']['videos'] == 2 * len(scored)
    assert rep['protocol'] == {'n_points': k, 'n_joints': 13, 'norm': 'bbox', 'ridge': 1e-6, 'train_frames_per_joint': rep['protocol']['train_frames_per_joint']}
    tr, te = rep['subsets']['train'], rep['subsets']['test']
    assert tr['frames'] == sum(lens[:-1]) and 0 < tr['valid_entries'] <= tr['entries'] and tr['err'] > 0 and 0 <= tr['pck'][0] <= tr['pck'][1] <= 1
    assert tr['err'] == te['err'] and tr['pck'] == te['pck']                 # the fixture lists the same videos in both subsets
    npz = np.load(str(out_dir / 'joints.npz'))
    d = 2 * k + 1
    assert npz['W'].shape == (13, d, 2) and npz['G'].shape == (13, d, d) and npz['Bm'].shape == (13, d, 2) and npz['n'].shape == (13,)
    assert int(npz['K']) == k and int(npz['J']) == 13 and npz['alphas'].tolist() == [0.1, 0.5] and str(npz['norm']) == 'bbox' and float(npz['ridge']) == 1e-6
    assert npz['subset'].tolist() == ['train'] * len(scored) + ['test'] * len(scored) and npz['idx'].tolist() == scored * 2
    assert np.array_equal(npz['G'], np.transpose(npz['G'], (0, 2, 1))) and npz['n'].tolist() == rep['protocol']['train_frames_per_joint']
    assert np.isfinite(npz['W']).all() and npz['frames'].tolist() == lens[:-1] * 2 and (npz['count'] <= npz['frames'] * 13).all()
    # W is the solution of the normal equations in the file
    assert np.allclose(npz['W'], joints.solve(npz['G'], npz['Bm'], npz['n'], 1e-6), rtol=0, atol=1e-12)
    assert sorted(os.listdir(str(out_dir / 'sheets'))) == sorted('%04d.png' % v for v in scored)
    for pos, v in enumerate(loader.videos(DEV)):
        if int(v['idx']) in scored:
            sheet = np.asarray(Image.open(str(out_dir / 'sheets' / ('%04d.png' % int(v['idx'])))))
            assert sheet.shape == (128, 3 * 128, 3) and sheet.dtype == np.uint8
            assert np.array_equal(sheet[:, :128], unit8(v['image'][0].cpu().numpy()))
            assert sheet[:, 128:256].any() and sheet[:, 256:].any()           # both point maps are drawn
    # a label file that disagrees with its video is an error that names both counts
    bad = joints.read_labels(str(data / 'labels' / ('%04d.npz' % ids[0])))
    np.savez(str(data / 'labels' / ('%04d.npz' % ids[0])), x=bad['x'][:-1], y=bad['y'][:-1], visibility=bad['visibility'][:-1], bbox=bad['bbox'][:-1],
             nframes=bad['nframes'] - 1)
    with pytest.raises(ValueError, match='the video has %d' % lens[0]):
        make_pseudo_labels.main(base + ['--joints'])
    # the synthetic form: planted annotations, even videos train and odd videos test
    for name in os.listdir(str(labels)):
        os.remove(str(labels / name))
    syn = base + ['--synthetic', '2', '--frames', '64']
    make_pseudo_labels.main(syn)
    plain = label_bytes()
    assert sorted(plain) == ['0000.npy', '0001.npy']
    make_pseudo_labels.main(syn + ['--joints', '--joints-sheets', '--joints-norm', 'image'])
    assert label_bytes() == plain
    rep = _strict_json((out_dir / 'joints.json').read_text())
    assert rep['synthetic'] is True and rep['missing'] == [] and list(rep['subsets']) == ['train', 'test'] and rep['protocol']['norm'] == 'image'
    assert rep['alphas'] == [0.05, 0.1, 0.2] and rep['overall']['videos'] == 2 and rep['subsets']['test']['videos'] == 1
    npz = np.load(str(out_dir / 'joints.npz'))
    assert npz['subset'].tolist() == ['train', 'test'] and npz['idx'].tolist() == [0, 1] and str(npz['norm']) == 'image'
    assert {'0000.png', '0001.png'} <= set(os.listdir(str(out_dir / 'sheets')))
