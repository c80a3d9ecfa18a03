"""CPU: make_pseudo_labels.py --stability without a GPU -- the draw of the maps (determinism, inverse o forward, pixel units), the numpy
restatement of the warp (stability_ref.py) on maps whose answer is the input's own bits, summarise_stability on planted arrays (ratio 0
and exactly 1, an empty frame), the parser errors of the new flags and the argument checks of the two entries of csrc/stability.hip."""
import math

import numpy as np
import pytest

import stability_ref as R


def _lib():
    from kpx_amd import stability
    return stability


def _apply(m, p):
    return np.stack([(m[..., 0] * p[..., 0] + m[..., 1] * p[..., 1]) + m[..., 2], (m[..., 3] * p[..., 0] + m[..., 4] * p[..., 1]) + m[..., 5]], axis=-1)


# ------------------------------------------------------------------------------------------------ the draw
def test_draw_is_deterministic_per_seed_and_inside_its_bounds():
    S = _lib()
    a, b, c = S.draw_warps(5, 3, seed=7), S.draw_warps(5, 3, seed=7), S.draw_warps(5, 3, seed=8)
    assert all(x.dtype == np.float64 and x.shape == (5, 3, 6) for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[1], c[1])
    assert np.array_equal(S.draw_warps(4, 2, seed=[3, 1, 17])[1], S.draw_warps(4, 2, seed=[3, 1, 17])[1])      # the script's per-video seeds
    assert not np.array_equal(S.draw_warps(4, 2, seed=[3, 1, 17])[1], S.draw_warps(4, 2, seed=[3, 0, 17])[1])
    fwd = S.draw_warps(400, 2, seed=1)[1]
    scale, angle = np.hypot(fwd[..., 0], fwd[..., 3]), np.degrees(np.arctan2(fwd[..., 3], fwd[..., 0]))
    assert scale.min() >= 1 / 1.2 - 1e-12 and scale.max() <= 1.2 + 1e-12 and scale.min() < 0.9 and scale.max() > 1.1
    assert np.abs(angle).max() <= 15 + 1e-9 and angle.min() < -10 and angle.max() > 10
    assert np.abs(fwd[..., [2, 5]]).max() <= 0.1 and np.abs(fwd[..., [2, 5]]).max() > 0.08
    assert np.array_equal(fwd[..., 0], fwd[..., 4]) and np.array_equal(fwd[..., 1], -fwd[..., 3])             # a similarity: no flip, no shear
    assert (S.DEFAULT_ROT_DEG, S.DEFAULT_LOG_SCALE, S.DEFAULT_SHIFT, S.DEFAULT_WARPS) == (15.0, math.log(1.2), 0.1, 2)
    assert S.draw_warps(0, 2, seed=1)[0].shape == (0, 2, 6)
    with pytest.raises(ValueError):
        S.draw_warps(3, 0)


def test_inverse_after_forward_is_the_identity_and_pixel_units_send_corners_home():
    S = _lib()
    res = 128
    coef, fwd = S.draw_warps(50, 2, seed=3, rot_deg=170.0, log_scale=math.log(2.0), shift=0.5, res=res)
    rs = np.random.RandomState(0)
    p = rs.uniform(-1, 1, size=(50, 2, 2))
    inv = S.invert_maps(fwd)
    assert np.abs(_apply(inv, _apply(fwd, p)) - p).max() <= 1e-12              # float64 algebra on values of order 1
    assert np.abs(_apply(fwd, _apply(inv, p)) - p).max() <= 1e-12
    # pixel units: the output pixel that shows the (normalised) point fwd(p) reads the source at p's pixel.  Corners: p = (+-1, +-1) <-> pixels
    # (0 or res - 1); the tolerance is the 1e-12 above times the (res - 1) / 2 pixels per unit
    h = (res - 1) / 2.0
    for cx in (-1.0, 1.0):
        for cy in (-1.0, 1.0):
            corner = np.broadcast_to(np.array([cx, cy]), (50, 2, 2))
            out_px = (_apply(fwd, corner) + 1.0) * h
            src_px = _apply(coef, out_px)
            assert np.abs(src_px - (corner + 1.0) * h).max() <= 1e-12 * h * 4
    # the identity and a pure shift convert exactly
    eye = np.array([1.0, 0, 0, 0, 1.0, 0])
    assert np.array_equal(S.to_pixel_units(S.invert_maps(eye), 16), eye)
    shift = S.to_pixel_units(S.invert_maps(np.array([1.0, 0, 4 / 15.0 * 2, 0, 1.0, 0])), 16)                # 4 pixels of a 16-pixel frame to the right
    assert np.abs(shift - np.array([1.0, 0, -4.0, 0, 1.0, 0])).max() <= 1e-14
    with pytest.raises(ValueError):
        S.to_pixel_units(eye, 1)


# ------------------------------------------------------------------------------------------------ the restatement, exact cases
def _frames(n, h, w, c, seed=0):
    return np.random.RandomState(seed).uniform(-1, 1, size=(n, h, w, c)).astype(np.float32)


@pytest.mark.parametrize('name', sorted(R.EXACT))
@pytest.mark.parametrize('c', (1, 3))
def test_restatement_reproduces_input_bits_on_pixel_to_pixel_maps(name, c):
    f = _frames(3, 16, 16, c, seed=5)
    rows = [2, 0, 0, 1]
    got = R.affine_warp(f, rows, np.tile(np.array(R.EXACT[name], np.float64), (4, 1)))
    want = R.exact_case(name, f)[rows]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_restatement_edges_and_degenerate_sizes():
    f = _frames(1, 4, 5, 3, seed=6)
    far = R.affine_warp(f, [0], np.array([[1.0, 0, 1e6, 0, 1.0, -1e6]]))                # the whole frame outside: every tap clamped
    assert np.array_equal(far[0], np.broadcast_to(f[0, 0, 4], (4, 5, 3)))
    one = _frames(2, 1, 1, 3, seed=7)
    assert np.array_equal(R.affine_warp(one, [1, 0], np.array([[0.3, 0.2, 5.0, 1.0, 2.0, -3.0]] * 2)), one[[1, 0]])
    half = R.affine_warp(np.array([[[[0.0], [1.0]]]], np.float32), [0], np.array([[1.0, 0, 0.25, 0, 1.0, 0]]))   # [1,1,2,1] read at x + 0.25
    assert np.array_equal(half[0, 0, :, 0], np.array([0.25, 1.0], np.float32))


def test_scores_restatement_on_planted_points():
    pts = np.array([[[0.5, -0.25], [1.0, 1.0], [np.nan, 0.0]]], np.float32)
    fwd = np.array([[1.0, 0, 0, 0, 1.0, 0], [1.0, 0, 0.5, 0, 1.0, 0]])
    pts_w = np.array([[[0.5, -0.25], [1.0, 1.0], [0.0, 0.0]], [[1.0, 0.15], [0.0, 0.0], [0.0, 0.0]]], np.float32)
    scores, valid, mean, n = R.equivariance_scores(pts, pts_w, [0, 0], fwd)
    assert valid.tolist() == [[1, 1, 0], [1, 0, 0]] and n.tolist() == [2, 1]            # on the bound: valid; past it or NaN: not
    assert scores[0, :2].tolist() == [[0.0, 0.0], [0.0, 0.0]] and mean[0].tolist() == [0.0, 0.0]
    d = np.float64(np.float32(0.15)) - np.float64(-0.25)
    e = np.sqrt(d * d)
    assert scores[1, 0].tolist() == [e, 0.5] and mean[1].tolist() == [e, 0.5]
    none = R.equivariance_scores(pts, pts_w[:1], [0], np.array([[1.0, 0, 3.0, 0, 1.0, 0]]))
    assert none[1].sum() == 0 and none[3].tolist() == [0] and np.isnan(none[2]).all()


# ------------------------------------------------------------------------------------------------ the summary
def _records(pts, pts_w, fwd, subset='train', idx=0):
    """pts [T,K,2], pts_w [T,W,K,2], fwd [T,W,6] -> the record of one video from the restatement's scores"""
    S = _lib()
    t, w, k = pts_w.shape[:3]
    rows = np.repeat(np.arange(t), w)
    scores, valid, mean, n = R.equivariance_scores(pts, pts_w.reshape(t * w, k, 2), rows, fwd.reshape(t * w, 6))
    return S.video_record(subset, idx, scores.astype(np.float32).reshape(t, w, k, 2), valid.reshape(t, w, k),
                          mean.astype(np.float32).reshape(t, w, 2), n.reshape(t, w))


def test_summary_ratio_is_zero_for_followed_and_exactly_one_for_ignored_maps():
    S = _lib()
    rs = np.random.RandomState(2)
    t, w, k, res = 6, 2, 5, 128
    pts = rs.uniform(-0.6, 0.6, size=(t, k, 2)).astype(np.float32)
    _, fwd = S.draw_warps(t, w, seed=4, res=res)
    rows = np.repeat(np.arange(t), w)
    target = R.targets(pts, rows, fwd.reshape(t * w, 6)).astype(np.float32).reshape(t, w, k, 2)
    draw = {'warps': w, 'seed': 4, 'rot_deg': S.DEFAULT_ROT_DEG, 'log_scale': S.DEFAULT_LOG_SCALE, 'shift': S.DEFAULT_SHIFT}
    # the detector follows the map up to the float32 rounding of its output: err is that rounding, ratio ~ 1e-7; with float64-exact
    # targets (planted through maps whose products are exact) it is 0.0
    grid = (rs.randint(-38, 39, size=(t, k, 2)) / 64.0).astype(np.float32)           # multiples of 1/64: the shifted points are float32 values
    exact_fwd = np.tile(np.array([1.0, 0, 0.25, 0, 1.0, -0.125]), (t, w, 1))
    exact_target = R.targets(grid, rows, exact_fwd.reshape(t * w, 6)).reshape(t, w, k, 2)
    assert np.array_equal(exact_target, exact_target.astype(np.float32))
    followed = S.summarise_stability([_records(grid, exact_target.astype(np.float32), exact_fwd)], res, draw)['overall']
    assert followed['equiv'] == 0.0 and followed['ratio'] == 0.0 and followed['equiv_px'] == 0.0 and followed['moved'] > 0.25
    assert followed['valid_fraction'] == 1.0 and followed['per_point']['equiv'] == [0.0] * k
    nearly = S.summarise_stability([_records(pts, target, fwd)], res, draw)['overall']
    assert 0.0 <= nearly['ratio'] < 1e-6
    # the detector ignores the image: pts_w == pts, so err and moved are the same expression and the ratio is exactly 1
    ignored = S.summarise_stability([_records(pts, np.repeat(pts[:, None], w, axis=1), fwd)], res, draw)
    o = ignored['overall']
    assert o['ratio'] == 1.0 and o['equiv'] == o['moved'] > 0 and o['equiv_px'] == o['equiv'] * (res - 1) / 2.0
    assert o['per_point']['equiv'] == o['per_point']['moved'] and len(o['per_point']['equiv']) == k
    assert ignored['draw'] == draw and ignored['res'] == res and "own quantity" in ignored['note'] and list(ignored['subsets']) == ['train']
    assert ignored['subsets']['train'] == o


def test_summary_skips_an_empty_frame_and_splits_subsets():
    S = _lib()
    rs = np.random.RandomState(3)
    t, w, k, res = 4, 2, 3, 64
    pts = rs.uniform(-0.5, 0.5, size=(t, k, 2)).astype(np.float32)
    pts_w = rs.uniform(-0.5, 0.5, size=(t, w, k, 2)).astype(np.float32)
    _, fwd = S.draw_warps(t, w, seed=9, res=res)
    draw = {'warps': w, 'seed': 9}
    full = _records(pts, pts_w, fwd)
    assert full['n_valid'].min() == k
    # a fifth frame whose maps throw every point out of the frame: its means are NaN, its counts 0, and nothing else moves
    pts5 = np.concatenate([pts, pts[:1]])
    pts_w5 = np.concatenate([pts_w, pts_w[:1]])
    fwd5 = np.concatenate([fwd, np.tile(np.array([1.0, 0, 5.0, 0, 1.0, 0]), (1, w, 1))])
    more = _records(pts5, pts_w5, fwd5)
    assert np.isnan(more['frame_mean'][4]).all() and not more['n_valid'][4].any() and np.array_equal(more['frame_mean'][:4], full['frame_mean'])
    a, b = S.summarise_stability([full], res, draw)['overall'], S.summarise_stability([more], res, draw)['overall']
    for key in ('equiv', 'equiv_px', 'moved', 'ratio', 'per_point', 'valid_entries'):
        assert a[key] == b[key], key
    assert a['valid_fraction'] == 1.0 and b['valid_fraction'] == 4 / 5 and b['entries'] == 5 * w * k
    # a video with nothing valid: NaN for the video, null in the JSON, and the other subset's figures unchanged
    empty = _records(pts5[4:], pts_w5[4:], fwd5[4:], subset='test', idx=7)
    both = S.summarise_stability([full, empty], res, draw)
    assert list(both['subsets']) == ['train', 'test'] and both['subsets']['train'] == a
    assert math.isnan(both['subsets']['test']['equiv']) and math.isnan(both['subsets']['test']['ratio']) and both['subsets']['test']['valid_fraction'] == 0.0
    assert both['overall']['equiv'] == a['equiv'] and both['overall']['videos'] == 2
    assert S.jsonable(both)['subsets']['test']['equiv'] is None
    arr = S.per_video_arrays([full, empty])
    assert arr['subset'].tolist() == ['train', 'test'] and arr['idx'].tolist() == [0, 7] and arr['n_valid'].tolist() == [t * w * k, 0]
    assert arr['err'][0] == a['equiv'] and np.isnan(arr['err'][1]) and arr['n_total'].tolist() == [t * w * k, w * k]
    assert math.isnan(S.summarise_stability([], res, draw)['overall']['equiv'])


# ------------------------------------------------------------------------------------------------ the script and the entries
def test_parser_errors_of_the_new_flags(tmp_path, capsys):
    import make_pseudo_labels
    base = ['--config', str(tmp_path / 'none.yaml'), '--checkpoint', str(tmp_path / 'none.npz')]
    for extra, text in ((['--stability-warps', '2'], 'belong to --stability'), (['--stability-seed', '3'], 'belong to --stability'),
                        (['--stability-sheets'], 'belong to --stability'), (['--stability', '--stability-warps', '0'], 'must be >= 1'),
                        (['--stability', '--stability-warps', '-2'], 'must be >= 1'),
                        (['--stability', '--stability-sheets', '--stability-warps', '65'], 'at most 64')):
        with pytest.raises(SystemExit) as e:
            make_pseudo_labels.main(base + extra)
        assert e.value.code == 2, extra
        assert text in capsys.readouterr().err, extra


def test_entries_refuse_bad_arguments_without_a_device_call():
    from kpx_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION >= 18 and lib.kpx_abi_version() == _lib.ABI_VERSION
    a = 1 << 20                                                              # an aligned fake address: nothing is dereferenced

    def warp(inp=a, n=2, h=8, w=8, c=3, rows=a, coef=a, r=4, out=a):
        return lib.kpx_affine_warp_f32(inp, n, h, w, c, rows, coef, r, out, None)

    for bad in (dict(inp=None), dict(rows=None), dict(coef=None), dict(out=None), dict(n=0), dict(h=0), dict(h=1025), dict(w=0), dict(w=1025),
                dict(c=2), dict(c=4), dict(r=0), dict(r=65537), dict(inp=a + 2), dict(out=a + 1), dict(rows=a + 2), dict(coef=a + 4)):
        assert warp(**bad) == -1, bad

    def scores(pts=a, pts_w=a, rows=a, fwd=a, r=4, k=5, out=a, valid=a, mean=a, n=a):
        return lib.kpx_equivariance_scores_f32(pts, pts_w, rows, fwd, r, k, out, valid, mean, n, None)

    for bad in (dict(pts=None), dict(pts_w=None), dict(rows=None), dict(fwd=None), dict(out=None), dict(valid=None), dict(mean=None), dict(n=None),
                dict(r=0), dict(r=(1 << 20) + 1), dict(k=0), dict(k=1025), dict(pts=a + 2), dict(fwd=a + 4), dict(mean=a + 1), dict(n=a + 2)):
        assert scores(**bad) == -1, bad


def test_ops_refuse_cpu_tensors():
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    rows, maps = torch.zeros(2, dtype=torch.int32), torch.zeros((2, 6), dtype=torch.float64)
    with pytest.raises(KpxError):
        ops.affine_warp(torch.zeros((1, 4, 4, 3)), rows, maps)
    with pytest.raises(KpxError):
        ops.equivariance_scores(torch.zeros((1, 3, 2)), torch.zeros((2, 3, 2)), rows, maps)
