"""GPU: the detector's equivariance score -- kpx_affine_warp_f32 against the numpy float64 restatement (stability_ref.py) bit for bit at
every shape class, alignment and store path, its exact cases, row independence, graph replay and refusals; kpx_equivariance_scores_f32
against the restatement; KeypointModel.stability against the pieces it is made of; make_pseudo_labels.py --stability end to end on the
fixture videos."""
import json
import math
import os

import numpy as np
import pytest
import torch

import stability_ref as R
from motion_metrics_ref import within_one_ulp
from sheet_ref import unit8

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHAPES = [(1, 1, 1, 3), (1, 1, 5, 1), (1, 4, 1, 3), (2, 2, 3, 3), (2, 5, 7, 1), (3, 16, 16, 3), (2, 17, 33, 3), (1, 128, 128, 3)]
GUARD = 8                                                    # floats before and after a guarded buffer
SENTINEL = 1234.5


def _ops():
    from kpx_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(shape, off, fill=None):
    """A contiguous fp32 view of ``shape`` that starts 4 * off bytes past a 16-byte boundary, inside a buffer with guard words around it
    -> (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[GUARD + off:GUARD + off + n].view(*shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off and view.is_contiguous()
    if fill is not None:
        view.copy_(torch.from_numpy(fill))
    return buf, view


def _guards_intact(buf, off, n):
    g = buf.cpu().numpy()
    return bool((g[:GUARD + off] == SENTINEL).all() and (g[GUARD + off + n:] == SENTINEL).all())


def _maps(rs, r, h, w):
    """r inverse maps in pixel units about the frame centre: any angle (beyond a quarter turn), scales 0.5 .. 2, shifts of up to half a
    frame; row 0 sends the whole frame outside (every tap clamped), row 1 is the identity."""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    th, s = rs.uniform(-math.pi, math.pi, size=r), np.exp(rs.uniform(math.log(0.5), math.log(2.0), size=r))
    a, b = s * np.cos(th), s * np.sin(th)
    tx, ty = rs.uniform(-0.5, 0.5, size=r) * w, rs.uniform(-0.5, 0.5, size=r) * h
    coef = np.stack([a, -b, cx - a * cx + b * cy + tx, b, a, cy - b * cx - a * cy + ty], axis=1)
    coef[0, 2] += 4.0 * (w + h) * 2.0
    coef[0, 5] -= 4.0 * (w + h) * 2.0
    if r > 1:
        coef[1] = [1.0, 0, 0, 0, 1.0, 0]
    return coef


# ------------------------------------------------------------------------------------------------ 1. the warp
@pytest.mark.parametrize('offs', ((0, 0), (1, 1), (1, 0)), ids=('aligned', 'both+4', 'in+4'))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_warp_equals_the_restatement_bit_for_bit(shape, offs):
    ops = _ops()
    n, h, w, c = shape
    rs = np.random.RandomState(1000 * h + 10 * w + c)
    frames = rs.uniform(-1, 1, size=shape).astype(np.float32)
    r = 7
    rows = rs.randint(0, n, size=r).astype(np.int32)                         # any order, repeats
    rows[-1] = n - 1
    coef = _maps(rs, r, h, w)
    want = R.affine_warp(frames, rows, coef)
    assert np.array_equal(_bits(want[0]), _bits(np.broadcast_to(frames[rows[0], 0, w - 1], (h, w, c))))      # the row that left the frame
    assert np.array_equal(_bits(want[1]), _bits(frames[rows[1]]))
    _, fin = _guarded(shape, offs[0], frames)
    obuf, out = _guarded((r, h, w, c), offs[1])
    got = ops.affine_warp(fin, _dev(rows), _dev(coef), out=out)
    torch.cuda.synchronize()
    assert got is out and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert _guards_intact(obuf, offs[1], want.size)
    fresh = ops.affine_warp(fin, _dev(rows), _dev(coef))                     # an output of the op's own
    assert fresh.dtype == torch.float32 and tuple(fresh.shape) == (r, h, w, c) and torch.equal(fresh, out)


@pytest.mark.parametrize('c', (1, 3))
@pytest.mark.parametrize('name', sorted(R.EXACT))
def test_pixel_to_pixel_maps_copy_input_bits(name, c):
    ops = _ops()
    f = np.random.RandomState(5).uniform(-1, 1, size=(3, 16, 16, c)).astype(np.float32)
    rows = np.array([2, 0, 0, 1], np.int32)
    for off in (0, 1):                                                       # the 16-byte and the 4-byte store path
        _, out = _guarded((4, 16, 16, c), off)
        ops.affine_warp(_dev(f), _dev(rows), _dev(np.tile(np.array(R.EXACT[name], np.float64), (4, 1))), out=out)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(R.exact_case(name, f)[rows])), (name, off)


def test_a_row_does_not_depend_on_the_rest_of_the_table():
    ops = _ops()
    rs = np.random.RandomState(11)
    frames = _dev(rs.uniform(-1, 1, size=(3, 17, 33, 3)).astype(np.float32))
    rows, coef = rs.randint(0, 3, size=9).astype(np.int32), _maps(rs, 9, 17, 33)
    whole = ops.affine_warp(frames, _dev(rows), _dev(coef))
    for r in (0, 4, 8):
        alone = ops.affine_warp(frames, _dev(rows[r:r + 1]), _dev(coef[r:r + 1]))
        assert torch.equal(alone[0], whole[r]), r
    back = ops.affine_warp(frames, _dev(rows[::-1].copy()), _dev(coef[::-1].copy()))
    assert torch.equal(back.flip(0), whole)


def test_warp_graph_replays_bitwise():
    ops = _ops()
    rs = np.random.RandomState(12)
    frames = _dev(rs.uniform(-1, 1, size=(2, 32, 32, 3)).astype(np.float32))
    rows, coef = _dev(rs.randint(0, 2, size=5).astype(np.int32)), _dev(_maps(rs, 5, 32, 32))
    out = torch.empty((5, 32, 32, 3), device=DEV)
    ops.affine_warp(frames, rows, coef, out=out)
    torch.cuda.synchronize()
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.affine_warp(frames, rows, coef, out=out, check_tables=False)
    out.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_ops_refuse_bad_arguments_before_any_launch():
    from kpx_amd import _lib
    from kpx_amd._lib import KpxError
    ops = _ops()
    f = torch.zeros((2, 8, 8, 3), device=DEV)
    rows, coef = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros((4, 6), dtype=torch.float64, device=DEV)
    out = torch.full((4, 8, 8, 3), 7.0, device=DEV)
    wide = torch.zeros((2, 8, 8, 6), device=DEV)
    pts, pts_w = torch.zeros((2, 5, 2), device=DEV), torch.zeros((4, 5, 2), device=DEV)
    souts = (torch.full((4, 5, 2), 7.0, device=DEV), torch.full((4, 5), 7, dtype=torch.uint8, device=DEV), torch.full((4, 2), 7.0, device=DEV),
             torch.full((4,), 7, dtype=torch.int32, device=DEV))
    nan_coef, inf_coef = coef.clone(), coef.clone()
    nan_coef[2, 3], inf_coef[0, 0] = float('nan'), float('inf')
    bad = [lambda: ops.affine_warp(f.cpu(), rows, coef, out),                                       # device
           lambda: ops.affine_warp(f, rows.cpu(), coef, out),
           lambda: ops.affine_warp(f, rows, coef.cpu(), out),
           lambda: ops.affine_warp(f, rows, coef, out.cpu()),
           lambda: ops.affine_warp(f.double(), rows, coef, out),                                    # dtype
           lambda: ops.affine_warp(f, rows.long(), coef, out),
           lambda: ops.affine_warp(f, rows, coef.float(), out),
           lambda: ops.affine_warp(f, rows, coef, out.double()),
           lambda: ops.affine_warp(wide[..., ::2], rows, coef, out),                                # contiguity
           lambda: ops.affine_warp(f, torch.zeros(8, dtype=torch.int32, device=DEV)[::2], coef, out),
           lambda: ops.affine_warp(f, rows, torch.zeros((4, 12), dtype=torch.float64, device=DEV)[:, ::2], out),
           lambda: ops.affine_warp(f, rows, coef, torch.zeros((4, 8, 8, 6), device=DEV)[..., ::2]),
           lambda: ops.affine_warp(f[0], rows, coef, None),                                         # shapes and sizes
           lambda: ops.affine_warp(torch.zeros((2, 8, 8, 2), device=DEV), rows, coef, None),
           lambda: ops.affine_warp(torch.zeros((1, 1025, 1, 1), device=DEV), rows, coef, None),
           lambda: ops.affine_warp(torch.zeros((0, 8, 8, 3), device=DEV), rows, coef, None),
           lambda: ops.affine_warp(f, rows[:3], coef, None),
           lambda: ops.affine_warp(f, rows[:0], coef[:0], None),
           lambda: ops.affine_warp(f, rows, coef[:, :5].contiguous(), None),
           lambda: ops.affine_warp(f, rows, coef, out[:3]),
           lambda: ops.affine_warp(f, torch.zeros(65537, dtype=torch.int32, device=DEV), torch.zeros((65537, 6), dtype=torch.float64, device=DEV)),
           lambda: ops.affine_warp(f, rows + 2, coef, out),                                         # a frame number outside [0, N)
           lambda: ops.affine_warp(f, rows - 1, coef, out),
           lambda: ops.affine_warp(f, rows, nan_coef, out),                                         # a non-finite coefficient
           lambda: ops.affine_warp(f, rows, inf_coef, out),
           lambda: ops.equivariance_scores(pts.cpu(), pts_w, rows, coef, souts),
           lambda: ops.equivariance_scores(pts, pts_w.double(), rows, coef, souts),
           lambda: ops.equivariance_scores(pts, pts_w[:3], rows, coef, souts),
           lambda: ops.equivariance_scores(pts, torch.zeros((4, 6, 2), device=DEV), rows, coef, souts),
           lambda: ops.equivariance_scores(torch.zeros((2, 1025, 2), device=DEV), torch.zeros((4, 1025, 2), device=DEV), rows, coef, None),
           lambda: ops.equivariance_scores(pts, pts_w, rows + 2, coef, souts),
           lambda: ops.equivariance_scores(pts, pts_w, rows, nan_coef, souts),
           lambda: ops.equivariance_scores(pts, pts_w, rows, coef.float(), souts),
           lambda: ops.equivariance_scores(pts, pts_w, rows, coef, (souts[0], souts[1].int(), souts[2], souts[3])),
           lambda: ops.equivariance_scores(pts, pts_w, rows, coef, (souts[0], souts[1], souts[2], souts[3][:3])),
           lambda: ops.equivariance_scores(pts, pts_w, rows, coef, souts[:3])]
    torch.cuda.synchronize()
    launched = _lib.abi_calls[0]
    for i, fn in enumerate(bad):
        with pytest.raises(KpxError):
            fn()
            pytest.fail('case %d raised nothing' % i)
    torch.cuda.synchronize()
    assert _lib.abi_calls[0] == launched                                                        # no entry was called ...
    assert bool((out == 7).all()) and all(bool((o == 7).all()) for o in souts)                  # ... and nothing was written


# ------------------------------------------------------------------------------------------------ 2. the scores
def _score_case(rs, r, k, shift):
    """Inputs whose rows cycle through four kinds (shift picks where the cycle starts): 0 random similarity maps; 1 the identity with points
    planted exactly on and just past the bounds (the identity's products are exact); 2 a shift that leaves no valid point; 3 random maps
    with NaN and infinite points on both sides."""
    n = r // 2 + 1
    pts = rs.uniform(-0.9, 0.9, size=(n, k, 2)).astype(np.float32)
    rows = rs.randint(0, n, size=r).astype(np.int32)
    th, s = rs.uniform(-0.5, 0.5, size=r), np.exp(rs.uniform(-0.3, 0.3, size=r))
    fwd = np.stack([s * np.cos(th), -s * np.sin(th), rs.uniform(-0.3, 0.3, size=r), s * np.sin(th), s * np.cos(th), rs.uniform(-0.3, 0.3, size=r)], axis=1)
    kinds = (np.arange(r) + shift) % 4
    fwd[kinds == 1] = [1.0, 0, 0, 0, 1.0, 0]
    fwd[kinds == 2] = [1.0, 0, 5.0, 0, 1.0, 0]
    planted = []
    for row in np.nonzero(kinds == 1)[0]:                                    # a frame of its own for each identity row, with planted points
        pts = np.concatenate([pts, rs.uniform(-0.9, 0.9, size=(1, k, 2)).astype(np.float32)])
        rows[row] = pts.shape[0] - 1
        edge = [(1.0, -1.0), (-1.0, 0.5), (np.nextafter(np.float32(1), np.float32(2)), 0.0), (0.0, np.nextafter(np.float32(-1), np.float32(-2)))]
        for kk, e in enumerate(edge[:k]):
            pts[-1, kk] = e
        planted.append((row, [True, True, False, False][:k]))
    pts_w = (R.targets(pts, rows, fwd) + rs.normal(0, 0.02, size=(r, k, 2))).astype(np.float32)
    for row in np.nonzero(kinds == 3)[0]:
        pts_w[row, rs.randint(0, k)] = [np.nan, 0.0]
        pts_w[row, rs.randint(0, k)] = [0.1, np.inf]
    if (kinds == 3).any():                                                   # and a frame with a NaN and an infinite point of its own
        pts = np.concatenate([pts, rs.uniform(-0.9, 0.9, size=(1, k, 2)).astype(np.float32)])
        pts[-1, 0] = [0.0, np.nan]
        pts[-1, k - 1] = [-np.inf, 0.0]
        rows[np.nonzero(kinds == 3)[0][0]] = pts.shape[0] - 1
    # no target within 2^-40 of a bound unless it sits exactly on it: a last-bit difference cannot flip `valid`
    t = R.targets(pts, rows, fwd)
    with np.errstate(invalid='ignore'):
        near = (np.abs(np.abs(t) - 1.0) < 2.0 ** -40) & (np.abs(t) != 1.0)
    assert not near.any()
    return pts, pts_w, rows, fwd, planted


@pytest.mark.parametrize('r', (1, 3, 130))
@pytest.mark.parametrize('k', (1, 15, 40, 65, 1024))
def test_scores_match_the_restatement(k, r):
    ops = _ops()
    rs = np.random.RandomState(100 * k + r)
    seen = {'empty row': False, 'nan': False, 'planted': False}
    for shift in range(4 if r < 4 else 1):
        pts, pts_w, rows, fwd, planted = _score_case(rs, r, k, shift)
        w_scores, w_valid, w_mean, w_n = R.equivariance_scores(pts, pts_w, rows, fwd)
        for row, flags in planted:
            assert w_valid[row, :len(flags)].tolist() == [int(v) for v in flags]
        seen = {'empty row': seen['empty row'] or bool((w_n == 0).any()), 'nan': seen['nan'] or bool(np.isnan(w_scores).any()),
                'planted': seen['planted'] or bool(planted)}
        scores, valid, mean, n_valid = ops.equivariance_scores(_dev(pts), _dev(pts_w), _dev(rows), _dev(fwd))
        assert (scores.dtype, valid.dtype, mean.dtype, n_valid.dtype) == (torch.float32, torch.uint8, torch.float32, torch.int32)
        assert (tuple(scores.shape), tuple(valid.shape), tuple(mean.shape), tuple(n_valid.shape)) == ((r, k, 2), (r, k), (r, 2), (r,))
        assert np.array_equal(valid.cpu().numpy(), w_valid) and np.array_equal(n_valid.cpu().numpy(), w_n), shift
        assert within_one_ulp(scores.cpu().numpy(), w_scores), shift
        assert within_one_ulp(mean.cpu().numpy(), w_mean), shift
        empty = w_n == 0
        assert np.isnan(mean.cpu().numpy()[empty]).all() and np.isfinite(mean.cpu().numpy()[~empty]).all()
    assert all(seen.values()), seen                                          # every kind of row was among the cases
    # into given outputs, and replayed from a graph
    outs = (torch.empty((r, k, 2), device=DEV), torch.empty((r, k), dtype=torch.uint8, device=DEV), torch.empty((r, 2), device=DEV),
            torch.empty(r, dtype=torch.int32, device=DEV))
    args = (_dev(pts), _dev(pts_w), _dev(rows), _dev(fwd))
    got = ops.equivariance_scores(*args, out=outs)
    assert all(g is o for g, o in zip(got, outs)) and torch.equal(outs[1], valid) and torch.equal(outs[0].view(torch.int32), scores.view(torch.int32))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.equivariance_scores(*args, out=outs, check_tables=False)
    for o in outs:
        o.fill_(9)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), scores.view(torch.int32)) and torch.equal(outs[1], valid) and torch.equal(outs[3], n_valid)
    assert torch.equal(outs[2].view(torch.int32), mean.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. the model
RES, K = 32, 5


@pytest.fixture(scope='module')
def small_model():
    import kpx_amd
    cfg = {'model': {'n_pts': K}, 'paths': {'log_dir': '/tmp/kpx_stability'}}
    model = kpx_amd.KeypointModel(cfg, device=DEV, image_size=RES, frames_per_launch=4)
    model.build(None)
    return model


def test_stability_with_identity_maps_returns_the_points_themselves(small_model):
    """One map per frame: the warped slabs then hold the frames of the original slabs (6 frames in slabs of 4 and 2), so the detector sees
    the same batches -- it is not promised to give a frame the same bits in another batch."""
    t = 6
    frames = _dev(np.random.RandomState(20).uniform(-1, 1, size=(t, RES, RES, 3)).astype(np.float32))
    eye = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0]), (t, 1, 1))
    pts = small_model.run(None, {'image': frames[None]})['pts'][0]
    for given in (None, pts):
        out = small_model.stability(frames, eye, eye, pts=given)
        assert tuple(out['pts_w'].shape) == (t, 1, K, 2) and torch.equal(out['pts_w'][:, 0].view(torch.int32), pts.view(torch.int32))
        assert torch.equal(out['pts'].view(torch.int32), pts.contiguous().view(torch.int32))
        assert not out['scores'].cpu().numpy().any() and not out['frame_mean'].cpu().numpy().any()             # err and moved exactly 0
        assert bool((out['valid'] == 1).all()) and bool((out['n_valid'] == K).all())


def test_stability_with_drawn_maps_is_warp_then_run_then_scores(small_model):
    from kpx_amd import stability as S
    ops = _ops()
    t, w = 5, 2                                                              # 10 warped frames in slabs of 4, 4 and 2
    frames = _dev(np.random.RandomState(21).uniform(-1, 1, size=(t, RES, RES, 3)).astype(np.float32))
    coef, fwd = S.draw_warps(t, w, seed=6, res=RES)
    out = small_model.stability(frames, coef, fwd)
    rows = np.repeat(np.arange(t), w).astype(np.int32)
    warped = ops.affine_warp(frames, _dev(rows), _dev(coef.reshape(t * w, 6)))
    assert np.array_equal(_bits(warped.cpu().numpy()), _bits(R.affine_warp(frames.cpu().numpy(), rows, coef.reshape(t * w, 6))))
    pts_w = small_model.run(None, {'image': warped[None]})['pts'][0]
    assert torch.equal(out['pts_w'].reshape(t * w, K, 2).view(torch.int32), pts_w.contiguous().view(torch.int32))
    pts = small_model.run(None, {'image': frames[None]})['pts'][0]
    assert torch.equal(out['pts'].view(torch.int32), pts.contiguous().view(torch.int32))
    w_scores, w_valid, w_mean, w_n = R.equivariance_scores(pts.cpu().numpy(), pts_w.cpu().numpy(), rows, fwd.reshape(t * w, 6))
    assert within_one_ulp(out['scores'].cpu().numpy().reshape(t * w, K, 2), w_scores)
    assert np.array_equal(out['valid'].cpu().numpy().reshape(t * w, K), w_valid) and np.array_equal(out['n_valid'].cpu().numpy().reshape(-1), w_n)
    assert within_one_ulp(out['frame_mean'].cpu().numpy().reshape(t * w, 2), w_mean)
    with pytest.raises(ValueError):
        small_model.stability(frames, coef[:4], fwd[:4])


# ------------------------------------------------------------------------------------------------ 4. the script
def _close(a, b, rel):
    """a == b up to the relative difference ``rel``; None (JSON's null) and NaN stand for each other"""
    if isinstance(a, dict):
        return set(a) == set(b) and all(_close(a[k], b[k], rel) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_close(x, y, rel) for x, y in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        a, b = (float('nan') if v is None else float(v) for v in (a, b))
        return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rel * abs(b)
    return a == b


def test_make_pseudo_labels_stability_end_to_end(tmp_path):
    """The labels are the same bytes with and without --stability; the report equals summarise_stability over the restatement's scores of
    the recorded points.  The kernel's err, moved and per-frame means are within one float32 ulp (2^-23 relative) of the restatement's, all
    are >= 0, so every mean of them is within 2^-23 relative and their ratio within 2^-22: the bound below is 2^-21."""
    import yaml
    import kpx_amd
    from kpx_amd import stability as S
    from PIL import Image
    from test_data_gpu import _fixture_dataset
    import make_pseudo_labels
    ops = _ops()
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
    make_pseudo_labels.main(base)
    plain = {name: (labels / name).read_bytes() for name in sorted(os.listdir(str(labels)))}
    assert plain and not (tmp_path / 'results' / 'stability').exists()
    w, seed, res = 2, 3, 128
    make_pseudo_labels.main(base + ['--stability', '--stability-warps', str(w), '--stability-seed', str(seed), '--stability-sheets', '--colors_seed', '1'])
    assert {name: (labels / name).read_bytes() for name in sorted(os.listdir(str(labels)))} == plain              # nothing else in there either
    out_dir = tmp_path / 'results' / 'stability'
    assert sorted(os.listdir(str(out_dir))) == ['sheets', 'stability.json', 'stability.npz']
    # the report, from the recorded points: the detector again on the warp, then the restatement
    model = kpx_amd.KeypointModel(cfg, device=DEV)
    model.build(None)
    model.restore(None, ckpt)
    records, first = [], {}
    for s_no, subset in enumerate(('train', 'test')):
        for v in kpx_amd.data.KeypointDataLoader(str(data), subset).videos(DEV):
            n, idx = int(v['len']), int(v['idx'])
            pts = np.load(str(labels / ('%04d.npy' % idx)))
            coef, fwd = S.draw_warps(n, w, seed=[seed, s_no, idx], res=res)
            rows = np.repeat(np.arange(n), w).astype(np.int32)
            frames = v['image'][:n].contiguous()
            warped = ops.affine_warp(frames, _dev(rows), _dev(coef.reshape(n * w, 6)))
            pts_w = model.run(None, {'image': warped[None]})['pts'][0].cpu().numpy()
            scores, valid, mean, nv = R.equivariance_scores(pts, pts_w, rows, fwd.reshape(n * w, 6))
            records.append(S.video_record(subset, idx, scores.astype(np.float32).reshape(n, w, k, 2), valid.reshape(n, w, k),
                                          mean.astype(np.float32).reshape(n, w, 2), nv.reshape(n, w)))
            first[idx] = (frames[0].cpu().numpy(), R.affine_warp(frames[:1].cpu().numpy(), np.zeros(w, np.int32), coef[0]))
    draw = {'warps': w, 'seed': seed, 'rot_deg': S.DEFAULT_ROT_DEG, 'log_scale': S.DEFAULT_LOG_SCALE, 'shift': S.DEFAULT_SHIFT}
    want = S.jsonable(S.summarise_stability(records, res, draw))
    got = json.loads((out_dir / 'stability.json').read_text())
    assert got['draw'] == want['draw'] and got['note'] == want['note'] and 'own quantity' in got['note'] and list(got['subsets']) == ['train', 'test']
    assert _close(got, want, 2.0 ** -21), (got['overall'], want['overall'])
    assert got['overall']['valid_entries'] > 0 and got['overall']['equiv'] > 0 and got['overall']['ratio'] > 0
    npz, arr = np.load(str(out_dir / 'stability.npz')), S.per_video_arrays(records)
    assert sorted(npz.files) == sorted(arr)
    for key in ('subset', 'idx', 'n_valid', 'n_total'):
        assert np.array_equal(npz[key], arr[key]), key
    for key in ('err', 'moved'):
        assert np.allclose(npz[key], arr[key], rtol=2.0 ** -21, atol=0, equal_nan=True), key
    # the sheets: one per video; per map a row of frame | warped frame | two point maps; the first two cells are the 'unit' bytes
    assert sorted(os.listdir(str(out_dir / 'sheets'))) == sorted('%04d.png' % idx for idx in first)
    for idx, (frame, warped) in first.items():
        sheet = np.asarray(Image.open(str(out_dir / 'sheets' / ('%04d.png' % idx))))
        assert sheet.shape == (w * res, 4 * res, 3) and sheet.dtype == np.uint8
        for j in range(w):
            assert np.array_equal(sheet[j * res:(j + 1) * res, :res], unit8(frame)), (idx, j)
            assert np.array_equal(sheet[j * res:(j + 1) * res, res:2 * res], unit8(warped[j])), (idx, j)
            assert sheet[j * res:(j + 1) * res, 2 * res:].any()                                   # the point maps are drawn
    # the synthetic form
    make_pseudo_labels.main(base + ['--synthetic', '1', '--frames', '8', '--stability'])
    got = json.loads((out_dir / 'stability.json').read_text())
    assert list(got['subsets']) == ['synthetic'] and got['overall']['videos'] == 1 and got['draw']['warps'] == 2 and got['draw']['seed'] == 0
    assert np.load(str(out_dir / 'stability.npz'))['subset'].tolist() == ['synthetic']
