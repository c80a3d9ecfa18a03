"""GPU: the driven rollout -- kpx_points_retarget_f32 against the float64 restatement (drive_ref.py) in every mode, on both load / store
paths, with special values, batch invariance, graph replay and argument errors; FinalModel.run(drive=...) against the model's own rollout,
against a restatement composed from the oracle's functions, and through capture, replay and a change of parameters; then
evaluate.py --drive end to end on the fixture videos."""
import json
import os

import numpy as np
import pytest
import torch

import drive_ref as D
import metrics_ref
import motion_metrics_ref as M
import sheet_ref
from oracle import restatement as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHEET_FRAMES = [3, 7, 11, 15, 19, 23, 27, 31]
#        hold                  absolute                    relative                     relative, scaled
MODES = [('hold', False), ('absolute', False), ('relative', False), ('relative', True)]
SHAPES = [(1, 1, 1), (2, 3, 1), (3, 5, 7), (2, 32, 15), (2, 32, 40), (5, 4, 65), (1, 2, 1024)]


def _ops():
    from kpx_amd import ops
    return ops


def _dev_at(a, off):
    """a on the device, contiguous, its first element ``off`` elements past a 16-byte boundary"""
    buf = torch.empty(a.size + 16, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    assert t.is_contiguous() and t.data_ptr() % 16 == (off * 4) % 16
    return t


def _inputs(b, t, k, seed=0):
    rs = np.random.RandomState(seed)
    return (rs.uniform(-1, 1, (b, k, 2)).astype(np.float32), rs.uniform(-1, 1, (b, k, 2)).astype(np.float32),
            rs.uniform(-1, 1, (b, t, k, 2)).astype(np.float32))


def _run(src, first, seq, mode, scaled, shift, off=0, out=None):
    """ops.points_retarget on host arrays -> host array"""
    ops = _ops()
    t = seq.shape[1]
    if mode == 'hold':
        got = ops.points_retarget(_dev_at(src, off), 'hold', frames=t, out=out)
    else:
        got = ops.points_retarget(_dev_at(src, off), mode, _dev_at(first, off), _dev_at(seq, off), shift=shift, scaled=scaled, out=out)
    return got.cpu().numpy()


def _want(src, first, seq, mode, scaled, shift):
    if mode == 'hold':
        return D.retarget(src, 'hold', frames=seq.shape[1])
    return D.retarget(src, mode, first, seq, shift=shift, scaled=scaled)


def _same(got, want, mode, what):
    if mode == 'relative':
        assert M.within_one_ulp(got, want.astype(np.float64)), what
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize('mode,scaled', MODES, ids=['hold', 'absolute', 'relative', 'relative_scaled'])
def test_kernel_matches_the_float64_restatement(shape, mode, scaled):
    b, t, k = shape
    src, first, seq = _inputs(b, t, k, seed=b * 1000 + t * 10 + k)
    for shift in sorted({0, 1 % b, b - 1}):
        got = _run(src, first, seq, mode, scaled, shift)
        assert got.shape == (b, t, k, 2) and got.dtype == np.float32
        _same(got, _want(src, first, seq, mode, scaled, shift), mode, (shape, mode, scaled, shift))
    if mode == 'relative' and k > 1:
        assert not np.array_equal(_want(src, first, seq, mode, True, 0), _want(src, first, seq, mode, False, 0))      # the scale is not 1


@pytest.mark.parametrize('mode,scaled', MODES, ids=['hold', 'absolute', 'relative', 'relative_scaled'])
def test_bases_four_bytes_past_a_16_byte_boundary_and_guards_around_out(mode, scaled):
    """K = 40 is even: aligned bases take the 16-byte path, these the 4-byte path, and nothing is written outside out"""
    b, t, k = 2, 32, 40
    src, first, seq = _inputs(b, t, k, seed=3)
    n = b * t * k * 2
    for off in (1, 0):
        guard = torch.full((n + 32,), 12345.0, dtype=torch.float32, device=DEV)
        out = guard[16 + off:16 + off + n].view(b, t, k, 2)
        assert out.data_ptr() % 16 == 4 * off
        got = _run(src, first, seq, mode, scaled, 1, off=off, out=out)
        _same(got, _want(src, first, seq, mode, scaled, 1), mode, (mode, scaled, off))
        g = guard.cpu().numpy()
        assert (g[:16 + off] == 12345.0).all() and (g[16 + off + n:] == 12345.0).all()
        assert np.array_equal(g[16 + off:16 + off + n].reshape(got.shape), got)


def test_coinciding_points_scale_by_one():
    b, t, k = 2, 4, 7
    src, first, seq = _inputs(b, t, k, seed=4)
    flat_first = first.copy()
    flat_first[1] = first[1, :1]                                       # driver 1's frame-0 points coincide: v_drv = 0
    flat_src = src.copy()
    flat_src[0] = src[0, :1]                                           # source 0's points coincide: v_src = 0
    for s_, f_ in ((src, flat_first), (flat_src, first), (flat_src, flat_first)):
        for shift in (0, 1):
            got = _run(s_, f_, seq, 'relative', True, shift)
            assert M.within_one_ulp(got, D.retarget(s_, 'relative', f_, seq, shift=shift, scaled=True).astype(np.float64))
            assert np.isfinite(got).all()
    # where the scale is 1 the scaled result is the unscaled one: sample 0 with shift 1 reads driver 1
    assert np.array_equal(_run(src, flat_first, seq, 'relative', True, 1)[0], _run(src, flat_first, seq, 'relative', False, 1)[0])


@pytest.mark.parametrize('mode,scaled', MODES[1:], ids=['absolute', 'relative', 'relative_scaled'])
def test_non_finite_values_reach_only_the_outputs_that_read_them(mode, scaled):
    b, t, k = 3, 4, 6
    src, first, seq = _inputs(b, t, k, seed=5)
    clean = _run(src, first, seq, mode, scaled, 1)
    seq_bad, first_bad = seq.copy(), first.copy()
    seq_bad[1, 2, 3, 0] = np.nan                                       # driver 1, frame 2, point 3, x
    seq_bad[1, 0, 5, 1] = np.inf
    first_bad[1, 4, 1] = -np.inf                                       # driver 1's frame-0 point 4, y (not read by 'absolute')
    got = _run(src, first_bad, seq_bad, mode, scaled, 1)               # shift 1: sample 0 reads driver 1
    want = _want(src, first_bad, seq_bad, mode, scaled, 1)
    _same(got, want, mode, (mode, scaled))
    assert np.array_equal(got[1:], clean[1:])                          # samples 1 and 2 read drivers 2 and 0: unchanged
    assert np.isfinite(got[1:]).all()
    bad = ~np.isfinite(got[0])
    expect = np.zeros((t, k, 2), bool)
    expect[2, 3, 0] = expect[0, 5, 1] = True
    if mode == 'relative':
        expect[:, 4, 1] = True                                         # every frame subtracts the driver's frame-0 point
    assert np.array_equal(bad, expect)                                 # (scaled: the driver's spread is non-finite, so s = 1)
    base = _run(src, first, seq, mode, False, 1) if scaled else clean  # (scaled: against the clean run at s = 1, the unscaled one)
    assert np.array_equal(got[0][~expect], base[0][~expect])           # the finite outputs of sample 0 are those of the clean run


@pytest.mark.parametrize('mode,scaled', MODES, ids=['hold', 'absolute', 'relative', 'relative_scaled'])
def test_a_batch_equals_its_samples_one_by_one(mode, scaled):
    b, t, k = 3, 5, 7
    src, first, seq = _inputs(b, t, k, seed=6)
    whole = _run(src, first, seq, mode, scaled, 0)
    for i in range(b):
        one = _run(src[i:i + 1], first[i:i + 1], seq[i:i + 1], mode, scaled, 0)
        assert np.array_equal(whole[i:i + 1].view(np.uint32), one.view(np.uint32)), (mode, scaled, i)


def test_graph_replay_is_bitwise_the_eager_result():
    ops = _ops()
    b, t, k = 4, 32, 15
    src, first, seq = (_dev_at(a, 0) for a in _inputs(b, t, k, seed=7))
    outs = [torch.empty((b, t, k, 2), device=DEV) for _ in MODES]

    def enqueue():
        ops.points_retarget(src, 'hold', frames=t, out=outs[0])
        ops.points_retarget(src, 'absolute', None, seq, shift=3, out=outs[1])
        ops.points_retarget(src, 'relative', first, seq, shift=1, out=outs[2])
        ops.points_retarget(src, 'relative', first, seq, shift=2, scaled=True, out=outs[3])

    enqueue()
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for o in outs:
        o.fill_(77.0)
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o, e) and not bool((o == 77.0).all())
    assert len({e.cpu().numpy().tobytes() for e in eager}) == 4        # the scalars (mode, shift, scaled) replayed too


def test_bad_arguments_raise_kpx_error_and_launch_nothing():
    from kpx_amd import _lib
    from kpx_amd._lib import KpxError
    ops = _ops()
    b, t, k = 2, 4, 6
    src, first = torch.zeros((b, k, 2), device=DEV), torch.zeros((b, k, 2), device=DEV)
    seq = torch.zeros((b, t, k, 2), device=DEV)
    out = torch.full((b, t, k, 2), 5.0, device=DEV)
    wide = torch.zeros((b, k, 4), device=DEV)
    big = torch.zeros((1, 1, 1025, 2), device=DEV)
    r = lambda *a, **kw: ops.points_retarget(*a, out=out, **kw)
    bad = [lambda: r(src.double(), 'relative', first, seq),                               # dtype
           lambda: r(src, 'relative', first.half(), seq),
           lambda: r(src, 'relative', first, seq.to(torch.int32)),
           lambda: ops.points_retarget(src, 'relative', first, seq, out=out.double()),
           lambda: r(src.cpu(), 'relative', first, seq),                                  # device
           lambda: r(src, 'relative', first.cpu(), seq),
           lambda: r(src, 'absolute', first, seq.cpu()),
           lambda: ops.points_retarget(src, 'hold', frames=t, out=out.cpu()),
           lambda: r(wide[:, :, ::2], 'relative', first, seq),                            # contiguity
           lambda: r(src, 'relative', first, seq.transpose(0, 1).contiguous().transpose(0, 1)),
           lambda: r(src[0], 'relative', first, seq),                                     # rank
           lambda: r(src, 'relative', first, seq[0]),
           lambda: r(src, 'relative', first[:, :, 0], seq),
           lambda: r(src[:1], 'relative', first, seq),                                    # B of the three inputs
           lambda: r(src, 'relative', first[:1], seq),
           lambda: r(src, 'relative', first, seq[:1]),
           lambda: r(src[:, :5].contiguous(), 'relative', first, seq),                    # K
           lambda: r(src, 'relative', first[:, :5].contiguous(), seq),
           lambda: r(src, 'absolute', first, seq[:, :, :5].contiguous()),
           lambda: r(src, 'relative', first, torch.zeros((b, t, k, 3), device=DEV)),      # a point has two coordinates
           lambda: ops.points_retarget(big[0], 'absolute', None, big, out=torch.zeros_like(big)),       # K = 1025
           lambda: ops.points_retarget(big[0], 'hold', frames=1),
           lambda: r(src, 'relative', first, seq, shift=b),                               # shift
           lambda: r(src, 'relative', first, seq, shift=-1),
           lambda: r(src, 'relative', first, seq, shift=0.5),
           lambda: r(src, 'scaled', first, seq),                                          # mode
           lambda: r(src, 2, first, seq),
           lambda: r(src, 'absolute', first, seq, scaled=True),                           # scaled belongs to 'relative'
           lambda: r(src, 'relative', None, seq),                                         # a missing driver
           lambda: r(src, 'relative', first, None),
           lambda: r(src, 'relative'),
           lambda: r(src, 'absolute', first),
           lambda: r(src, 'hold'),                                                        # frames missing for 'hold'
           lambda: r(src, 'hold', frames=0),
           lambda: r(src, 'hold', frames=2.0),
           lambda: r(src, 'hold', first, seq, frames=t),                                  # 'hold' takes no driver
           lambda: r(src, 'relative', first, seq, frames=t),                              # frames belongs to 'hold'
           lambda: r(src, 'hold', frames=t + 1),                                          # out of another shape
           lambda: ops.points_retarget(src, 'relative', first, seq, out=out[:1])]
    launched = _lib.abi_calls[0]
    for i, fn in enumerate(bad):
        with pytest.raises(KpxError):
            fn()
            pytest.fail('case %d raised nothing' % i)
    assert _lib.abi_calls[0] == launched                               # no entry was called ...
    assert bool((out == 5.0).all())                                    # ... and nothing was written
    assert ops.points_retarget(src, 'hold', frames=t, out=out) is out and _lib.abi_calls[0] == launched + 1 and bool((out == 0.0).all())


# ---------------------------------------------------------------------------------------------------------------- FinalModel.run(drive=...)
RES, K, B, CELLS, VDIM = 32, 3, 2, (64, 64), 8
KEYS = ('pred_im_seq', 'mask', 'pred_im_crude', 'fut_pt_raw', 'first_pt')


def _toy_arrays(seed=77):
    """the parameters of test_final_model_rollout_matches_oracle: randomised inference statistics, affine parameters and biases"""
    arrays = {**R.init_variables(K, res=RES, seed=seed), **R.init_stage2_decoder(K, cell_info=CELLS, vae_dim=VDIM, seed=seed + 1)}
    rs = np.random.RandomState(5)
    for n in list(arrays):
        if n.endswith('moving_mean') or n.endswith('/beta'):
            arrays[n] = (rs.randn(*arrays[n].shape) * 0.1).astype(np.float32)
        elif n.endswith('moving_variance') or n.endswith('/gamma'):
            arrays[n] = (rs.uniform(0.5, 1.5, arrays[n].shape)).astype(np.float32)
        elif n.endswith('/bias') or n.endswith('/biases') or n.endswith('/b'):
            arrays[n] = (rs.randn(*arrays[n].shape) * 0.05).astype(np.float32)
    return {n: a for n, a in arrays.items() if not n.startswith('img_discr')}


def _toy_model(arrays):
    import kpx_amd
    cfg = {'model': {'n_pts': K, 'cell_info': list(CELLS), 'vae_dim': VDIM, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_final'}}
    fm = kpx_amd.FinalModel(cfg, device=DEV, image_size=RES, frames_per_launch=32)
    fm.build()
    fm.store.load_numpy(arrays, strict=True)
    return fm


def _toy_feed():
    im, _ = R.synthetic_pair(B, res=RES, seed0=8, seed1=9)
    rs = np.random.RandomState(6)
    return ({'image': torch.from_numpy(im).to(DEV), 'action_code': torch.from_numpy(np.eye(9, dtype=np.float32)[[2, 7]]).to(DEV)},
            torch.from_numpy(rs.randn(B, VDIM).astype(np.float32)).to(DEV), im)


def _snap(o):
    return {k_: o[k_].cpu().numpy().copy() for k_ in KEYS}


def _equal(a, b, keys=KEYS):
    return all(np.array_equal(a[k_], b[k_]) for k_ in keys)


def test_driving_with_the_models_own_key_points_reproduces_its_rollout_bit_for_bit():
    """1: absolute, shift 0, seq = the own run's fut_pt_raw -> the own run's frames, eagerly and from the replayed graph;
    6: plain runs around driven runs are unchanged"""
    fm = _toy_model(_toy_arrays())
    feed, z, _ = _toy_feed()
    own = _snap(fm.run(None, feed, z=z))
    seq = torch.from_numpy(own['fut_pt_raw']).to(DEV).clone()
    first = torch.full((B, K, 2), float('nan'), device=DEV)            # 'absolute' does not read it
    for call in range(4):                                              # eager, capture + replay, replay, replay
        got = _snap(fm.run(None, feed, drive={'mode': 'absolute', 'first': first, 'seq': seq, 'shift': 0, 'scaled': False}))
        assert _equal(got, own), call
    assert len(fm._graphs) == 1 and not fm._graph_failed               # the driven graph; the own rollout ran once, eagerly
    for call in range(3):                                              # the own rollout: capture + replay, replay, replay
        assert _equal(_snap(fm.run(None, feed, z=z)), own), call
        got = _snap(fm.run(None, feed, drive={'mode': 'hold'}))        # a driven call of another key between them
        assert not np.array_equal(got['pred_im_seq'], own['pred_im_seq'])
    assert len(fm._graphs) == 3 and not fm._graph_failed
    assert _equal(_snap(fm.run(None, feed, z=z)), own)
    # shift 1 swaps the two samples' key points: another key, another graph, another result
    swapped = _snap(fm.run(None, feed, drive={'mode': 'absolute', 'seq': seq, 'shift': 1}))
    assert np.array_equal(swapped['fut_pt_raw'], own['fut_pt_raw'][::-1]) and not np.array_equal(swapped['pred_im_seq'], own['pred_im_seq'])


def test_driven_rollout_matches_the_restatement_with_the_points_injected():
    """2: random key points against image_encoder, pose_encoder, get_gaussian_maps and translator composed as final_model_forward does"""
    arrays = _toy_arrays()
    fm = _toy_model(arrays)
    feed, _, im_np = _toy_feed()
    rs = np.random.RandomState(12)
    seq = rs.uniform(-1, 1, (B, 32, K, 2)).astype(np.float32)
    first = rs.uniform(-1, 1, (B, K, 2)).astype(np.float32)
    t = 32
    with torch.no_grad():
        net = R.Net({n: torch.from_numpy(a) for n, a in arrays.items()}, train_mode=False)
        im = torch.from_numpy(im_np)
        tiled_im = im.unsqueeze(1).expand(B, t, RES, RES, 3).reshape(B * t, RES, RES, 3)
        emb = R.image_encoder(net, im)[-2]
        emb_t = emb.unsqueeze(1).expand(B, t, *emb.shape[1:]).reshape(B * t, *emb.shape[1:])
        first_pt = R.pose_encoder(net, im, final_res=RES)
        heat = RES // 4
        cur_map = R.get_gaussian_maps(first_pt, [heat, heat])
        cur_map_t = cur_map.unsqueeze(1).expand(B, t, *cur_map.shape[1:]).reshape(B * t, *cur_map.shape[1:])

        def frames(points):
            pred_map = R.get_gaussian_maps(torch.from_numpy(points).reshape(B * t, K, 2), [heat, heat])
            crude, mask = R.translator(net, torch.cat([emb_t, cur_map_t, pred_map], dim=-1), final_res=RES)
            final = tiled_im * mask + crude * (1 - mask)
            return {'pred_im_seq': torch.clamp(final, -1, 1).reshape(B, t, RES, RES, 3).numpy(),
                    'pred_im_crude': torch.clamp(crude, -1, 1).reshape(B, t, RES, RES, 3).numpy(), 'mask': mask.reshape(B, t, RES, RES, 1).numpy()}

        first_np = first_pt.numpy()
        rel_l2 = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
        for drive, points in (({'mode': 'absolute', 'seq': seq, 'shift': 1}, D.retarget(first_np, 'absolute', first, seq, shift=1)),
                              ({'mode': 'relative', 'first': first, 'seq': seq, 'shift': 1, 'scaled': True}, None)):
            dev_drive = {k_: torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v for k_, v in drive.items()}
            for call in range(3):                                      # eager, capture + replay, replay
                got = _snap(fm.run(None, feed, drive=dev_drive))
                np.testing.assert_allclose(got['first_pt'], first_np, atol=2e-5)
                if call == 0:
                    if points is None:                                 # from the detected points the device itself used: the kernel's own bar
                        assert M.within_one_ulp(got['fut_pt_raw'], D.retarget(got['first_pt'], 'relative', first, seq, shift=1,
                                                                              scaled=True).astype(np.float64))
                        points = got['fut_pt_raw']
                    want = frames(points)
                assert np.array_equal(got['fut_pt_raw'], points), (drive['mode'], call)
                for k_ in ('pred_im_seq', 'pred_im_crude', 'mask'):
                    assert rel_l2(got[k_], want[k_]) < 1e-4, (drive['mode'], call, k_)
                assert float(np.abs(got['pred_im_seq']).max()) <= 1.0
    assert len(fm._graphs) == 2 and not fm._graph_failed


def test_hold_gives_32_identical_frames_and_no_driven_run_touches_the_rng():
    """3 and 4"""
    fm = _toy_model(_toy_arrays())
    feed, _, _ = _toy_feed()
    rs = np.random.RandomState(13)
    first = torch.from_numpy(rs.uniform(-1, 1, (B, K, 2)).astype(np.float32)).to(DEV)
    seq = torch.from_numpy(rs.uniform(-1, 1, (B, 32, K, 2)).astype(np.float32)).to(DEV)
    torch.manual_seed(1234)
    torch.randn(3, device=DEV)
    state, host_state = torch.cuda.get_rng_state(DEV).clone(), torch.get_rng_state().clone()
    for call in range(3):                                              # eager, capture + replay, replay
        got = _snap(fm.run(None, {'image': feed['image']}, drive={'mode': 'hold'}))        # no action code is needed either
        assert torch.equal(torch.cuda.get_rng_state(DEV), state) and torch.equal(torch.get_rng_state(), host_state), call
        for k_ in ('pred_im_seq', 'mask', 'pred_im_crude', 'fut_pt_raw'):
            assert all(np.array_equal(got[k_][:, i], got[k_][:, 0]) for i in range(32)), (call, k_)
        assert np.array_equal(got['fut_pt_raw'][:, 0], got['first_pt'])
        assert not np.array_equal(got['pred_im_seq'][0], got['pred_im_seq'][1])
        fm.run(None, feed, drive={'mode': 'relative', 'first': first, 'seq': seq, 'shift': 1, 'scaled': call == 1})
        assert torch.equal(torch.cuda.get_rng_state(DEV), state) and torch.equal(torch.get_rng_state(), host_state), call
    after = torch.randn(3, device=DEV)
    torch.manual_seed(1234)
    torch.randn(3, device=DEV)
    assert torch.equal(after, torch.randn(3, device=DEV))              # the next draw is the one it would have been


def test_bad_drives_are_refused_before_anything_is_copied_or_launched():
    from kpx_amd import _lib
    fm = _toy_model(_toy_arrays())
    feed, _, _ = _toy_feed()
    first, seq = torch.zeros((B, K, 2), device=DEV), torch.zeros((B, 32, K, 2), device=DEV)
    ok = {'mode': 'relative', 'first': first, 'seq': seq, 'shift': 1, 'scaled': False}
    for _ in range(2):                                                 # the second call captures: the bad ones below meet a graph
        fm.run(None, feed, drive=ok)
    torch.cuda.synchronize()
    launched = _lib.abi_calls[0]
    for bad in (dict(ok, mode='scaled'), dict(ok, shift=B), dict(ok, shift=-1), dict(ok, scaled=1), dict(ok, seq=seq[:, :31]),
                dict(ok, seq=torch.zeros((B + 1, 32, K, 2), device=DEV)), dict(ok, first=torch.zeros((B, K + 1, 2), device=DEV)),
                dict(ok, seq=seq.double()), dict(ok, seq=seq.cpu()), dict(ok, first=None), {'mode': 'relative', 'seq': seq},
                {'mode': 'hold', 'seq': seq}, {'mode': 'absolute', 'seq': seq, 'scaled': True}, dict(ok, frames=32), 'hold'):
        with pytest.raises(_lib.KpxError):
            fm.run(None, feed, drive=bad)
    assert _lib.abi_calls[0] == launched


def test_loading_new_parameters_drops_the_driven_graph():
    """5: as test_rollout_graph_is_recaptured_after_the_parameters_change, for a driven graph"""
    feed, _, _ = _toy_feed()
    rs = np.random.RandomState(14)
    drive = {'mode': 'relative', 'first': torch.from_numpy(rs.uniform(-1, 1, (B, K, 2)).astype(np.float32)).to(DEV),
             'seq': torch.from_numpy(rs.uniform(-1, 1, (B, 32, K, 2)).astype(np.float32)).to(DEV), 'shift': 1, 'scaled': True}
    want = {seed: _snap(_toy_model(_toy_arrays(seed)).run(None, feed, drive=drive)) for seed in (77, 177)}      # fresh models, eager
    assert not np.array_equal(want[77]['pred_im_seq'], want[177]['pred_im_seq'])
    fm = _toy_model(_toy_arrays(77))
    for _ in range(3):                                                 # eager, capture + replay, replay
        got = _snap(fm.run(None, feed, drive=drive))
    assert len(fm._graphs) == 1 and _equal(got, want[77])
    fm.store.load_numpy(_toy_arrays(177), strict=True)                 # second checkpoint into the same model object
    torch.empty(1 << 22, device=DEV).fill_(float('nan'))               # recycle freed blocks with poison: a stale graph would read it
    for call in range(3):
        assert _equal(_snap(fm.run(None, feed, drive=drive)), want[177]), call
    assert len(fm._graphs) == 1 and not fm._graph_failed


# ---------------------------------------------------------------------------------------------------------------- evaluate.py --drive
def _png(path, mode=None):
    from PIL import Image
    im = Image.open(path)
    assert mode is None or im.mode == mode
    return np.asarray(im, np.uint8)


def _read_seq(d, mode='RGB'):
    assert sorted(os.listdir(d)) == ['%06d.png' % i for i in range(32)]
    return np.stack([_png(os.path.join(d, '%06d.png' % i), mode) for i in range(32)])


def _check_metrics(got, want, what):
    """the bounds of tests/test_metrics_gpu.py: got, want [N,3] = (ssim, mse, psnr)"""
    got = got.astype(np.float64)
    assert np.abs(got[:, 0] - want[:, 0]).max() <= 1e-5, what
    assert (np.abs(got[:, 1] - want[:, 1]) <= 1e-6 * np.abs(want[:, 1])).all(), what
    fin = np.isfinite(want[:, 2])
    assert np.array_equal(np.isfinite(got[:, 2]), fin) and (got[~fin, 2] == want[~fin, 2]).all(), what
    assert np.abs(got[fin, 2] - want[fin, 2]).max(initial=0) <= 1e-4, what


def test_evaluate_drive_end_to_end_on_the_fixture_videos(tmp_path, monkeypatch):
    import yaml
    import kpx_amd
    import evaluate
    import make_pseudo_labels
    from test_data_gpu import _fixture_dataset
    data = tmp_path / 'penn'
    golden = _fixture_dataset(data)
    k, n_action = int(golden['n_points']), int(golden['n_action'])
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    make_pseudo_labels.main(['--config', str(cfg_path), '--checkpoint', ckpt])

    calls = []
    run = kpx_amd.FinalModel.run
    host = lambda t: None if t is None else t.detach().cpu().numpy().copy()

    def recording_run(self, sess, feed_dict, z=None, drive=None):
        out = run(self, sess, feed_dict, z=z) if drive is None else run(self, sess, feed_dict, z=z, drive=drive)
        calls.append({'drive': None if drive is None else {key: host(v) if isinstance(v, torch.Tensor) else v for key, v in drive.items()},
                      'image': host(feed_dict['image']), 'pred': host(out['pred_im_seq']), 'kp': host(out['fut_pt_raw']),
                      'first_pt': host(out['first_pt']), 'fut': host(out.get('future_points'))})
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    stage1 = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--batch', '2']
    recorded = {}
    for name, extra in (('eval', ['--checkpoint_stage2', ckpt, '--metrics', '--drive', 'transfer,labels,hold']),
                        ('only', ['--metrics', '--drive-only', '--drive', 'labels,hold', '--sheet-frames', '0,31']),
                        ('plain', ['--checkpoint_stage2', ckpt, '--metrics'])):
        del calls[:]
        torch.manual_seed(11)
        evaluate.main(stage1 + extra + ['--save_dir', str(tmp_path / name)])
        recorded[name] = list(calls)
    loader = kpx_amd.data.SequenceDataLoader(str(data), 'test', n_points=k, n_action=n_action, random_order=False, randomness=False,
                                             with_image_seq=True)
    batches = [{key: b[key].cpu().numpy() for key in ('image', 'real_im_seq', 'real_seq', 'keypoints', 'action_code')}
               for b in loader.batches(2, DEV, repeat=False, num_preprocess_threads=2)]
    assert [b['image'].shape[0] for b in batches] == [2, 1]                              # batches of 2 and 1
    res, cols = 128, 1 + len(SHEET_FRAMES)

    # ---- per batch: the own rollout, then labels, hold, transfer on the batch's labels, with shifts 0, 0 and 1 (0 for the batch of one)
    rec = recorded['eval']
    assert len(rec) == 4 * len(batches)
    ev = tmp_path / 'eval'
    samples = sorted(n for n in os.listdir(str(ev)) if n.isdigit())
    assert samples == ['0000', '0001', '0002']
    rows = ['real', 'labels', 'model', 'hold', 'driver', 'transfer']
    want_scores = {'labels': [], 'hold': []}
    s = 0
    for b, batch in enumerate(batches):
        bsz = batch['image'].shape[0]
        own, labels, hold, transfer = rec[4 * b:4 * b + 4]
        shift = 1 % bsz
        assert own['drive'] is None
        assert labels['drive']['mode'] == 'absolute' and labels['drive']['shift'] == 0 and labels['drive']['scaled'] is False
        assert hold['drive'] == {'mode': 'hold', 'shift': 0, 'scaled': False}
        assert transfer['drive']['mode'] == 'relative' and transfer['drive']['shift'] == shift and transfer['drive']['scaled'] is False
        for call in (labels, transfer):
            assert np.array_equal(call['drive']['seq'], batch['real_seq']) and np.array_equal(call['drive']['first'], batch['keypoints'])
        for call in (own, labels, hold, transfer):
            assert np.array_equal(call['image'], batch['image'])
        # what the runs were given is what they rolled out
        assert np.array_equal(labels['kp'], batch['real_seq'])
        assert np.array_equal(hold['kp'], np.repeat(hold['first_pt'][:, None], 32, axis=1))
        assert M.within_one_ulp(transfer['kp'], D.retarget(transfer['first_pt'], 'relative', batch['keypoints'], batch['real_seq'],
                                                           shift=shift).astype(np.float64))
        driver = (np.arange(bsz) + shift) % bsz
        for i in range(bsz):
            d = ev / samples[s]
            assert sorted(os.listdir(str(d))) == ['crude', 'current_points.png', 'drive.png', 'drive_hold', 'drive_labels', 'drive_transfer',
                                                  'drive_transfer_points', 'input_im.png', 'mask', 'pred_points', 'pred_seq', 'real_seq']
            # every PNG of drive_*/ is the quantised recorded tensor
            for name, call in (('labels', labels), ('hold', hold), ('transfer', transfer)):
                assert np.array_equal(_read_seq(str(d / ('drive_' + name))), metrics_ref.png8(call['pred'][i])), (samples[s], name)
            assert np.array_equal(_read_seq(str(d / 'drive_transfer_points')), sheet_ref.raw8(transfer['fut'][i])), samples[s]
            # the sheet: the restatement's paste of the recorded tensors, row by row
            want = np.zeros((1, len(rows) * res, cols * res, 3), np.uint8)
            image = batch['image'][i:i + 1, None]
            for r, (first_cell, seq) in enumerate(((image, batch['real_im_seq'][i:i + 1]), (image, labels['pred'][i:i + 1]),
                                                   (image, own['pred'][i:i + 1]), (image, hold['pred'][i:i + 1]),
                                                   (batch['image'][driver[i]][None, None], batch['real_im_seq'][driver[i]][None]),
                                                   (image, transfer['pred'][i:i + 1]))):
                sheet_ref.paste(want, first_cell, [0], r, 0, 'unit')
                sheet_ref.paste(want, seq, SHEET_FRAMES, r, 1, 'unit')
            sheet = _png(str(d / 'drive.png'), 'RGB')
            assert sheet.shape == (len(rows) * res, cols * res, 3) and np.array_equal(sheet, want[0]), samples[s]
            # ... and its real, model and labels cells are the PNGs of real_seq/, pred_seq/ and drive_labels/
            cell = lambda row, col: sheet[row * res:(row + 1) * res, col * res:(col + 1) * res]
            for row, folder in ((0, 'real_seq'), (1, 'drive_labels'), (2, 'pred_seq'), (3, 'drive_hold'), (5, 'drive_transfer')):
                assert np.array_equal(cell(row, 0), _png(str(d / 'input_im.png')))
                for j, fr in enumerate(SHEET_FRAMES):
                    assert np.array_equal(cell(row, 1 + j), _png(str(d / folder / ('%06d.png' % fr)))), (samples[s], folder, fr)
            s += 1
        real8 = metrics_ref.png8(batch['real_im_seq']).reshape(bsz * 32, res, res, 3) / 255.0
        for name, call in (('labels', labels), ('hold', hold)):
            want_scores[name].append(metrics_ref.frame_metrics(metrics_ref.png8(call['pred']).reshape(bsz * 32, res, res, 3) / 255.0, real8))
    assert json.loads((ev / 'drive.json').read_text()) == {'rows': rows, 'sheet_frames': SHEET_FRAMES, 'cell': [res, res],
                                                           'modes': ['labels', 'hold', 'transfer'], 'scaled': False, 'n_self_driven': 1}

    # ---- the scores of labels and hold against the restatement on the recorded frames
    npz = np.load(str(ev / 'metrics.npz'))
    drive_keys = ['drive_%s_%s' % (m, n) for m in ('hold', 'labels') for n in ('mse', 'psnr', 'ssim')]
    assert sorted(npz.files) == drive_keys + ['mse', 'psnr', 'ssim']
    for name in ('labels', 'hold'):
        got = np.stack([npz['drive_%s_%s' % (name, n)] for n in ('ssim', 'mse', 'psnr')], axis=-1)
        assert got.shape == (3, 32, 3) and got.dtype == np.float32
        _check_metrics(got.reshape(-1, 3), np.concatenate(want_scores[name]), name)
    summary = json.loads((ev / 'metrics.json').read_text())
    block = evaluate.summarise_drive({m: {n: npz['drive_%s_%s' % (m, n)] for n in ('ssim', 'psnr', 'mse')} for m in ('labels', 'hold')},
                                     model={n: npz[n] for n in ('ssim', 'psnr', 'mse')})
    assert summary['drive'] == json.loads(json.dumps(block, allow_nan=False))
    assert set(block['skill']) == {'ssim', 'psnr', 'mse'} and block['modes'] == ['labels', 'hold']
    assert len(block['hold']['ssim']['per_frame']) == 32 and block['hold']['ssim']['mean'] is not None

    # ---- --drive-only without a stage-2 checkpoint: driven runs alone, no model row, the drive scores alone -- and the same ones
    only = tmp_path / 'only'
    rec = recorded['only']
    assert len(rec) == 2 * len(batches) and all(c['drive'] is not None for c in rec)
    assert [c['drive']['mode'] for c in rec] == ['absolute', 'hold'] * len(batches)
    assert sorted(os.listdir(str(only))) == samples + ['drive.json', 'metrics.json', 'metrics.npz']
    assert json.loads((only / 'drive.json').read_text()) == {'rows': ['real', 'labels', 'hold'], 'sheet_frames': [0, 31], 'cell': [res, res],
                                                             'modes': ['labels', 'hold'], 'scaled': False, 'n_self_driven': 0}
    s = 0
    for b, batch in enumerate(batches):
        labels, hold = rec[2 * b:2 * b + 2]
        for i in range(batch['image'].shape[0]):
            d = only / samples[s]
            assert sorted(os.listdir(str(d))) == ['drive.png', 'drive_hold', 'drive_labels', 'input_im.png', 'real_seq']
            want = np.zeros((1, 3 * res, 3 * res, 3), np.uint8)
            for r, seq in enumerate((batch['real_im_seq'][i:i + 1], labels['pred'][i:i + 1], hold['pred'][i:i + 1])):
                sheet_ref.paste(want, batch['image'][i:i + 1, None], [0], r, 0, 'unit')
                sheet_ref.paste(want, seq, [0, 31], r, 1, 'unit')
            assert np.array_equal(_png(str(d / 'drive.png'), 'RGB'), want[0]), samples[s]
            assert np.array_equal(_read_seq(str(d / 'drive_hold')), _read_seq(str(ev / samples[s] / 'drive_hold')))     # stage 2 plays no part
            s += 1
    npz1 = np.load(str(only / 'metrics.npz'))
    assert sorted(npz1.files) == drive_keys
    for key in drive_keys:
        assert np.array_equal(npz1[key], npz[key]), key
    summary1 = json.loads((only / 'metrics.json').read_text())
    assert set(summary1) == {'drive'} and 'skill' not in summary1['drive']
    assert {m: summary1['drive'][m] for m in ('labels', 'hold')} == {m: summary['drive'][m] for m in ('labels', 'hold')}

    # ---- without --drive: the files, keys and calls of before
    plain = tmp_path / 'plain'
    assert all(c['drive'] is None for c in recorded['plain']) and len(recorded['plain']) == len(batches)
    assert sorted(os.listdir(str(plain))) == samples + ['metrics.json', 'metrics.npz']
    for name in samples:
        assert sorted(os.listdir(str(plain / name))) == ['crude', 'current_points.png', 'input_im.png', 'mask', 'pred_points', 'pred_seq', 'real_seq']
    assert sorted(np.load(str(plain / 'metrics.npz')).files) == ['mse', 'psnr', 'ssim']
    assert 'drive' not in json.loads((plain / 'metrics.json').read_text())


def test_evaluate_drive_hold_on_synthetic_inputs(tmp_path, monkeypatch):
    """--synthetic has no labels: hold alone, beside the model's own rollout and, with --drive-only, without it or a stage-2 checkpoint"""
    import yaml
    import kpx_amd
    import evaluate
    k, n_action, res = 5, 6, 128
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    calls = []
    run = kpx_amd.FinalModel.run

    def recording_run(self, sess, feed_dict, z=None, drive=None):
        out = run(self, sess, feed_dict, z=z) if drive is None else run(self, sess, feed_dict, z=z, drive=drive)
        calls.append({'drive': drive, 'image': feed_dict['image'].cpu().numpy().copy(), 'pred': out['pred_im_seq'].cpu().numpy().copy()})
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--batch', '2', '--synthetic', '3', '--drive', 'hold', '--sheet-frames', '0,31']
    for name, extra, rows in (('both', ['--checkpoint_stage2', ckpt], ['model', 'hold']), ('only', ['--drive-only'], ['hold'])):
        del calls[:]
        ev = tmp_path / name
        evaluate.main(base + extra + ['--save_dir', str(ev)])
        per_batch = len(rows)
        assert len(calls) == 2 * per_batch and sorted(os.listdir(str(ev))) == ['0000', '0001', '0002', 'drive.json']
        assert json.loads((ev / 'drive.json').read_text()) == {'rows': rows, 'sheet_frames': [0, 31], 'cell': [res, res], 'modes': ['hold'],
                                                               'scaled': False, 'n_self_driven': 0}
        s = 0
        for b in range(2):
            group = calls[per_batch * b:per_batch * (b + 1)]
            assert [c['drive'] for c in group] == [None, {'mode': 'hold', 'shift': 0, 'scaled': False}][-per_batch:]
            for i in range(group[0]['image'].shape[0]):
                want = np.zeros((1, per_batch * res, 3 * res, 3), np.uint8)
                for r, call in enumerate(group):
                    sheet_ref.paste(want, call['image'][i:i + 1, None], [0], r, 0, 'unit')
                    sheet_ref.paste(want, call['pred'][i:i + 1], [0, 31], r, 1, 'unit')
                d = ev / ('%04d' % s)
                assert np.array_equal(_png(str(d / 'drive.png'), 'RGB'), want[0]), (name, s)
                assert np.array_equal(_read_seq(str(d / 'drive_hold')), metrics_ref.png8(group[-1]['pred'][i]))
                assert sorted(os.listdir(str(d))) == (['drive.png', 'drive_hold', 'input_im.png'] if name == 'only' else
                                                      ['crude', 'current_points.png', 'drive.png', 'drive_hold', 'input_im.png', 'mask',
                                                       'pred_points', 'pred_seq'])
                s += 1
        assert s == 3
