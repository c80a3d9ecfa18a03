"""tests/streaming_ref.py checked on the CPU: the fp32 restatements against oracle.restatement.resize2x (bit for bit) and torch autograd
(resize backward, max_pool2d(ceil_mode=True), the feature-gradient composition on tie-free data), the bf16 rounding against
torch.Tensor.bfloat16(), the fp32 evaluation of the three bounded operations inside its bound under both contractions, and every planted slip
rejected by the assertion tests/test_streaming_gpu.py uses, on the cases it uses."""
import numpy as np
import pytest
import torch

import streaming_ref as R
from oracle import f64_loops, restatement

F32, F64 = np.float32, np.float64
RESIZE_SHAPES = [s['shape'] for s in R.RESIZE_F32.values()]


def _close(a, b, tol):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), 1.0)))


# ----------------------------------------------------------------------------------------------- bf16 rounding
def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(3)
    x = np.concatenate([R.HALFWAY, (rng.standard_normal(4096) * 10 ** rng.uniform(-20, 20, 4096)).astype(F32),
                        rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(F32)])
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(x), want)
    assert np.array_equal(R.bf16_bits(R.HALFWAY), R.HALFWAY_BF16)
    assert np.isnan(R.to_bf16(np.array([np.nan], F32)))[0]
    # both parities of the kept bit are among the exact ties, and truncation differs from rounding on half of them
    ties = R.HALFWAY[(R.HALFWAY.view(np.uint32) & 0xffff) == 0x8000]
    kept = (ties.view(np.uint32) >> 16) & 1
    assert set(kept.tolist()) == {0, 1}
    assert R.differing(R.to_bf16(ties, 'bf16_trunc'), R.to_bf16(ties)) == int(kept.sum())


# ----------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize('shape', RESIZE_SHAPES + [s['shape'] for s in R.RESIZE_BF16.values()])
def test_resize_forward_is_the_oracles(shape):
    x = R.resize_input(shape)
    assert R.differing(R.resize2x_fwd(x, F32), restatement.resize2x(torch.from_numpy(x)).numpy()) == 0
    assert np.array_equal(R.resize2x_fwd(x, F64), f64_loops.resize2x(x))
    assert _close(R.resize2x_fwd(x, F32), R.resize2x_fwd(x), 4 * R.U)
    # contracted or not: fma(d, t, tl) with t in {0, 0.5} gives the bits of the separate operations
    n, h, w, c = shape
    tl, tr = x[:, :, :, :], x[:, :, np.minimum(np.arange(w) + 1, w - 1)]
    for t in (F32(0), F32(0.5)):
        assert R.differing(R.fma32(tr - tl, t, tl), tl + (tr - tl) * t) == 0


@pytest.mark.parametrize('shape', RESIZE_SHAPES)
def test_resize_backward_is_torch_autograd(shape):
    dy = R.resize_gradient(shape)
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    (restatement.resize2x(x) * torch.from_numpy(dy.astype(F64))).sum().backward()
    assert _close(R.resize2x_bwd(dy), x.grad.numpy(), 1e-14)
    assert _close(R.resize2x_bwd(dy, F32), x.grad.numpy(), 16 * R.U * 4)
    # each output pixel's weights add up to 1: the gradient of all-ones sums to the number of output elements
    assert R.resize2x_bwd(np.ones_like(dy), F32).sum(dtype=F64) == dy.size


# ----------------------------------------------------------------------------------------------- pool, feature gradient
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def _nhwc(t):
    return np.transpose(t.detach().numpy(), (0, 2, 3, 1))


@pytest.mark.parametrize('name', list(R.POOL_F32))
def test_pool_is_torch_max_pool_with_ceil_mode(name):
    shape = R.POOL_F32[name]['shape']
    for kind in ('cont', 'ties'):
        x = R.pool_inputs(shape, kind)
        want = torch.nn.functional.max_pool2d(_nchw(x), 2, 2, ceil_mode=True)
        assert R.differing(R.maxpool2_fwd(x, F32), _nhwc(want)) == 0
    x, dy = R.pool_inputs(shape, 'cont'), R.pool_gradient(shape)
    xt = _nchw(x.astype(F64)).requires_grad_(True)
    (torch.nn.functional.max_pool2d(xt, 2, 2, ceil_mode=True) * _nchw(dy.astype(F64))).sum().backward()
    assert np.array_equal(R.maxpool2_bwd(dy, x, F32), _nhwc(xt.grad).astype(F32))
    # on ties the whole gradient still arrives, at exactly one position per window
    xt = R.pool_inputs(shape, 'ties')
    dx = R.maxpool2_bwd(np.ones_like(dy), xt, F32)
    n, h, w, c = shape
    assert dx.sum() == dy.size and set(np.unique(dx).tolist()) <= {0.0, 1.0}


def test_first_maximum_in_scan_order():
    x = np.zeros((1, 2, 2, 15), F32)
    for ch, pat in enumerate(R.PATTERNS):
        x[0, :, :, ch] = np.array(pat, F32).reshape(2, 2)
    bi, best = R.first_max(x)
    assert bi[0, 0, 0].tolist() == [pat.index(True) for pat in R.PATTERNS] and np.all(best == 1)
    last, _ = R.first_max(x, 'tie_last')
    assert last[0, 0, 0].tolist() == [3 - pat[::-1].index(True) for pat in R.PATTERNS]
    assert R.max_patterns(x) == set(R.PATTERNS)


@pytest.mark.parametrize('shape', R.FEAT_F32)
@pytest.mark.parametrize('pooled', [False, True])
def test_feature_gradient_is_the_four_pass_chain_in_torch(shape, pooled):
    """d = dL/dz for y = relu(z), L = sum(dy_pooled * max_pool(y)) + g * sum |y - y_gt|, on tie-free z."""
    rng = np.random.default_rng(17)
    z = rng.standard_normal(shape)
    gt = np.maximum(rng.standard_normal(shape), 0)
    dyp = R.pooled_gradient(shape).astype(F64)
    g = R.gscale(R.GHOST, R.GDEV)
    zt = _nchw(z).requires_grad_(True)
    y = torch.relu(zt)
    loss = g * (y - _nchw(gt)).abs().sum()
    if pooled:
        loss = loss + (torch.nn.functional.max_pool2d(y, 2, 2, ceil_mode=True) * _nchw(dyp)).sum()
    loss.backward()
    d = R.vgg_feat_bwd(gt, np.maximum(z, 0), g, dyp if pooled else None)
    assert _close(d, _nhwc(zt.grad), 1e-14)
    d32 = R.vgg_feat_bwd(gt.astype(F32), np.maximum(z, 0).astype(F32), R.gscale(R.GHOST, R.GDEV, F32), dyp.astype(F32) if pooled else None, F32)
    assert d32.dtype == F32 and _close(d32, _nhwc(zt.grad), 4 * R.U)


def test_every_tie_case_holds_every_pattern_and_the_zero_cases():
    for shape in [s['shape'] for s in R.POOL_F32.values()] + R.FEAT_F32 + R.FEAT_BF16:
        gt, pred = R.features('ties', shape)
        if R.full_windows(shape) >= 16:
            assert R.max_patterns(pred) >= set(R.PATTERNS)
        assert set(np.unique(pred).tolist()) <= {0.0, 1.0, 2.0}
        if pred.size >= 64:
            assert np.any(gt == pred) and np.any(gt > pred) and np.any(gt < pred) and np.any(pred == 0)
    # the bf16 case where |l1| is below half a unit of dy_pooled: the rounded sum is dy_pooled itself
    d = R.pooled_gradient(R.FEAT_BF16[0], bf16=True)
    g = R.gscale(R.GHOST, R.GDEV, F32)
    big = np.abs(d) >= 1
    assert big.any() and np.array_equal(R.to_bf16(d[big] + g), d[big]) and not np.array_equal(R.to_bf16(d[big] + F32(R.GHOST)), d[big])


# ----------------------------------------------------------------------------------------------- the three bounded operations
@pytest.mark.parametrize('P', R.PREP_P)
def test_vgg_prep_fp32_stays_inside_its_bound_under_both_contractions(P):
    x = R.prep_values(P)
    ref, bound = R.vgg_prep_fwd(x), R.vgg_prep_fwd_bound(x)
    # (x + 1) / 2 * 255 - mean a second time, channel by channel
    for ch in range(3):
        assert np.array_equal(ref[:, ch], (x[:, 2 - ch].astype(F64) + 1) / 2 * 255 - float(R.VGG_MEAN_BGR[ch]))
    for contracted in (False, True):
        r = R.worst(R.vgg_prep_fwd(x, F32, contracted=contracted) - ref, bound)
        print('ratio vgg_prep_fwd fp32 contracted=%d %.4f' % (contracted, r))
        assert r <= 1.0
    assert np.all(bound > 0)
    # the backward is the transpose: d/dx sum(dbgr * fwd(x))
    d = R.normal('prep_d', (P, 3))
    xt = torch.tensor(x.astype(F64), requires_grad=True)
    (((xt + 1) / 2 * 255).flip(1) * torch.from_numpy(d.astype(F64))).sum().backward()
    assert np.array_equal(R.vgg_prep_bwd(d), xt.grad.numpy())
    assert _close(R.vgg_prep_bwd(d, F32), xt.grad.numpy(), R.U)


@pytest.mark.parametrize('n', R.ACT_N)
def test_tanh_backward_fp32_stays_inside_its_bound_under_both_contractions(n):
    dy, y = R.act_values(n)
    ref, bound = R.act_bwd(dy, y, R.ACT_TANH), R.tanh_bwd_bound(dy, y)
    yt = torch.tensor(np.arctanh(np.clip(y.astype(F64), -0.999, 0.999)), requires_grad=True)
    (torch.tanh(yt) * torch.from_numpy(dy.astype(F64))).sum().backward()
    inner = np.abs(y) < 0.999
    assert _close(ref[inner], yt.grad.numpy()[inner], 1e-9)
    for contracted in (False, True):
        r = R.worst(R.act_bwd(dy, y, R.ACT_TANH, F32, contracted=contracted) - ref, bound)
        print('ratio act_bwd tanh fp32 n=%d contracted=%d %.4f' % (n, contracted, r))
        assert r <= 1.0


@pytest.mark.parametrize('n', R.AXPY_N)
@pytest.mark.parametrize('a', R.AXPY_A)
def test_axpy_fp32_stays_inside_its_bound_under_both_contractions(n, a):
    y, x = R.normal('axpy_y', (n,)), R.normal('axpy_x', (n,))
    ref, bound = R.axpy(y, x, a), R.axpy_bound(y, x, a)
    assert np.array_equal(ref, y.astype(F64) + float(F32(a)) * x.astype(F64))
    for contracted in (False, True):
        r = R.worst(R.axpy(y, x, a, F32, contracted=contracted) - ref, bound)
        print('ratio axpy fp32 n=%d a=%g contracted=%d %.4f' % (n, a, contracted, r))
        assert r <= 1.0


@pytest.mark.parametrize('n', R.ACT_N)
def test_relu_and_leaky_backward_at_the_zeros(n):
    dy, y = R.act_values(n)
    for act, slope in ((R.ACT_NONE, 1.0), (R.ACT_RELU, 0.0), (R.ACT_LRELU, 0.01)):
        yt = torch.tensor(y.astype(F64), requires_grad=True)      # y of a (leaky) ReLU has the sign of its input: differentiate through y itself
        (torch.nn.functional.leaky_relu(yt, slope) * torch.from_numpy(dy.astype(F64))).sum().backward()
        got = R.act_bwd(dy, y, act)
        away = y != 0                                               # at 0 torch takes the negative side too, but keep the rule explicit below
        assert _close(got[away], yt.grad.numpy()[away], 1e-8)
        assert np.array_equal(got[~away], dy[~away].astype(F64) * float(F32(slope) if slope != 0.01 else R.LRELU))
        g32 = R.act_bwd(dy, y, act, F32)
        assert g32.dtype == F32 and _close(g32, got, R.U)
    if n >= 8:
        z = R.act_bwd(dy, y, R.ACT_RELU, F32)
        assert np.signbit(z[6]) and np.signbit(z[7]) and z[6] == 0          # a negative gradient through a dead unit is -0


def test_casts():
    x = R.cast_values(37, 16, nan=True)
    out = R.cast(x, 0)
    assert np.isnan(out.ravel()[-1]) and np.array_equal(R.bf16_bits(out.ravel()[:R.HALFWAY.size]), R.HALFWAY_BF16)
    b = R.cast_values(37, 16, bf16_exact=True)
    assert np.array_equal(R.to_bf16(b).view(np.uint32), b.view(np.uint32)) and R.differing(R.cast(b, 1), b) == 0 and R.differing(R.cast(b, 2), b) == 0
    p = R.cast(R.cast_values(37, 4), 3)
    assert p.shape == (37, 8) and np.all(p[:, 4:].view(np.uint32) == 0)


# ----------------------------------------------------------------------------------------------- planted slips
def _pairs(slip):
    """(what the GPU test would demand, what the slipped restatement gives) over the GPU test's cases of the operation the slip belongs to."""
    if slip in ('half_pixel', 'no_clamp_last_row'):
        for s in R.RESIZE_F32.values():
            x = R.resize_input(s['shape'])
            yield R.expect_resize_fwd(x), R.expect_resize_fwd(x, slip=slip)
        for s in R.RESIZE_BF16.values():
            x = R.resize_input(s['shape'], bf16=True)
            yield R.expect_resize_fwd(x, True), R.to_bf16(R.resize2x_fwd(x, F32, slip))
    elif slip in ('bwd_last_half', 'bwd_neg_tap'):
        for s in R.RESIZE_F32.values():
            dy = R.resize_gradient(s['shape'])
            yield R.expect_resize_bwd(dy), R.expect_resize_bwd(dy, slip=slip)
    elif slip == 'tie_last':
        for s in R.POOL_F32.values():
            x, dy = R.pool_inputs(s['shape'], 'ties'), R.pool_gradient(s['shape'])
            yield R.maxpool2_bwd(dy, x, F32), R.maxpool2_bwd(dy, x, F32, slip)
        for shape in R.FEAT_F32:
            gt, pred = R.features('ties', shape)
            dyp = R.pooled_gradient(shape)
            yield R.expect_feat(gt, pred, R.GHOST, R.GDEV, dyp), R.expect_feat(gt, pred, R.GHOST, R.GDEV, dyp, slip=slip)
    elif slip in ('relu_from_gt', 'l1_sign', 'l1_dropped_with_pool'):
        for shape in R.FEAT_F32:
            for kind in ('cont', 'ties'):
                gt, pred = R.features(kind, shape)
                for dyp in (None, R.pooled_gradient(shape)):
                    yield R.expect_feat(gt, pred, R.GHOST, None, dyp), R.expect_feat(gt, pred, R.GHOST, None, dyp, slip=slip)
    elif slip == 'bf16_trunc':
        x = R.cast_values(*R.CAST_VEC[:2], nan=True)
        yield R.cast(x, 0), R.cast(x, 0, slip)
        for s in R.RESIZE_BF16.values():
            x = R.resize_input(s['shape'], bf16=True)
            yield R.expect_resize_fwd(x, True), R.expect_resize_fwd(x, True, slip)
    elif slip == 'prep_bwd_255':
        for P in R.PREP_P:
            d = R.normal('prep_d', (P, 3))
            yield R.vgg_prep_bwd(d, F32), R.vgg_prep_bwd(d, F32, slip)
    elif slip == 'leaky_at_zero':
        for n in R.ACT_N:
            dy, y = R.act_values(n)
            yield R.expect_act(dy, y, R.ACT_LRELU), R.expect_act(dy, y, R.ACT_LRELU, slip=slip)
    else:
        raise AssertionError(slip)


@pytest.mark.parametrize('slip', [s for s in R.SLIPS if s != 'prep_no_swap'])
def test_every_planted_slip_changes_bits(slip):
    """The GPU test demands 0 differing elements: a slip must differ on at least one case, and the correct restatement on none."""
    counts = [R.differing(got, want) for want, got in _pairs(slip)]
    print('differing', slip, counts)
    assert len(counts) >= 1 and max(counts) > 0, (slip, counts)


def test_prep_without_the_channel_swap_misses_the_bound():
    for P in R.PREP_P:
        x = R.prep_values(P)
        r = R.worst(R.vgg_prep_fwd(x, F32, slip='prep_no_swap') - R.vgg_prep_fwd(x), R.vgg_prep_fwd_bound(x))
        assert r > 1.0, r


def test_the_slip_list_is_complete():
    assert len(R.SLIPS) >= 10
    which = {'relu_from_gt': 0, 'l1_sign': 0, 'l1_dropped_with_pool': 0}
    # the three feature-gradient slips are told apart from each other as well: no two give the same tensor on the tie case
    gt, pred = R.features('ties', R.FEAT_F32[0])
    dyp = R.pooled_gradient(R.FEAT_F32[0])
    outs = [R.expect_feat(gt, pred, R.GHOST, R.GDEV, dyp, slip=s) for s in which]
    assert all(R.differing(a, b) > 0 for i, a in enumerate(outs) for b in outs[i + 1:])
    # H = 1 is where the last-row slips collapse: the weight of the only row, and the clamp of its only neighbour
    dy = R.resize_gradient((3, 1, 9, 8))
    assert R.differing(R.resize2x_bwd(dy, F32, 'bwd_last_half'), R.resize2x_bwd(dy, F32)) == dy.size // 4
