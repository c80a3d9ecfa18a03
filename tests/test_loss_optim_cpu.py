"""The restatements of tests/loss_optim_ref.py, checked without a GPU.

Independent derivation: each float64 restatement agrees with torch in float64 to 1e-12 relative (binary_cross_entropy_with_logits,
clamp / sigmoid, repeat_interleave and autograd; oracle.restatement.AdamTF for the optimiser).
Reachability: the fp32 evaluation of every restatement stays within its bound on the very inputs the GPU tests use, so every bound
is one that fp32 arithmetic can meet.
"""
import numpy as np
import pytest
import torch

import loss_optim_ref as R
from oracle import restatement as O

F64 = torch.float64


def close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300) + 1e-300)


# ----------------------------------------------------------------------------------------------- independent derivation
def test_adam_step_is_the_oracles_apply_adam_over_three_steps():
    n = 1003
    p, m, v = R.adam_state(n)
    m[:] = 0
    v[:] = 0                                                   # AdamTF starts from the zero state
    params = {'w': torch.from_numpy(p).double()}
    opt = O.AdamTF(['w'], params, beta1=R.BETA1, beta2=R.BETA2, eps=R.ADAM_EPS)
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for step in (1, 2, 3):
        g = R.adam_grad(n, step)
        assert R.adam_alpha(step) == float(opt.alpha(R.LR))
        opt.step(params, {'w': torch.from_numpy(g).double()}, R.LR)
        p64, m64, v64 = R.adam_step(p64, g, m64, v64, R.adam_alpha(step))
        assert close(p64, params['w'].numpy()) and close(m64, opt.m['w'].numpy()) and close(v64, opt.v['w'].numpy())


def test_adam_gscale_scales_the_gradient():
    n = 257
    p, m, v = R.adam_state(n)
    g = R.adam_grad(n, 1)
    a = R.adam_alpha(2)
    for gs in (0.125, 0.5):                                    # powers of two: gs*g is exact in fp32
        want = R.adam_step(p, (g * np.float32(gs)), m, v, a)
        got = R.adam_step(p, g, m, v, a, gscale=gs)
        assert all(close(x, y) for x, y in zip(got, want))


@pytest.mark.parametrize('n0,n1', R.XENT_SIZES + (R.XENT_RAW_SIZE,))
@pytest.mark.parametrize('z0,z1', R.XENT_LABELS)
def test_xent_is_torchs_bce_with_logits(n0, n1, z0, z1):
    x = R.xent_logits(n0, n1)
    z0f, z1f = float(np.float32(z0)), float(np.float32(z1))
    xt = torch.from_numpy(x).double().requires_grad_(True)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    m0 = bce(xt[:n0], torch.full((n0,), z0f, dtype=F64)) if n0 else torch.zeros((), dtype=F64)
    m1 = bce(xt[n0:], torch.full((n1,), z1f, dtype=F64)) if n1 else torch.zeros((), dtype=F64)
    (2.5 * (m0 + m1)).backward()
    m0, m1 = m0.detach(), m1.detach()
    # 1e-12 relative, and 1e-15 absolute for the saturated logits: torch forms log(1 + e^-|x|) and sigmoid(x) - z, which carry 1e-16
    # absolute in float64 whatever the size of the result (2.06e-9 at x = -20), where the restatement's log1p is exact to the last digit
    want = np.array([float(m0 + m1), float(m0), float(m1)])
    assert np.all(np.abs(R.xent_fwd(x, n0, z0, n1, z1) - want) <= 1e-12 * np.abs(want) + 1e-15)
    want = xt.grad.numpy()
    got = R.xent_bwd(x, n0, z0, n1, z1, 2.5)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-15 * 2.5 / max(min(n0 or n1, n1 or n0), 1))


@pytest.mark.parametrize('half', R.L1_SIZES[:4])
def test_pair_l1_is_torchs_l1_loss(half):
    f = R.l1_pair_inputs(half)
    gt = torch.from_numpy(f[:half]).double()
    pred = torch.from_numpy(f[half:]).double().requires_grad_(True)
    loss = torch.nn.functional.l1_loss(pred, gt, reduction='mean')
    (loss * half).backward()                                   # d sum|gt - pred| / d pred = -sign(gt - pred)
    assert close(R.l1_pair_fwd(f, half), float(loss.detach()))
    got = R.l1_pair_bwd(f, half, 0.7, 2.5)
    assert got.dtype == np.float32
    assert np.array_equal(got, pred.grad.numpy().astype(np.float32) * np.float32(np.float32(0.7) * np.float32(2.5)))
    ties = np.arange(R.L1_TIE_FIRST, half, R.L1_TIE_EVERY)
    assert np.all(got[ties] == 0) and np.count_nonzero(got) == half - ties.size


def test_bf16_rounding_is_torchs():
    a = np.random.RandomState(0).randn(4099).astype(np.float32)
    a[:4] = (1.00390625, 1.01171875, -1.00390625, 3.0)          # exact ties: to even
    assert np.array_equal(R.to_bf16(a), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize('n,h,w', R.BLEND_SHAPES[:3] + ((2, 5, 7),))
def test_blend_is_torchs_sigmoid_blend(n, h, w):
    im, raw, g = R.blend_inputs(n, n, h, w)
    rt = torch.from_numpy(raw).double().requires_grad_(True)
    mask = torch.sigmoid(rt[..., 3:])
    fin = torch.from_numpy(im).double() * mask + rt[..., :3] * (1 - mask)
    fin.backward(torch.from_numpy(g).double())
    got = R.blend_fwd(im, raw)
    assert close(got[0], fin.detach().numpy()) and np.array_equal(got[1], raw[..., :3].astype(np.float64))
    assert close(got[2], mask.detach().numpy())
    # mask*(1-mask) at a saturated logit: torch forms 1-mask (absolute 1e-16) as the restatement does
    want = rt.grad.numpy()
    assert np.all(np.abs(R.blend_bwd(g, im, raw) - want) <= 1e-12 * np.abs(want) + 1e-300)


@pytest.mark.parametrize('b,t,h,w', R.TILED_SHAPES)
@pytest.mark.parametrize('clip', [True, False])
def test_tiled_blend_is_torchs_repeat_and_clamp(b, t, h, w, clip):
    im, raw, _ = R.blend_inputs(b, b * t, h, w, seed=R.TILED_SEED)
    rt = torch.from_numpy(raw).double()
    mask = torch.sigmoid(rt[..., 3:])
    fin = torch.repeat_interleave(torch.from_numpy(im).double(), t, dim=0) * mask + rt[..., :3] * (1 - mask)
    crude = rt[..., :3]
    if clip:
        fin, crude = torch.clamp(fin, -1, 1), torch.clamp(crude, -1, 1)
    got = R.blend_tiled_fwd(im, raw, t, clip=clip)
    assert close(got[0], fin.numpy()) and np.array_equal(got[1], crude.numpy()) and close(got[2], mask.numpy())
    # the share of values the clamp acts on (the GPU test asserts the same): a clamp on `final` only, or none, cannot pass
    unclipped = R.blend_tiled_fwd(im, raw, t, clip=False)
    assert np.mean(np.abs(unclipped[0]) > 1) >= 0.25 and np.mean(np.abs(unclipped[1]) > 1) >= 0.5


@pytest.mark.parametrize('b,t,pix,c', R.TILE_CASES[:4] + (R.TILE_SLICE_CASE,))
def test_tile_batch_is_repeat_interleave(b, t, pix, c):
    x = R.tile_input(b, pix, c)
    assert np.unique(x).size == x.size
    assert np.array_equal(R.tile_batch(x, t), torch.repeat_interleave(torch.from_numpy(x), t, dim=0).numpy())


@pytest.mark.parametrize('bsz,n_in,u', [(3, 30, 64), (2, 7, 13)])
def test_lstm_cell_is_the_oracles_cell(bsz, n_in, u):
    x, h, c, kernel, bias = R.lstm_cell_inputs(bsz, n_in, u)
    xt, ht, ct, kt, bt = (torch.from_numpy(a).double() for a in (x, h, c, kernel, bias))
    i, j, f, o = torch.split(torch.cat([xt, ht], 1) @ kt + bt, u, dim=1)
    c2 = ct * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    h2 = torch.tanh(c2) * torch.sigmoid(o)
    got = R.lstm_cell(x, h, c, kernel, bias)
    assert close(got[0], h2.numpy(), 1e-11) and close(got[1], c2.numpy(), 1e-11)


@pytest.mark.parametrize('act', R.DENSE_ACTS)
def test_dense_is_torchs_linear(act):
    x, w, b = R.dense_inputs(*R.DENSE_SHAPES[0])
    z = torch.from_numpy(x).double() @ torch.from_numpy(w).double() + torch.from_numpy(b).double()
    want = {0: z, 1: torch.relu(z), 3: torch.tanh(z)}[act]
    assert R.rel_l2(R.dense(x, w, b, act), want.numpy()) < 1e-13


# ----------------------------------------------------------------------------------------------- reachability in fp32
@pytest.mark.parametrize('n', R.ADAM_SIZES)
@pytest.mark.parametrize('gs', R.ADAM_GSCALES)
def test_fp32_adam_meets_its_bounds(n, gs):
    p, m, v = R.adam_state(n)
    worst = [0.0, 0.0, 0.0]
    for step in (1, 2, 3):
        g, m, v, idx = R.adam_plant(R.adam_grad(n, step), m, v, gs)
        a = R.adam_alpha(step)
        want = R.adam_step(p, g, m, v, a, gscale=gs)
        got = R.adam_step(p, g, m, v, a, gscale=gs, dtype=np.float32)
        assert all(x.dtype == np.float32 for x in got)
        for k, (x, y, bound) in enumerate(zip(got, want, R.adam_bounds(p, g, m, v, a, gscale=gs))):
            worst[k] = max(worst[k], R.worst(x - y, bound))
        z = idx['zero']
        assert np.array_equal(got[0][z], p[z]) and not got[1][z].any() and not got[2][z].any()
        p, m, v = got
    print('fp32 Adam n=%d gscale=%g: worst error/bound  p %.3f  m %.3f  v %.3f' % ((n, gs) + tuple(worst)))
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize('n0,n1', R.XENT_SIZES + (R.XENT_RAW_SIZE,))
@pytest.mark.parametrize('z0,z1', R.XENT_LABELS)
def test_fp32_xent_meets_its_bounds(n0, n1, z0, z1):
    x = R.xent_logits(n0, n1)
    wf = R.worst(R.xent_fwd(x, n0, z0, n1, z1, dtype=np.float32) - R.xent_fwd(x, n0, z0, n1, z1),
                 R.xent_fwd_bounds(x, n0, z0, n1, z1) + R.TINY)
    wb = R.worst(R.xent_bwd(x, n0, z0, n1, z1, 2.5, dtype=np.float32) - R.xent_bwd(x, n0, z0, n1, z1, 2.5),
                 R.xent_bwd_bounds(x, n0, z0, n1, z1, 2.5))
    print('fp32 xent (%d,%d) labels (%g,%g): worst error/bound  fwd %.3f  bwd %.3f' % (n0, n1, z0, z1, wf, wb))
    assert wf <= 1.0 and wb <= 1.0


@pytest.mark.parametrize('half', R.L1_SIZES)
def test_fp32_pair_l1_meets_its_bound(half):
    f = R.l1_pair_inputs(half)
    ref = R.l1_pair_fwd(f, half)
    got = R.l1_pair_fwd(f, half, dtype=np.float32)
    assert got.dtype == np.float32 and ref > 0
    assert abs(float(got) - ref) <= R.l1_fwd_bound(ref)
    fb = R.to_bf16(f)
    assert abs(float(R.l1_pair_fwd(fb, half, dtype=np.float32)) - R.l1_pair_fwd(fb, half)) <= R.l1_fwd_bound(R.l1_pair_fwd(fb, half))


@pytest.mark.parametrize('n,h,w', R.BLEND_SHAPES)
def test_fp32_blend_meets_its_bounds(n, h, w):
    im, raw, g = R.blend_inputs(n, n, h, w)
    want, got = R.blend_fwd(im, raw), R.blend_fwd(im, raw, dtype=np.float32)
    bf, bm = R.blend_fwd_bounds(im, raw)
    wf, wm = R.worst(got[0] - want[0], bf), R.worst(got[2] - want[2], bm)
    wb = R.worst(R.blend_bwd(g, im, raw, dtype=np.float32) - R.blend_bwd(g, im, raw), R.blend_bwd_bounds(g, im, raw))
    print('fp32 blend %s: worst error/bound  final %.3f  mask %.3f  d raw %.3f' % ((n, h, w), wf, wm, wb))
    assert got[0].dtype == np.float32 and np.array_equal(got[1], raw[..., :3])
    assert max(wf, wm, wb) <= 1.0
    if n * h * w > 1:
        assert np.mean(np.abs(raw[..., :3]) > 1) > 0.5


@pytest.mark.parametrize('b,t,h,w', R.TILED_SHAPES)
@pytest.mark.parametrize('clip', [True, False])
def test_fp32_tiled_blend_meets_its_bounds(b, t, h, w, clip):
    im, raw, _ = R.blend_inputs(b, b * t, h, w, seed=R.TILED_SEED)
    want, got = R.blend_tiled_fwd(im, raw, t, clip), R.blend_tiled_fwd(im, raw, t, clip, dtype=np.float32)
    bf, bm = R.blend_fwd_bounds(np.repeat(im, t, axis=0), raw)
    assert R.worst(got[0] - want[0], bf) <= 1.0 and R.worst(got[2] - want[2], bm) <= 1.0
    assert np.array_equal(got[1], np.clip(raw[..., :3], -1, 1) if clip else raw[..., :3])


@pytest.mark.parametrize('bsz,n_in,u', R.LSTM_CELL_SHAPES)
def test_fp32_lstm_cell_meets_the_rel_l2_bar(bsz, n_in, u):
    args = R.lstm_cell_inputs(bsz, n_in, u)
    want, got = R.lstm_cell(*args), R.lstm_cell(*args, dtype=np.float32)
    assert R.rel_l2(got[0], want[0]) < 1e-5 and R.rel_l2(got[1], want[1]) < 1e-5


@pytest.mark.parametrize('rows,n_in,n_out', R.DENSE_SHAPES)
@pytest.mark.parametrize('act', R.DENSE_ACTS)
def test_fp32_dense_meets_the_rel_l2_bar(rows, n_in, n_out, act):
    x, w, b = R.dense_inputs(rows, n_in, n_out)
    assert R.rel_l2(R.dense(x, w, b, act, dtype=np.float32), R.dense(x, w, b, act)) < 1e-5


# ----------------------------------------------------------------------------------------------- the bounds reject the usual slips
def test_adam_bounds_reject_a_dropped_tail_a_missing_gscale_and_a_stale_alpha():
    n, gs = R.ADAM_SIZES[4], 1.0 / 3.0
    p, m, v = R.adam_state(n)
    g, m, v, _ = R.adam_plant(R.adam_grad(n, 1), m, v, gs)
    a = R.adam_alpha(1)
    want, bounds = R.adam_step(p, g, m, v, a, gscale=gs), R.adam_bounds(p, g, m, v, a, gscale=gs)
    tail = [x.astype(np.float64) for x in R.adam_step(p, g, m, v, a, gscale=gs, dtype=np.float32)]
    for k, before in enumerate((p, m, v)):
        tail[k][n - n % 4:] = before[n - n % 4:]              # the scalar tail loop never ran
    slips = {'dropped tail': tail, 'gscale ignored': R.adam_step(p, g, m, v, a), 'alpha of the next step': R.adam_step(p, g, m, v, R.adam_alpha(2), gscale=gs)}
    for name, got in slips.items():
        assert max(R.worst(x - y, b) for x, y, b in zip(got, want, bounds)) > 1.0, name


def test_blend_and_l1_checks_reject_the_usual_slips():
    b, t, h, w = R.TILED_SHAPES[1]
    im, raw, _ = R.blend_inputs(b, b * t, h, w, seed=R.TILED_SEED)
    want = R.blend_tiled_fwd(im, raw, t, clip=True)
    bf, _ = R.blend_fwd_bounds(np.repeat(im, t, axis=0), raw)
    modulo = R.blend_fwd(im[np.arange(b * t) % b], raw)[0]                      # image f % B (what f % T indexes when T = B) for f // T
    assert R.worst(np.clip(modulo, -1, 1) - want[0], bf) > 1.0
    assert R.worst(R.blend_tiled_fwd(im, raw, t, clip=False)[0] - want[0], bf) > 1.0          # no clamp on final
    half = R.L1_SIZES[3]
    f = R.l1_pair_inputs(half)
    swapped = R.l1_pair_bwd(np.concatenate([f[half:], f[:half]]), half, 0.7)               # pred - gt for gt - pred
    assert not np.array_equal(swapped, R.l1_pair_bwd(f, half, 0.7))
