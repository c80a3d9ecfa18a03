"""The kernels at the end of a training step against float64, at the sizes and values where they can go wrong:
kpx_adam_tf_flat_f32 / kpx_adam_tf_flat_dev_alpha_f32, kpx_sigmoid_xent_{fwd,bwd}_f32, kpx_l1_pair_{fwd,bwd}_f32 (ops.l1_mean),
kpx_l1_pair_fwd_bf16 and ops.head_blend.  Restatements, inputs and bounds live in tests/loss_optim_ref.py; tests/test_loss_optim_cpu.py
derives the restatements a second time with torch and holds an fp32 evaluation of each to the same bounds.

Bounds (fixed before measuring): 16 fp32 ulps of the magnitudes involved plus 1e-30, the bar of this suite's pointwise kernels.
  Adam          m' 16e(|m|+|gr|) ; v' 16e(|v|+gr^2) ; p' 2e|p| + 16e*alpha(|m|+|gr|)/(sqrt(v')+eps), gr = gscale*g; an element with
                g = m = v = 0 keeps the bits of p, m and v; the two entries agree bit for bit, eagerly and under graph replay
  cross-entropy group mean 16e*mean(max(x,0)+|x z|+log1p(e^-|x|)), out[0] both plus e|out[0]| ; gradient 16e(sigmoid(x)+|z|)|g|/n
  pair L1       forward 4e*ref (fp32 and bf16 entry) ; gradient exact: -g, 0 or +g with g = ghost*gdev rounded once, 0 at ties
  head blend    final 16e(|im| mask + |raw|) ; mask 16e*mask ; crude the bits of raw ; d raw[0:3] 16e|g| ;
                d raw[3] 16e*mask*sum|g|(|im|+|raw|)
Every buffer a kernel writes through the C ABI is 8 elements longer than the kernel is told, filled with a sentinel bit pattern that
must survive the launch.  Each test prints its worst error/bound ratio per entry point (``ratio <entry> <value>``).
"""
import numpy as np
import pytest
import torch

import loss_optim_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 0x7fa5c3e1                   # a NaN bit pattern no kernel here produces
GUARD = 8


@pytest.fixture(scope='module')
def kpx():
    import kpx_amd
    return kpx_amd


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def t2n(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def guarded(dev, data, lead=0):
    """(buffer, fp32 view of data.size elements starting ``lead`` elements in): sentinels before and after the view."""
    data = np.ascontiguousarray(data, dtype=np.float32).ravel()
    buf = torch.full((lead + data.size + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    view = buf[lead:lead + data.size].view(torch.float32)
    view.copy_(torch.from_numpy(data))
    assert view.data_ptr() == buf.data_ptr() + 4 * lead and buf.data_ptr() % 16 == 0
    return buf, view


def intact(buf, view):
    lead = (view.data_ptr() - buf.data_ptr()) // 4
    b = t2n(buf)
    return bool(np.all(b[:lead] == SENTINEL) and np.all(b[lead + view.numel():] == SENTINEL))


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def report(entry, ratio):
    print('ratio %s %.4f' % (entry, ratio))
    return ratio


# ----------------------------------------------------------------------------------------------- Adam
def _adam_launch(kpx, dev, entry, arrays, alpha, gs):
    """One launch of the host-alpha or dev-alpha entry on guarded copies of (p, g, m, v) -> (p', m', v') as numpy."""
    pairs = [guarded(dev, a) for a in arrays]
    P, G, M, V = (view for _, view in pairs)
    if entry == 'host':
        kpx.ops.adam_tf_flat_(P, G, M, V, alpha, R.BETA1, R.BETA2, R.ADAM_EPS, gs)
    else:
        a_dev = torch.tensor([alpha], dtype=torch.float32, device=dev)
        kpx.ops.adam_tf_flat_dev_alpha_(P, G, M, V, a_dev, R.BETA1, R.BETA2, R.ADAM_EPS, gs)
    torch.cuda.synchronize(dev)
    assert all(intact(buf, view) for buf, view in pairs), 'a guard element was overwritten'
    assert np.array_equal(bits(t2n(G)), bits(arrays[1])), 'the gradient was written'
    return t2n(P), t2n(M), t2n(V)


@pytest.mark.parametrize('n', R.ADAM_SIZES)
@pytest.mark.parametrize('gs', R.ADAM_GSCALES)
def test_adam_three_steps_both_entries_against_float64(kpx, dev, n, gs):
    """Each step is compared with the float64 step on the kernel's own previous fp32 state; the special elements are planted anew
    before every step.  n % 4 != 0 runs the scalar tail, the last size the grid-stride loop with a 3-element tail."""
    p, m, v = R.adam_state(n)
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for step in (1, 2, 3):
        g, m, v, idx = R.adam_plant(R.adam_grad(n, step), m, v, gs)
        alpha = R.adam_alpha(step)
        got = _adam_launch(kpx, dev, 'host', (p, g, m, v), alpha, gs)
        got_dev = _adam_launch(kpx, dev, 'dev', (p, g, m, v), alpha, gs)
        for name, a, b in zip('pmv', got, got_dev):
            assert np.array_equal(bits(a), bits(b)), 'step %d: %s differs between the host-alpha and dev-alpha entries' % (step, name)
        want = R.adam_step(p, g, m, v, alpha, gscale=gs)
        for name, a, w, bound in zip('pmv', got, want, R.adam_bounds(p, g, m, v, alpha, gscale=gs)):
            worst[name] = max(worst[name], R.worst(a - w, bound))
        z = idx['zero']
        for name, a, before in zip('pmv', got, (p, m, v)):
            assert np.array_equal(bits(a[z]), bits(before[z])), 'g = m = v = 0 changed %s' % name
        p, m, v = got
    report('adam n=%d gscale=%g' % (n, gs), max(worst.values()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('entry', ['host', 'dev'])
def test_adam_refuses_a_misaligned_base_and_writes_nothing(kpx, dev, entry):
    from kpx_amd._lib import KpxError
    n = 1003
    p, m, v = R.adam_state(n)
    g = R.adam_grad(n, 1)
    a_dev = torch.tensor([R.adam_alpha(1)], dtype=torch.float32, device=dev)
    for which in range(4):                                      # p, g, m, v in turn 4 bytes past a 16-byte boundary
        pairs = [guarded(dev, a, 1 if k == which else 0) for k, a in enumerate((p, g, m, v))]
        before = [t2n(buf).copy() for buf, _ in pairs]
        P, G, M, V = (view for _, view in pairs)
        with pytest.raises(KpxError):
            if entry == 'host':
                kpx.ops.adam_tf_flat_(P, G, M, V, R.adam_alpha(1), R.BETA1, R.BETA2, R.ADAM_EPS, 1.0)
            else:
                kpx.ops.adam_tf_flat_dev_alpha_(P, G, M, V, a_dev, R.BETA1, R.BETA2, R.ADAM_EPS, 1.0)
        torch.cuda.synchronize(dev)
        for (buf, _), b in zip(pairs, before):
            assert np.array_equal(t2n(buf), b)


def test_adam_dev_alpha_graph_replay_equals_the_eager_host_alpha_step(kpx, dev):
    """One captured dev-alpha launch, replayed twice with the [1] alpha tensor rewritten in between: bit-equal to two eager host-alpha steps."""
    n, gs = 4100, 1.0 / 3.0
    p, m, v = R.adam_state(n)
    g, m, v, _ = R.adam_plant(R.adam_grad(n, 1), m, v, gs)
    pairs = [guarded(dev, a) for a in (p, g, m, v)]
    P, G, M, V = (view for _, view in pairs)
    a_dev = torch.tensor([R.adam_alpha(1)], dtype=torch.float32, device=dev)

    def enqueue():
        kpx.ops.adam_tf_flat_dev_alpha_(P, G, M, V, a_dev, R.BETA1, R.BETA2, R.ADAM_EPS, gs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for view, a in zip((P, M, V), (p, m, v)):                   # undo the warm-up
        view.copy_(torch.from_numpy(a))
    state = (p, m, v)
    for step in (1, 2):
        alpha = R.adam_alpha(step)
        a_dev.copy_(torch.tensor([alpha], dtype=torch.float32))
        graph.replay()
        torch.cuda.synchronize(dev)
        want = _adam_launch(kpx, dev, 'host', (state[0], g, state[1], state[2]), alpha, gs)
        got = (t2n(P), t2n(M), t2n(V))
        for name, a, b in zip('pmv', got, want):
            assert np.array_equal(bits(a), bits(b)), 'replay %d: %s' % (step, name)
        assert all(intact(buf, view) for buf, view in pairs)
        state = want
    assert not np.array_equal(bits(state[0]), bits(p))


# ----------------------------------------------------------------------------------------------- sigmoid cross-entropy
def _xent_raw(dev, x, n0, z0, n1, z1, ghost):
    """Forward and backward through the C ABI with gdev = NULL -> (out [3], dlogits)."""
    from kpx_amd._lib import lib
    X = torch.from_numpy(x).to(dev)
    obuf, out = guarded(dev, np.zeros(3))
    dbuf, dl = guarded(dev, np.zeros(x.size))
    out.fill_(float('nan'))
    dl.fill_(float('nan'))
    assert lib.kpx_sigmoid_xent_fwd_f32(X.data_ptr(), n0, z0, n1, z1, out.data_ptr(), stream_of(dev)) == 0
    assert lib.kpx_sigmoid_xent_bwd_f32(X.data_ptr(), n0, z0, n1, z1, None, ghost, dl.data_ptr(), stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert intact(obuf, out) and intact(dbuf, dl)
    return t2n(out), t2n(dl)


def _xent_check(tag, x, n0, z0, n1, z1, g, out, dl):
    wf = R.worst(out - R.xent_fwd(x, n0, z0, n1, z1), R.xent_fwd_bounds(x, n0, z0, n1, z1) + R.TINY)
    wb = R.worst(dl - R.xent_bwd(x, n0, z0, n1, z1, g), R.xent_bwd_bounds(x, n0, z0, n1, z1, g))
    report('sigmoid_xent_fwd %s (%d,%d) labels (%g,%g)' % (tag, n0, n1, z0, z1), wf)
    report('sigmoid_xent_bwd %s (%d,%d) labels (%g,%g)' % (tag, n0, n1, z0, z1), wb)
    assert wf <= 1.0 and wb <= 1.0, (wf, wb)


@pytest.mark.parametrize('n0,n1', R.XENT_SIZES)
@pytest.mark.parametrize('z0,z1', R.XENT_LABELS)
def test_sigmoid_xent_against_float64(kpx, dev, n0, n1, z0, z1):
    """All three outputs; the gradient through autograd with dout = [2.5, 0, 0] and through the C ABI with gdev = NULL, ghost = 0.7.
    (4608, 4608) is 36 passes of the single 256-thread block; (1, 0) and (300, 0) are the generator's one-group call."""
    x = R.xent_logits(n0, n1)
    assert n0 + n1 <= 8 or all(np.any(x == np.float32(s)) for s in R.XENT_SPECIALS)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = kpx.ops.sigmoid_xent(xg, n0, z0, n1, z1)
    torch.autograd.backward([out], [torch.tensor([2.5, 0.0, 0.0], device=dev)])
    _xent_check('autograd', x, n0, z0, n1, z1, 2.5, t2n(out), t2n(xg.grad))
    _xent_check('abi', x, n0, z0, n1, z1, 0.7, *_xent_raw(dev, x, n0, z0, n1, z1, 0.7))


@pytest.mark.parametrize('z0,z1', R.XENT_LABELS)
def test_sigmoid_xent_with_an_empty_first_group(kpx, dev, z0, z1):
    n0, n1 = R.XENT_RAW_SIZE
    x = R.xent_logits(n0, n1)
    out, dl = _xent_raw(dev, x, n0, z0, n1, z1, 0.7)
    assert out[1] == 0.0 and bits(out[0]) == bits(out[2])
    _xent_check('abi', x, n0, z0, n1, z1, 0.7, out, dl)


# ----------------------------------------------------------------------------------------------- pair L1
@pytest.mark.parametrize('half,lead', [(h, 0) for h in R.L1_SIZES] + [(1027, 1)])
def test_l1_pair_fwd_bwd_against_float64(kpx, dev, half, lead):
    """half % 4 != 0 or lead = 1 (a base 4 bytes past a 16-byte boundary) take the scalar forward; the last two sizes are past the
    forward cap of 1024 blocks on the vector and the scalar path, and past the backward cap of 2048."""
    from kpx_amd._lib import lib
    f = R.l1_pair_inputs(half)
    fbuf, F = guarded(dev, f, lead)
    assert F.data_ptr() % 16 == 4 * lead
    obuf, out = guarded(dev, np.zeros(1))
    out.fill_(float('nan'))
    scratch = torch.empty(8192, dtype=torch.uint8, device=dev)
    assert lib.kpx_l1_pair_fwd_f32(F.data_ptr(), half, out.data_ptr(), scratch.data_ptr(), stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    ref = R.l1_pair_fwd(f, half)
    assert ref > 0 or half == 1
    err = abs(float(t2n(out)[0]) - ref)
    report('l1_pair_fwd half=%d lead=%d' % (half, lead), err / max(R.l1_fwd_bound(ref), R.TINY))
    assert err <= R.l1_fwd_bound(ref) and intact(obuf, out)
    gdev = torch.tensor([2.5], dtype=torch.float32, device=dev)
    ties = np.arange(R.L1_TIE_FIRST, half, R.L1_TIE_EVERY)
    for use_dev in (True, False):
        dbuf, dpred = guarded(dev, np.zeros(half))
        dpred.fill_(float('nan'))
        assert lib.kpx_l1_pair_bwd_f32(F.data_ptr(), half, gdev.data_ptr() if use_dev else None, 0.7, dpred.data_ptr(), stream_of(dev)) == 0
        torch.cuda.synchronize(dev)
        got = t2n(dpred)
        assert np.array_equal(bits(got), bits(R.l1_pair_bwd(f, half, 0.7, 2.5 if use_dev else 1.0))), use_dev
        assert not got[ties].any() and np.count_nonzero(got) == half - ties.size
        assert intact(dbuf, dpred)
    assert intact(fbuf, F) and np.array_equal(bits(t2n(F)), bits(f))


@pytest.mark.parametrize('shape', [(3,), (13, 79), (4, 262657)])          # half = 3, 1027 and 1 050 628
def test_l1_mean_scale_1000_through_autograd(kpx, dev, shape):
    """The stage-2 reconstruction loss: scale * mean|target - pred|, differentiated with respect to pred (the second half of the pair)."""
    half = int(np.prod(shape))
    f = R.l1_pair_inputs(half)
    target = torch.from_numpy(f[:half].reshape(shape)).to(dev)
    pred = torch.from_numpy(f[half:].reshape(shape)).to(dev).requires_grad_(True)
    loss = kpx.ops.l1_mean(pred, target, scale=1000.0)
    loss.backward(torch.tensor([0.37], device=dev))
    ref = 1000.0 * R.l1_pair_fwd(f, half)
    err = abs(float(t2n(loss)[0]) - ref)
    report('l1_mean half=%d' % half, err / R.l1_fwd_bound(ref))
    assert err <= R.l1_fwd_bound(ref)
    want = R.l1_pair_bwd(f, half, 1000.0 / half, 0.37).reshape(shape)
    assert pred.grad.shape == pred.shape and np.array_equal(bits(t2n(pred.grad)), bits(want))
    assert np.count_nonzero(want) > 0 and (half < 100 or (np.any(want > 0) and np.any(want < 0)))


@pytest.mark.parametrize('half', R.L1_SIZES + R.L1_BF16_SIZES)
def test_l1_pair_fwd_bf16_against_float64(kpx, dev, half):
    """The bf16 entry takes multiples of 8 only: every fp32 size is refused with the output untouched, the same sizes rounded up to 8
    (and one past this entry's own cap of 1024 * 256 * 8 elements) are held to the 4e bound on the bf16-rounded inputs."""
    from kpx_amd._lib import lib
    f = R.to_bf16(R.l1_pair_inputs(half))
    F = torch.from_numpy(f).to(dev).to(torch.bfloat16)
    assert np.array_equal(t2n(F.float()), f)
    obuf, out = guarded(dev, np.zeros(1))
    out.fill_(-7.0)
    scratch = torch.empty(8192, dtype=torch.uint8, device=dev)
    rc = lib.kpx_l1_pair_fwd_bf16(F.data_ptr(), half, out.data_ptr(), scratch.data_ptr(), stream_of(dev))
    torch.cuda.synchronize(dev)
    assert intact(obuf, out)
    if half % 8:
        assert rc == -1 and float(t2n(out)[0]) == -7.0
        return
    assert rc == 0
    ref = R.l1_pair_fwd(f, half)
    err = abs(float(t2n(out)[0]) - ref)
    report('l1_pair_fwd_bf16 half=%d' % half, err / R.l1_fwd_bound(ref))
    assert ref > 0 and err <= R.l1_fwd_bound(ref)


# ----------------------------------------------------------------------------------------------- head blend
@pytest.mark.parametrize('n,h,w', R.BLEND_SHAPES)
def test_head_blend_fwd_bwd_against_float64(kpx, dev, n, h, w):
    """P = 1, 255, 257 and one size past the cap of 2048 blocks; mask logits at +-40, +-100 and in [10, 18], |raw| > 1."""
    im, raw, g = R.blend_inputs(n, n, h, w)
    rg = torch.from_numpy(raw).to(dev).requires_grad_(True)
    img = torch.from_numpy(im).to(dev).requires_grad_(True)
    fin, crude, mask = kpx.ops.head_blend(img, rg)
    fin.backward(torch.from_numpy(g).to(dev))
    want = R.blend_fwd(im, raw)
    bf, bm = R.blend_fwd_bounds(im, raw)
    wf = report('head_blend final %s' % ((n, h, w),), R.worst(t2n(fin) - want[0], bf))
    wm = report('head_blend mask %s' % ((n, h, w),), R.worst(t2n(mask) - want[2], bm))
    wb = report('head_blend d raw %s' % ((n, h, w),), R.worst(t2n(rg.grad) - R.blend_bwd(g, im, raw), R.blend_bwd_bounds(g, im, raw)))
    assert fin.shape == (n, h, w, 3) and crude.shape == (n, h, w, 3) and mask.shape == (n, h, w, 1)
    assert np.array_equal(bits(t2n(crude)), bits(raw[..., :3]))
    assert max(wf, wm, wb) <= 1.0, (wf, wm, wb)
    assert img.grad is None                                     # the blend is not differentiated with respect to the image
