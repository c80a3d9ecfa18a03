"""csrc/keypoints.hip against float64 at the shapes, values and launch paths where it can go wrong: kpx_keypoint_head_{fwd,bwd}_f32,
kpx_keypoint_head_proj_{fwd,bwd}_f32 and kpx_gaussian_maps_{fwd,bwd}_f32.  Restatements, seeded inputs and bounds live in
tests/keypoints_ref.py (its header lists every bound and derives the terms that are wider than n*e); tests/test_keypoints_cpu.py derives
the restatements a second time with torch autograd, holds a sequential-fp32 evaluation of each to the same bounds and shows that the
bounds reject the planted slips.

Every buffer an entry writes goes through the C ABI with 8 sentinel words after it (and before it where a lead is used), the kphead /
kpproj scratch included, sized exactly by the *_scratch_bytes query: the sentinels must survive every launch, the inputs must keep
their bits.  Backward entries are checked pointwise on the kernel's own saved state.  Each test prints ``ratio <entry> <worst error/bound>``.
"""
import numpy as np
import pytest
import torch

import keypoints_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 0x7fa5c3e1                   # a NaN bit pattern no kernel here produces
GUARD = 8
EINVAL = -1
F64 = np.float64


@pytest.fixture(scope='module')
def kpx():
    import kpx_amd
    return kpx_amd


@pytest.fixture(scope='module')
def lib(kpx):
    from kpx_amd import _lib
    return _lib.lib


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


def blank(dev, n, lead=0):
    """An output of n floats: the view itself starts as sentinels too, so an element a kernel skips, or a refused call, shows."""
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[lead:lead + n].view(torch.float32)


def intact(buf, view):
    lead = (view.data_ptr() - buf.data_ptr()) // 4
    b = t2n(buf)
    return bool(np.all(b[:lead] == SENTINEL) and np.all(b[lead + view.numel():] == SENTINEL))


def untouched(buf):
    return bool(np.all(t2n(buf) == SENTINEL))


def written(view):
    return not np.any(t2n(view).view(np.uint32) == SENTINEL)


def same_bits(pair, array):
    return np.array_equal(bits(t2n(pair[1])).ravel(), bits(array).ravel())


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def report(entry, ratio):
    print('ratio %s %.4f' % (entry, ratio))
    return ratio


def P(pair):
    return None if pair is None else pair[1].data_ptr()


# ----------------------------------------------------------------------------------------------- head
def _head_fwd(lib, dev, x):
    """kpx_keypoint_head_fwd_f32 on guarded buffers -> (mu, py, px) pairs; guards, scratch guards and the input checked."""
    b, h, w, k = x.shape
    xin = guarded(dev, x)
    outs = [blank(dev, b * k * 2), blank(dev, b * h * k), blank(dev, b * w * k)]
    nbytes = lib.kpx_keypoint_head_scratch_bytes(b, h, w, k)
    assert nbytes == 4 * (b * h * k + b * ((h + 7) // 8) * w * k)
    sc = blank(dev, nbytes // 4)
    rc = lib.kpx_keypoint_head_fwd_f32(P(xin), b, h, w, k, P(outs[0]), P(outs[1]), P(outs[2]), P(sc), stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0
    assert all(intact(*o) for o in outs) and intact(*sc) and intact(*xin), 'a guard element was overwritten'
    assert all(written(o[1]) for o in outs), 'an output element was never written'
    assert same_bits(xin, x), 'the logits were written'
    return outs


def _head_bwd(lib, dev, dmu, outs, shape):
    b, h, w, k = shape
    din = guarded(dev, dmu)
    dl = blank(dev, b * h * w * k)
    before = [t2n(o[1]).copy() for o in outs]
    rc = lib.kpx_keypoint_head_bwd_f32(P(din), P(outs[0]), P(outs[1]), P(outs[2]), b, h, w, k, P(dl), stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and intact(*dl) and written(dl[1]) and intact(*din) and same_bits(din, dmu)
    assert all(intact(*o) and same_bits(o, a) for o, a in zip(outs, before)), 'the saved state was written'
    return t2n(dl[1]).reshape(shape)


@pytest.mark.parametrize('shape', R.HEAD_SHAPES)
@pytest.mark.parametrize('regime', R.HEAD_REGIMES)
def test_head_forward_and_backward_against_float64(lib, dev, shape, regime):
    """(2,13,21,5): partial stripe, H != W, 256 % K != 0.  (1,70,130,3): 9 stripes, two and three registers per lane.  (1,512,2,1) and
    (1,2,512,1): both limits, K = 1 (256 groups).  (1,8,8,256): T = 256.  (1,8,12,129): one group, 127 idle threads."""
    b, h, w, k = shape
    x = R.head_logits(shape, regime)
    dmu = R.head_dmu(shape)
    outs = _head_fwd(lib, dev, x)
    got = [t2n(o[1]).reshape(s) for o, s in zip(outs, ((b, k, 2), (b, h, k), (b, w, k)))]
    assert all(np.all(np.isfinite(g)) for g in got), 'NaN or infinity (%s)' % regime
    ref, bnd = R.head(x), R.head_bounds(x)
    ratios = {n: R.worst(g - r, bb) for n, g, r, bb in zip(('mu', 'py', 'px'), got, ref, bnd)}
    report('kpx_keypoint_head_fwd_f32 %s %s' % (shape, regime), max(ratios.values()))
    dl = _head_bwd(lib, dev, dmu, outs, shape)
    rb = R.worst(dl - R.head_bwd(dmu, *got, h, w), R.head_bwd_bound(dmu, *got, h, w))
    report('kpx_keypoint_head_bwd_f32 %s %s' % (shape, regime), rb)
    assert max(ratios.values()) <= 1.0, ratios
    assert rb <= 1.0
    if regime in ('spike', 'huge'):
        # the largest mean of every profile leads by more than any fp32 evaluation can blur: exactly one-hot, mu an fp32 grid value
        assert R.head_one_hot_margin(x) > 104 and R.head_one_hot_ok(x, *got)
    if shape in R.HEAD_SHAPES[:2] and regime != 'huge':
        # against the float64 gradient of the float64 forward: the backward bound plus what the forward's bounds let through
        full = R.worst(dl - R.head_bwd(dmu, *ref, h, w), R.head_bwd_bound(dmu, *got, h, w) + R.head_bwd_forward_part(dmu, x))
        report('kpx_keypoint_head_bwd_f32 through the forward %s %s' % (shape, regime), full)
        assert full <= 1.0


def test_head_forward_refused_call_leaves_its_outputs_alone(lib, dev):
    b, h, w, k = R.HEAD_SHAPES[0]
    xin = guarded(dev, R.head_logits((b, h, w, k), 'normal'))
    outs = [blank(dev, b * k * 2), blank(dev, b * h * k), blank(dev, b * w * k)]
    sc = blank(dev, lib.kpx_keypoint_head_scratch_bytes(b, h, w, k) // 4)
    assert lib.kpx_keypoint_head_fwd_f32(P(xin), b, 513, w, k, P(outs[0]), P(outs[1]), P(outs[2]), P(sc), stream_of(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert all(untouched(o[0]) for o in outs) and untouched(sc[0])


# ----------------------------------------------------------------------------------------------- folded head
def _proj_fwd(lib, dev, x, wk, bk):
    b, h, w, c = x.shape
    k = wk.shape[1]
    ins = [guarded(dev, x), guarded(dev, wk), guarded(dev, bk) if bk is not None else None]
    outs = [blank(dev, n) for n in (b * k * 2, b * h * k, b * w * k, b * h * c, b * w * c)]
    nbytes = lib.kpx_keypoint_head_proj_scratch_bytes(b, h, w, c, k)
    assert nbytes == 4 * max(b * ((h + 7) // 8) * w * c, b * (h + w) * c + 2 * b * (c * k + k))
    sc = blank(dev, nbytes // 4)
    rc = lib.kpx_keypoint_head_proj_fwd_f32(P(ins[0]), P(ins[1]), P(ins[2]), b, h, w, c, k, *(P(o) for o in outs), P(sc), stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0
    assert all(intact(*o) and written(o[1]) for o in outs) and intact(*sc), 'a guard element was overwritten or an output skipped'
    assert all(intact(*i) and same_bits(i, a) for i, a in zip(ins, (x, wk, bk)) if i is not None), 'an input was written'
    return ins, outs, sc


def _proj_bwd(lib, dev, dmu, ins, outs, sc, dims, want=(True, True, True), accumulate=0, prefill=None):
    """-> [dx, dw, db] as numpy (None where the pointer was null); every guard and the saved state checked."""
    b, h, w, c, k = dims
    din = guarded(dev, dmu)
    sizes = (b * h * w * c, c * k, k)
    res = [(blank(dev, n) if prefill is None or i == 0 else guarded(dev, prefill[i])) if on else None for i, (n, on) in enumerate(zip(sizes, want))]
    before = [t2n(o[1]).copy() for o in outs]
    rc = lib.kpx_keypoint_head_proj_bwd_f32(P(din), *(P(o) for o in outs), P(ins[1]), b, h, w, c, k, P(res[0]), P(res[1]), P(res[2]),
                                            accumulate, P(sc), stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and intact(*sc) and intact(*din) and same_bits(din, dmu)
    assert all(intact(*r) and written(r[1]) for r in res if r is not None), 'a guard element was overwritten or an output skipped'
    assert all(intact(*o) and same_bits(o, a) for o, a in zip(outs, before)), 'the saved state was written'
    return [None if r is None else t2n(r[1]) for r in res]


@pytest.mark.parametrize('shape,bias', R.PROJ_SHAPES)
@pytest.mark.parametrize('regime', ['normal', 'wide', 'spike'])
def test_folded_head_against_float64_conv_then_head(lib, dev, shape, bias, regime):
    """(1,70,130,4,3): 9 stripes, one unrolled block of 8 plus a tail.  (9,8,12,8,17): 18 partial rows (unrolled reduce plus tail), K = 17
    sends k = 16 back to workgroup z = 0.  (1,16,16,4,64): four-way K split.  (1,8,8,256,1): one workgroup in z.  (1,480,2,32,32):
    exactly at the LDS limit.  (2,24,40,8,5): no bias."""
    b, h, w, c, k = shape
    x, wk, bk = R.proj_inputs(shape, bias, regime)
    dmu = R.head_dmu((b, h, w, k))
    assert lib.kpx_keypoint_head_proj_eligible(b, h, w, c, k) == 1
    ins, outs, sc = _proj_fwd(lib, dev, x, wk, bk)
    shapes = ((b, k, 2), (b, h, k), (b, w, k), (b, h, c), (b, w, c))
    got = [t2n(o[1]).reshape(s) for o, s in zip(outs, shapes)]
    x64 = x.astype(F64)
    ref = R.head(x64 @ wk.astype(F64) + (0.0 if bk is None else bk.astype(F64))) + (x64.sum(axis=2), x64.sum(axis=1))
    ratios = {n: R.worst(g - r, bb) for n, g, r, bb in zip(('mu', 'py', 'px', 'xs_y', 'xs_x'), got, ref, R.head_proj_bounds(x, wk, bk))}
    report('kpx_keypoint_head_proj_fwd_f32 %s %s' % (shape, regime), max(ratios.values()))
    assert max(ratios.values()) <= 1.0, ratios

    full = _proj_bwd(lib, dev, dmu, ins, outs, sc, shape)
    want = R.head_proj_bwd(dmu, *got, wk, h, w)
    bounds = R.head_proj_bwd_bounds(dmu, *got, wk, h, w)
    rb = {n: R.worst(g.reshape(r.shape) - r, bb) for n, g, r, bb in zip(('dx', 'dw', 'db'), full, want, bounds)}
    report('kpx_keypoint_head_proj_bwd_f32 %s %s' % (shape, regime), max(rb.values()))
    assert max(rb.values()) <= 1.0, rb
    if regime != 'normal':
        return
    for off in range(3):                                        # dx, dw, db null one at a time: the others keep their bits
        on = tuple(i != off for i in range(3))
        part = _proj_bwd(lib, dev, dmu, ins, outs, sc, shape, want=on)
        assert part[off] is None
        assert all(np.array_equal(bits(p), bits(f)) for i, (p, f) in enumerate(zip(part, full)) if i != off), 'null pointer %d' % off
    # accumulate = 1: pre-fill + fresh result, one more rounding
    rng = np.random.RandomState(11)
    pre = [None, rng.standard_normal(c * k).astype(np.float32), rng.standard_normal(k).astype(np.float32)]
    acc = _proj_bwd(lib, dev, dmu, ins, outs, sc, shape, accumulate=1, prefill=pre)
    assert np.array_equal(bits(acc[0]), bits(full[0]))
    for i, name in ((1, 'dw'), (2, 'db')):
        exact = pre[i].astype(F64) + want[i].ravel()
        assert R.worst(acc[i] - exact, bounds[i].ravel() + R.U * np.abs(exact)) <= 1.0, name
        assert np.array_equal(bits(acc[i]), bits(pre[i] + full[i])), name       # and it is the fp32 sum of the two


def test_folded_head_op_claims_a_gradient_slot_fresh_and_then_accumulates(kpx, lib, dev):
    """ops.keypoint_head_proj with w_grad_out / b_grad_out used twice in one backward: the first use overwrites what the slot held, the
    second adds to it."""
    shape = (2, 13, 21, 8, 5)
    b, h, w, c, k = shape
    x1, wk, bk = R.proj_inputs(shape, True)
    x2 = R.proj_inputs(shape, True, seed=5)[0]
    d1, d2 = R.head_dmu((b, h, w, k)), R.head_dmu((b, h, w, k), seed=9)
    fresh = []
    for x, d in ((x1, d1), (x2, d2)):
        ins, outs, sc = _proj_fwd(lib, dev, x, wk, bk)
        fresh.append(_proj_bwd(lib, dev, d, ins, outs, sc, shape))
    wt = torch.from_numpy(wk.reshape(1, 1, c, k)).to(dev).requires_grad_(True)
    bt = torch.from_numpy(bk).to(dev).requires_grad_(True)
    wg = torch.full((1, 1, c, k), 7.0, dtype=torch.float32, device=dev)
    bg = torch.full((k,), -3.0, dtype=torch.float32, device=dev)
    xt = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in (x1, x2)]
    kpx.ops.begin_backward()
    mus = [kpx.ops.keypoint_head_proj(x, wt, bt, w_grad_out=wg, b_grad_out=bg)[0] for x in xt]
    loss = (mus[0] * torch.from_numpy(d1).to(dev)).sum() + (mus[1] * torch.from_numpy(d2).to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize(dev)
    assert wt.grad is None and bt.grad is None
    for x, f in zip(xt, fresh):
        assert np.array_equal(bits(t2n(x.grad).ravel()), bits(f[0]))
    for got, i in ((wg, 1), (bg, 2)):
        g = t2n(got).ravel()
        a, bb = fresh[0][i], fresh[1][i]
        assert np.array_equal(bits(g), bits(a + bb)) or np.array_equal(bits(g), bits(bb + a))
    assert not np.any(t2n(wg) == 7.0)


# ----------------------------------------------------------------------------------------------- Gaussian maps, forward
def _gauss_fwd(lib, dev, mu_pair, dims, inv_std, ldy, lead=0):
    b, k, h, w = dims
    out = blank(dev, b * h * w * ldy, lead=lead)
    rc = lib.kpx_gaussian_maps_fwd_f32(P(mu_pair), b, k, h, w, float(inv_std), P(out), ldy, stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and intact(*out) and intact(*mu_pair)
    return t2n(out[1]).reshape(b, h, w, ldy)


GAUSS_RUNS = [(dims, path, inv, off) for dims, path, invs, off in R.GAUSS_CASES for inv in invs]


@pytest.mark.parametrize('dims,path,inv_std,offset', GAUSS_RUNS)
def test_gaussian_maps_forward_three_ways(lib, dev, dims, path, inv_std, offset):
    """Against float64 under the bound, bit for bit against the strided renderer (ldy = K + 3 into a wider buffer whose other columns keep
    their sentinels) and bit for bit against a second launch.  ``path`` is the branch of kpx_gaussian_maps_fwd_f32 the contiguous launch
    takes (keypoints_ref.gauss_path restates the selection; test_keypoints_cpu.py holds the table to it)."""
    b, k, h, w = dims
    assert R.gauss_path(b, k, h, w, aligned=not offset)[0] == path
    large = b == 512 or h * w * k >= (1 << 23)
    worst = 0.0
    for regime in (('inside',) if large else R.MU_REGIMES):
        mu = R.gauss_mu(b, k, h, w, regime)
        mu_pair = guarded(dev, mu)
        got = _gauss_fwd(lib, dev, mu_pair, dims, inv_std, k, lead=offset)
        assert not np.any(got.view(np.uint32) == SENTINEL), 'an element was never written'
        again = _gauss_fwd(lib, dev, mu_pair, dims, inv_std, k, lead=offset)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), 'two launches differ'
        wide = _gauss_fwd(lib, dev, mu_pair, dims, inv_std, k + 3)
        assert np.array_equal(wide[..., :k].view(np.uint32), got.view(np.uint32)), 'the %s path and the strided renderer differ' % path
        assert np.all(wide[..., k:].view(np.uint32) == SENTINEL), 'the strided renderer wrote outside its channel slice'
        assert same_bits(mu_pair, mu)
        del wide, again
        if h * w * k >= (1 << 23):
            rng = np.random.RandomState(5)
            idx = (np.zeros(4096, int), rng.randint(0, h, 4096), rng.randint(0, w, 4096), rng.randint(0, k, 4096))
            ref, bound = R.gauss_at(mu, h, w, inv_std, *idx)
            worst = max(worst, R.worst(got[idx] - ref, bound))
        else:
            for img in ((0, b - 1) if b == 512 else (slice(None),)):
                sel = slice(img, img + 1) if b == 512 else img
                ref, bound = R.gauss_with_bound(mu[sel], h, w, inv_std)
                worst = max(worst, R.worst(got[sel] - ref, bound))
    report('kpx_gaussian_maps_fwd_f32 %s %s inv_std=%g' % (dims, path, inv_std), worst)
    assert worst <= 1.0


def test_gaussian_forward_refused_call_leaves_its_output_alone(lib, dev):
    b, k, h, w = 2, 15, 32, 32
    mu_pair = guarded(dev, R.gauss_mu(b, k, h, w, 'inside'))
    out = blank(dev, b * h * w * k)
    assert lib.kpx_gaussian_maps_fwd_f32(P(mu_pair), b, k, h, w, 14.3, P(out), k - 1, stream_of(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert untouched(out[0])


# ----------------------------------------------------------------------------------------------- Gaussian maps, backward
def _gauss_bwd(lib, dev, dm, mu, dims, inv_std, lddy):
    """dmaps laid out with lddy columns per pixel, the extra ones NaN bit patterns that must not be read."""
    b, k, h, w = dims
    padded = np.full((b, h, w, lddy), np.float32(0), np.float32).view(np.uint32)
    padded[...] = 0x7fc00001
    padded[..., :k] = dm.view(np.uint32)
    din, mu_pair = guarded(dev, padded.view(np.float32)), guarded(dev, mu)
    out = blank(dev, b * k * 2)
    rc = lib.kpx_gaussian_maps_bwd_f32(P(din), lddy, P(mu_pair), b, k, h, w, float(inv_std), P(out), stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and intact(*out) and written(out[1]) and intact(*din) and intact(*mu_pair)
    assert np.array_equal(t2n(din[1]).view(np.uint32), padded.ravel()) and same_bits(mu_pair, mu), 'an input was written'
    return t2n(out[1]).reshape(b, k, 2)


@pytest.mark.parametrize('k,h,w', R.GAUSS_BWD_CASES)
@pytest.mark.parametrize('inv_std', R.GAUSS_BWD_INV_STDS)
def test_gaussian_maps_backward_against_float64(lib, dev, k, h, w, inv_std):
    """K = 1: 256 pixel groups; K = 15: 17 groups and 1 idle thread; K = 129: one group, 127 idle threads; K = 256: one group, none idle."""
    b = 2
    worst = 0.0
    dm = R.gauss_dmaps(b, h, w, k)
    for regime in R.MU_REGIMES:
        mu = R.gauss_mu(b, k, h, w, regime)
        want, bound = R.gauss_bwd(dm, mu, h, w, inv_std), R.gauss_bwd_bound(dm, mu, h, w, inv_std)
        plain = _gauss_bwd(lib, dev, dm, mu, (b, k, h, w), inv_std, k)
        padded = _gauss_bwd(lib, dev, dm, mu, (b, k, h, w), inv_std, k + 5)
        assert np.all(np.isfinite(plain)) and np.array_equal(bits(plain), bits(padded)), 'lddy = K + 5 changed the result (%s)' % regime
        worst = max(worst, R.worst(plain - want, bound))
    report('kpx_gaussian_maps_bwd_f32 K=%d %dx%d inv_std=%g' % (k, h, w, inv_std), worst)
    assert worst <= 1.0


def test_gaussian_backward_refused_call_leaves_dmu_alone(lib, dev):
    b, k, h, w = 1, 257, 9, 14
    din = guarded(dev, np.zeros((b, h, w, k), np.float32))
    mu_pair = guarded(dev, np.zeros((b, k, 2), np.float32))
    out = blank(dev, b * k * 2)
    assert lib.kpx_gaussian_maps_bwd_f32(P(din), k, P(mu_pair), b, k, h, w, 14.3, P(out), stream_of(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert untouched(out[0])


# ----------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_of_head_and_maps_equals_the_eager_launches(lib, dev):
    """Head forward + backward and map forward + backward, captured on one stream (no parallel branches), replayed twice."""
    hs = R.HEAD_SHAPES[0]
    b, h, w, k = hs
    gb, gk, gh, gw = R.GAUSS_CASES[0][0]
    x, dmu = R.head_logits(hs, 'normal'), R.head_dmu(hs)
    gmu, gdm = R.gauss_mu(gb, gk, gh, gw, 'inside'), R.gauss_dmaps(gb, gh, gw, gk)
    outs = _head_fwd(lib, dev, x)
    eager = [t2n(o[1]).copy() for o in outs] + [_head_bwd(lib, dev, dmu, outs, hs).ravel()]
    mu_pair = guarded(dev, gmu)
    eager.append(_gauss_fwd(lib, dev, mu_pair, (gb, gk, gh, gw), 14.3, gk).ravel())
    eager.append(_gauss_bwd(lib, dev, gdm, gmu, (gb, gk, gh, gw), 14.3, gk).ravel())

    xin, din, gdin = guarded(dev, x), guarded(dev, dmu), guarded(dev, gdm)
    res = [blank(dev, n) for n in (b * k * 2, b * h * k, b * w * k, b * h * w * k, gb * gh * gw * gk, gb * gk * 2)]
    sc = blank(dev, lib.kpx_keypoint_head_scratch_bytes(b, h, w, k) // 4)
    codes = []

    def enqueue():
        s = stream_of(dev)
        codes.append(lib.kpx_keypoint_head_fwd_f32(P(xin), b, h, w, k, P(res[0]), P(res[1]), P(res[2]), P(sc), s))
        codes.append(lib.kpx_keypoint_head_bwd_f32(P(din), P(res[0]), P(res[1]), P(res[2]), b, h, w, k, P(res[3]), s))
        codes.append(lib.kpx_gaussian_maps_fwd_f32(P(mu_pair), gb, gk, gh, gw, 14.3, P(res[4]), gk, s))
        codes.append(lib.kpx_gaussian_maps_bwd_f32(P(gdin), gk, P(mu_pair), gb, gk, gh, gw, 14.3, P(res[5]), s))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    assert codes == [0] * 8
    for _ in range(2):
        for buf, _view in res:
            buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize(dev)
        for r, e in zip(res, eager):
            assert intact(*r) and np.array_equal(bits(t2n(r[1])), bits(e))
        assert intact(*sc)
