"""The streaming kernels of csrc/pointwise.hip outside batch norm, bit for bit at their edges: kpx_resize2x_{fwd,bwd}_{f32,bf16},
kpx_maxpool2_{fwd,bwd}_f32, kpx_maxpool2_fwd_bf16, kpx_vgg_feat_bwd_{f32,bf16}, kpx_vgg_prep_{fwd,bwd}_f32, kpx_act_bwd_{f32,bf16},
kpx_cast_channels (kinds 0-3), kpx_copy_channels_f32, kpx_axpy_f32, kpx_fill_f32.  Restatements, seeded inputs, case lists and the three
bounds live in tests/streaming_ref.py (its header says why fp32 numpy can repeat these kernels exactly); tests/test_streaming_cpu.py holds
the restatements to the oracle and torch autograd and shows every planted slip rejected on these cases.

Everything runs through the C ABI.  Every output has 8 sentinel words behind it (and in front where a lead is used) and keeps its gap
channels between C and ld; every output element must be written, inputs must keep their bits (their gap channels hold NaN: a kernel that
reads one shows), a refused call returns KPX_EINVAL and writes nothing.  A bit-exact check prints ``differing <entry> <count>`` (must be 0),
a bounded one ``ratio <entry> <worst error/bound>`` (must be <= 1).

One branch is left out: resize2x_fwd_kernel<true> (the per-output-pixel vector kernel) runs only from 2^31 - 1 channel quads on, more than
32 GB of input; no test tries to reach it."""
import numpy as np
import pytest
import torch

import streaming_ref as R
from test_batchnorm_gpu import HALVES, Buf
from test_keypoints_gpu import EINVAL, GUARD, SENTINEL, report, stream_of

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def lib():
    from kpx_amd import _lib
    return _lib.lib


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


class SBuf(Buf):
    """Buf that also takes an odd number of bf16 slots (the half word behind the last element is one more gap slot) and wants every output
    element fresh on its own: no value stored here is a half of the sentinel word."""

    def __init__(self, dev, rows, C, ld, lead=0, data=None, half=False):
        n = (rows - 1) * ld + C
        if not (half and n % 2):
            super().__init__(dev, rows, C, ld, lead, data, half)
            return
        self.half, self.lead, self.words, self.shape = True, lead, (n + 1) // 2, (rows, C)
        self.buf = torch.full((lead + self.words + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.view = self.buf[lead:lead + self.words].view(torch.bfloat16)
        assert self.view.numel() == n + 1 and self.view.data_ptr() == self.buf.data_ptr() + 4 * lead
        self.idx = (np.arange(rows)[:, None] * ld + np.arange(C)[None, :]).ravel()
        self.gap = np.ones(n + 1, bool)
        self.gap[self.idx] = False
        self.pattern = HALVES[np.arange(n + 1) % 2]
        self.data = None
        if data is not None:
            self.data = np.ascontiguousarray(data, dtype=F32).reshape(rows, C)
            full = np.full(n + 1, np.nan, F32)
            full[self.idx] = self.data.ravel()
            self.view.copy_(torch.from_numpy(full))

    def output_ok(self):
        r = self.raw()
        assert self.guards_ok(), 'a guard word was overwritten'
        assert np.all(r[self.gap] == self.pattern[self.gap]), 'a gap channel between C and ld was written'
        assert np.all(r[self.idx] != self.pattern[self.idx]), 'an output element was never written'
        return True


class Big:
    """A large contiguous output, checked on the device: ``words`` sentinel words and the guard behind them."""

    def __init__(self, dev, words, half=False):
        self.words, self.half = words, half
        self.buf = torch.full((words + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        inner = self.buf[:words]
        self.view = inner.view(torch.bfloat16) if half else inner.view(torch.float32)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def output_ok(self):
        assert bool((self.buf[self.words:] == SENTINEL).all()), 'a guard word was overwritten'
        inner = self.buf[:self.words]
        if self.half:
            h = inner.view(torch.int16)
            assert bool((h[0::2] != int(HALVES[0])).all()) and bool((h[1::2] != int(HALVES[1])).all()), 'an output element was never written'
        else:
            assert bool((inner != SENTINEL).all()), 'an output element was never written'
        return True


def flat(dev, data, lead=0, half=False):
    data = np.asarray(data, F32).ravel()
    return SBuf(dev, 1, data.size, data.size, lead, data, half)


def blank(dev, n, lead=0, half=False):
    return SBuf(dev, 1, n, n, lead, half=half)


def same(entry, got, want):
    """Bit equality with the restatement (streaming_ref.differing: a NaN there wants a NaN here, whatever its payload)."""
    n = R.differing(got, want)
    print('differing %s %d' % (entry, n))
    assert n == 0, '%s: %d of %d elements differ' % (entry, n, np.size(want))


def geometry(s):
    n, h, w, c = s['shape']
    return n, h, w, c, s.get('ldx', c), s.get('ldy', c), s.get('lead', 0)


# ----------------------------------------------------------------------------------------------- resize x2
def resize_pair(lib, dev, s, half, label):
    n, h, w, c, ldx, ldy, lead = geometry(s)
    suffix = 'bf16' if half else 'f32'
    fwd, bwd = getattr(lib, 'kpx_resize2x_fwd_' + suffix), getattr(lib, 'kpx_resize2x_bwd_' + suffix)
    x = R.resize_input(s['shape'], half)
    xb, yb = SBuf(dev, n * h * w, c, ldx, lead, x.reshape(-1, c), half), SBuf(dev, 4 * n * h * w, c, ldy, lead, half=half)
    assert fwd(xb.ptr, n, h, w, c, ldx, yb.ptr, ldy, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert xb.input_ok() and yb.output_ok()
    same('kpx_resize2x_fwd_%s %s' % (suffix, label), yb.get(), R.expect_resize_fwd(x, half))
    dy = R.resize_gradient(s['shape'], half)
    db, dxb = SBuf(dev, 4 * n * h * w, c, ldy, lead, dy.reshape(-1, c), half), SBuf(dev, n * h * w, c, ldx, lead, half=half)
    assert bwd(db.ptr, n, h, w, c, ldy, dxb.ptr, ldx, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert db.input_ok() and dxb.output_ok()
    same('kpx_resize2x_bwd_%s %s' % (suffix, label), dxb.get(), R.expect_resize_bwd(dy, half))


@pytest.mark.parametrize('name', list(R.RESIZE_F32))
def test_resize_fp32_forward_and_backward_bit_for_bit(lib, dev, name):
    """The input-pixel (quad) kernel and the scalar one; the backward's vector and scalar kernels on the same shapes: ld > C on either side,
    H = 1, W = 1, a single pixel, C % 4, ld % 4 and a 4-byte-offset base."""
    resize_pair(lib, dev, R.RESIZE_F32[name], False, name)


@pytest.mark.parametrize('name', list(R.RESIZE_BF16))
def test_resize_bf16_forward_and_backward_bit_for_bit(lib, dev, name):
    resize_pair(lib, dev, R.RESIZE_BF16[name], True, name)


def test_resize_refusals_write_nothing(lib, dev):
    n, h, w, c = 2, 5, 7, 16
    x = R.resize_input((n, h, w, c), True)
    st = stream_of(dev)
    for change in (dict(c=4), dict(ld=20), dict(lead=1), dict(ld=8)):                  # C % 8, ld % 8, a 4-byte-offset base, ld < C
        lead, cc, bad = change.get('lead', 0), change.get('c', c), change.get('ld', 24)
        small, large = SBuf(dev, n * h * w, c, 24, lead, half=True), SBuf(dev, 4 * n * h * w, c, 24, lead, half=True)
        src, grad = SBuf(dev, n * h * w, c, 24, lead, x.reshape(-1, c), True), SBuf(dev, 4 * n * h * w, c, 24, lead, np.ones((4 * n * h * w, c)), True)
        for ldx, ldy in ((bad, 24), (24, bad)):
            assert lib.kpx_resize2x_fwd_bf16(src.ptr, n, h, w, cc, ldx, large.ptr, ldy, st) == EINVAL
            assert lib.kpx_resize2x_bwd_bf16(grad.ptr, n, h, w, cc, ldy, small.ptr, ldx, st) == EINVAL
        torch.cuda.synchronize(dev)
        assert small.untouched() and large.untouched() and src.input_ok() and grad.input_ok()
    xf, yf = SBuf(dev, n * h * w, c, c, 0, x.reshape(-1, c)), SBuf(dev, 4 * n * h * w, c, c)
    for args in ((0, h, w, c, c, c), (n, h, w, c, c - 1, c), (n, h, w, c, c, c - 1), (n, 0, w, c, c, c)):
        assert lib.kpx_resize2x_fwd_f32(xf.ptr, *args[:5], yf.ptr, args[5], st) == EINVAL
        assert lib.kpx_resize2x_bwd_f32(yf.ptr, *args[:4], args[5], xf.ptr, args[4], st) == EINVAL
    assert lib.kpx_resize2x_fwd_f32(None, n, h, w, c, c, yf.ptr, c, st) == EINVAL
    torch.cuda.synchronize(dev)
    assert yf.untouched() and xf.input_ok()


# ----------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize('name', list(R.POOL_F32))
@pytest.mark.parametrize('kind', ['cont', 'ties'])
def test_maxpool_fp32_forward_and_backward_bit_for_bit(lib, dev, name, kind):
    """Odd H and W (TF SAME: pad bottom / right only), H = 1, W = 1, one pixel; vector and scalar forward; the first-maximum rule on real ties."""
    s = R.POOL_F32[name]
    n, h, w, c = s['shape']
    lead, ho, wo = s.get('lead', 0), (h + 1) // 2, (w + 1) // 2
    x, dy = R.pool_inputs(s['shape'], kind), R.pool_gradient(s['shape'])
    xb, yb = flat(dev, x, lead), blank(dev, n * ho * wo * c, lead)
    assert lib.kpx_maxpool2_fwd_f32(xb.ptr, n, h, w, c, yb.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert xb.input_ok() and yb.output_ok()
    same('kpx_maxpool2_fwd_f32 %s %s' % (name, kind), yb.get(), R.maxpool2_fwd(x, F32))
    db, dxb = flat(dev, dy, lead), blank(dev, n * h * w * c, lead)
    assert lib.kpx_maxpool2_bwd_f32(db.ptr, xb.ptr, n, h, w, c, dxb.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert xb.input_ok() and db.input_ok() and dxb.output_ok()
    same('kpx_maxpool2_bwd_f32 %s %s' % (name, kind), dxb.get(), R.maxpool2_bwd(dy, x, F32))


@pytest.mark.parametrize('shape', R.POOL_BF16)
def test_maxpool_bf16_forward_bit_for_bit_and_odd_sizes_refused(lib, dev, shape):
    n, h, w, c = shape
    for kind in ('cont', 'ties'):
        x = R.to_bf16(R.pool_inputs(shape, kind))
        xb, yb = flat(dev, x, half=True), blank(dev, n * (h // 2) * (w // 2) * c, half=True)
        assert lib.kpx_maxpool2_fwd_bf16(xb.ptr, n, h, w, c, yb.ptr, stream_of(dev)) == 0
        torch.cuda.synchronize(dev)
        assert xb.input_ok() and yb.output_ok()
        same('kpx_maxpool2_fwd_bf16 %s %s' % (shape, kind), yb.get(), R.maxpool2_fwd(x, F32))
    out = blank(dev, n * h * w * c, half=True)
    odd = flat(dev, np.ones(n * h * w * c), 1, half=True)
    for args, src in (((n, h - 1, w, c), xb), ((n, h, w - 1, c), xb), ((n, h, w, c - 4), xb), ((n, h, w, c), odd)):
        assert lib.kpx_maxpool2_fwd_bf16(src.ptr, *args, out.ptr, stream_of(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert out.untouched()


# ----------------------------------------------------------------------------------------------- VGG feature gradient
def feat_run(lib, dev, shape, kind, pooled, devv, half, lead_d=0):
    b, h, w, c = shape
    gt, pred = R.features(kind, shape, half)
    dyp = R.pooled_gradient(shape, half) if pooled else None
    fb = flat(dev, np.concatenate([gt.ravel(), pred.ravel()]), half=half)
    pb = flat(dev, dyp, half=half) if pooled else None
    gb = flat(dev, [devv]) if devv is not None else None
    db = blank(dev, gt.size, lead_d, half=half)
    fn = lib.kpx_vgg_feat_bwd_bf16 if half else lib.kpx_vgg_feat_bwd_f32
    rc = fn(fb.ptr, gt.size, gb.ptr if gb else None, R.GHOST, pb.ptr if pb else None, b, h, w, c, db.ptr, stream_of(dev))
    torch.cuda.synchronize(dev)
    assert fb.input_ok() and (pb is None or pb.input_ok()) and (gb is None or gb.input_ok())
    return rc, db, R.expect_feat(gt, pred, R.GHOST, devv, dyp, half)


@pytest.mark.parametrize('shape', R.FEAT_F32)
@pytest.mark.parametrize('kind', ['cont', 'ties'])
@pytest.mark.parametrize('pooled', [False, True])
@pytest.mark.parametrize('devv', [None, R.GDEV])
def test_feature_gradient_fp32_bit_for_bit(lib, dev, shape, kind, pooled, devv):
    """Odd and even sizes, one pixel; the first-maximum rule on ties, all-zero windows, gt == pred (l1 exactly 0), pred == 0 (masked);
    g = 0.01 on the host alone and times a device scalar 0.37."""
    rc, db, want = feat_run(lib, dev, shape, kind, pooled, devv, False)
    assert rc == 0 and db.output_ok()
    same('kpx_vgg_feat_bwd_f32 %s %s pooled=%d dev=%s' % (shape, kind, pooled, devv), db.get(), want)


@pytest.mark.parametrize('shape,pooled', [(s, p) for s in R.FEAT_BF16 for p in (False, True)] + [(s, False) for s in R.FEAT_BF16_FLAT])
@pytest.mark.parametrize('kind', ['cont', 'ties'])
@pytest.mark.parametrize('devv', [None, R.GDEV])
def test_feature_gradient_bf16_bit_for_bit(lib, dev, shape, pooled, kind, devv):
    """With the device scalar |l1| = 0.0037 lies below half a bf16 unit of the dy_pooled values in [1, 2): the sum rounds back to dy_pooled."""
    rc, db, want = feat_run(lib, dev, shape, kind, pooled, devv, True)
    assert rc == 0 and db.output_ok()
    same('kpx_vgg_feat_bwd_bf16 %s %s pooled=%d dev=%s' % (shape, kind, pooled, devv), db.get(), want)


def test_feature_gradient_refusals_write_nothing(lib, dev):
    st = stream_of(dev)
    rc, db, _ = feat_run(lib, dev, (2, 4, 6, 6), 'cont', True, None, False)           # C % 4
    assert rc == EINVAL and db.untouched()
    rc, db, _ = feat_run(lib, dev, (2, 4, 6, 8), 'cont', True, None, False, lead_d=1)  # d at a 4-byte offset
    assert rc == EINVAL and db.untouched()
    b, h, w, c = 2, 4, 6, 8
    half = b * h * w * c
    f, p, d = flat(dev, np.ones(2 * half + 8)), flat(dev, np.ones(half // 4)), blank(dev, half + 8)
    assert lib.kpx_vgg_feat_bwd_f32(f.ptr, half + 4, None, R.GHOST, p.ptr, b, h, w, c, d.ptr, st) == EINVAL        # half != B H W C
    assert lib.kpx_vgg_feat_bwd_f32(f.ptr, half - 4, None, R.GHOST, None, b, h, w, c, d.ptr, st) == EINVAL
    f16, p16, d16 = flat(dev, np.ones(2 * 2 * 3 * 5 * 8), half=True), flat(dev, np.ones(2 * 2 * 3 * 8), half=True), blank(dev, 2 * 3 * 5 * 8, half=True)
    assert lib.kpx_vgg_feat_bwd_bf16(f16.ptr, 2 * 3 * 5 * 8, None, R.GHOST, p16.ptr, 2, 3, 5, 8, d16.ptr, st) == EINVAL   # odd sizes with dy_pooled
    assert lib.kpx_vgg_feat_bwd_bf16(f16.ptr, 2 * 3 * 5 * 4, None, R.GHOST, None, 2, 3, 5, 4, d16.ptr, st) == EINVAL      # C % 8
    torch.cuda.synchronize(dev)
    assert d.untouched() and d16.untouched()


# ----------------------------------------------------------------------------------------------- VGG input transform
@pytest.mark.parametrize('P', R.PREP_P)
def test_vgg_prep_forward_bounded_backward_bit_for_bit(lib, dev, P):
    x, d = R.prep_values(P), R.normal('prep_d', (P, 3))
    xb, yb = flat(dev, x), blank(dev, 3 * P)
    assert lib.kpx_vgg_prep_fwd_f32(xb.ptr, P, yb.ptr, stream_of(dev)) == 0
    db, gb = flat(dev, d), blank(dev, 3 * P)
    assert lib.kpx_vgg_prep_bwd_f32(db.ptr, P, gb.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert xb.input_ok() and yb.output_ok() and db.input_ok() and gb.output_ok()
    r = R.worst(yb.get().reshape(P, 3) - R.vgg_prep_fwd(x), R.vgg_prep_fwd_bound(x))
    report('kpx_vgg_prep_fwd_f32 P=%d' % P, r)
    assert r <= 1.0
    same('kpx_vgg_prep_bwd_f32 P=%d' % P, gb.get(), R.vgg_prep_bwd(d, F32))
    none = blank(dev, 3)
    assert lib.kpx_vgg_prep_fwd_f32(None, 1, none.ptr, stream_of(dev)) == EINVAL and lib.kpx_vgg_prep_bwd_f32(None, 1, none.ptr, stream_of(dev)) == EINVAL
    assert lib.kpx_vgg_prep_fwd_f32(xb.ptr, 0, none.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert none.untouched()


# ----------------------------------------------------------------------------------------------- activation backward
@pytest.mark.parametrize('n', R.ACT_N)
@pytest.mark.parametrize('act', [0, 1, 2, 3])
@pytest.mark.parametrize('in_place', [False, True])
def test_act_bwd_fp32(lib, dev, n, act, in_place):
    """The quad loop and its 1-3 element tail; y with +0, -0, +-1e-30, +-1; relu / leaky / none bit for bit (a negative gradient through a dead
    unit is -0), tanh inside its bound.  act 0 in place launches nothing: the buffer is as it was."""
    dy, y = R.act_values(n)
    gb, yb = flat(dev, dy), flat(dev, y)
    zb = gb if in_place else blank(dev, n)
    assert lib.kpx_act_bwd_f32(gb.ptr, yb.ptr, zb.ptr, n, act, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert yb.input_ok() and zb.guards_ok() and (in_place or (gb.input_ok() and zb.output_ok()))
    got = zb.get().ravel()
    if act == R.ACT_TANH:
        r = R.worst(got - R.act_bwd(dy, y, act), R.tanh_bwd_bound(dy, y))
        report('kpx_act_bwd_f32 tanh n=%d in_place=%d' % (n, in_place), r)
        assert r <= 1.0
    else:
        same('kpx_act_bwd_f32 act=%d n=%d in_place=%d' % (act, n, in_place), got, R.expect_act(dy, y, act))


def test_act_bwd_refusals_write_nothing(lib, dev):
    dy, y = R.act_values(16, bf16=True)
    st = stream_of(dev)
    g, v, z = flat(dev, dy), flat(dev, y), blank(dev, 16)
    g1, z1 = flat(dev, dy, 1), blank(dev, 16, 1)
    for act in (-1, 4):
        assert lib.kpx_act_bwd_f32(g.ptr, v.ptr, z.ptr, 16, act, st) == EINVAL
    assert lib.kpx_act_bwd_f32(g1.ptr, v.ptr, z.ptr, 16, 1, st) == EINVAL and lib.kpx_act_bwd_f32(g.ptr, v.ptr, z1.ptr, 16, 1, st) == EINVAL
    gh, vh, zh = flat(dev, dy, half=True), flat(dev, y, half=True), blank(dev, 16, half=True)
    for act in (-1, 3, 4):                                        # the bf16 entry has no tanh backward: refused, not the identity
        assert lib.kpx_act_bwd_bf16(gh.ptr, vh.ptr, zh.ptr, 16, act, st) == EINVAL
    assert lib.kpx_act_bwd_bf16(gh.ptr, vh.ptr, zh.ptr, 12, 1, st) == EINVAL           # n % 8
    zh1 = blank(dev, 16, 1, half=True)
    assert lib.kpx_act_bwd_bf16(gh.ptr, vh.ptr, zh1.ptr, 16, 1, st) == EINVAL
    torch.cuda.synchronize(dev)
    assert z.untouched() and z1.untouched() and zh.untouched() and zh1.untouched() and g.input_ok() and gh.input_ok()


@pytest.mark.parametrize('n', R.ACT_N_BF16)
@pytest.mark.parametrize('act', [0, 1, 2])
def test_act_bwd_bf16_bit_for_bit(lib, dev, n, act):
    dy, y = R.act_values(n, bf16=True)
    for in_place in (False, True):
        gb, yb = flat(dev, dy, half=True), flat(dev, y, half=True)
        zb = gb if in_place else blank(dev, n, half=True)
        assert lib.kpx_act_bwd_bf16(gb.ptr, yb.ptr, zb.ptr, n, act, stream_of(dev)) == 0
        torch.cuda.synchronize(dev)
        assert yb.input_ok() and zb.guards_ok() and (in_place or (gb.input_ok() and zb.output_ok()))
        same('kpx_act_bwd_bf16 act=%d n=%d in_place=%d' % (act, n, in_place), zb.get(), R.expect_act(dy, y, act, True))


# ----------------------------------------------------------------------------------------------- casts and copies
def cast_run(lib, dev, kind, P, C, lds, ldd, lead=0):
    src_half, dst_half = kind in (1, 2), kind != 1
    x = R.cast_values(P, C, bf16_exact=src_half, nan=not src_half)
    sb, ob = SBuf(dev, P, C, lds, lead, x, src_half), SBuf(dev, P, 8 if kind == 3 else C, ldd, lead, half=dst_half)
    assert lib.kpx_cast_channels(sb.ptr, lds, ob.ptr, ldd, P, C, kind, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert ob.output_ok() and sb.guards_ok()
    keep = ~np.isnan(x)
    assert np.array_equal(sb.get()[keep].view(np.uint32), x[keep].view(np.uint32)), 'an input was written'
    same('kpx_cast_channels kind=%d P=%d C=%d ld=%d,%d lead=%d' % (kind, P, C, lds, ldd, lead), ob.get(), R.cast(x, kind))
    return x, ob


@pytest.mark.parametrize('kind', [0, 1, 2])
@pytest.mark.parametrize('geom', [R.CAST_VEC + (0,), R.CAST_SCALAR + (0,), (37, 8, 8, 8, 1)])
def test_cast_channels_bit_for_bit(lib, dev, kind, geom):
    """Octet path (ld > C on the source), scalar path by C % 8 with odd strides, and C = 8 from a 4-byte-offset base; the fp32 sources carry
    the half-way values of both parities, the neighbours of the largest bf16, +-inf, +-0 and a NaN (which stays one)."""
    x, ob = cast_run(lib, dev, kind, *geom)
    if kind == 0:
        k = min(R.HALFWAY.size, x.size - 1)
        assert np.array_equal(R.bf16_bits(ob.get().ravel()[:k]), R.HALFWAY_BF16[:k]) and np.isnan(ob.get().ravel()[-1])


@pytest.mark.parametrize('C', R.CAST_PAD_C)
def test_cast_pad8_bit_for_bit_and_refusals(lib, dev, C):
    x, ob = cast_run(lib, dev, 3, 37, C, C + 3, 8)
    assert np.all(ob.get()[:, C:].view(np.uint32) == 0), 'channels C .. 7 must be +0'
    sb, bad = SBuf(dev, 37, 9, 12, 0, np.ones((37, 9))), SBuf(dev, 37, 16, 16, half=True)
    st = stream_of(dev)
    assert lib.kpx_cast_channels(sb.ptr, 12, bad.ptr, 8, 37, 9, 3, st) == EINVAL          # C = 9
    assert lib.kpx_cast_channels(sb.ptr, 12, bad.ptr, 16, 37, C, 3, st) == EINVAL         # lddst != 8
    assert lib.kpx_cast_channels(sb.ptr, 12, bad.ptr, 16, 37, 8, 4, st) == EINVAL and lib.kpx_cast_channels(sb.ptr, 4, bad.ptr, 16, 37, 8, 0, st) == EINVAL
    torch.cuda.synchronize(dev)
    assert bad.untouched()


@pytest.mark.parametrize('name', list(R.COPY))
def test_copy_channels_bit_for_bit(lib, dev, name):
    P, C, lds, ldd = R.COPY[name]
    x = R.cast_values(P, C, nan=True)
    sb, ob = SBuf(dev, P, C, lds, 0, x), SBuf(dev, P, C, ldd)
    assert lib.kpx_copy_channels_f32(sb.ptr, lds, ob.ptr, ldd, P, C, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert ob.output_ok() and sb.guards_ok()
    same('kpx_copy_channels_f32 %s' % name, ob.get(), x)
    none = SBuf(dev, P, C, ldd)
    assert lib.kpx_copy_channels_f32(sb.ptr, C - 1, none.ptr, ldd, P, C, stream_of(dev)) == EINVAL
    assert lib.kpx_copy_channels_f32(sb.ptr, lds, none.ptr, C - 1, P, C, stream_of(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert none.untouched()


# ----------------------------------------------------------------------------------------------- axpy, fill
@pytest.mark.parametrize('n', R.AXPY_N)
@pytest.mark.parametrize('a', R.AXPY_A)
def test_axpy_against_float64(lib, dev, n, a):
    y, x = R.normal('axpy_y', (n,)), R.normal('axpy_x', (n,))
    yb, xb = flat(dev, y), flat(dev, x)
    assert lib.kpx_axpy_f32(yb.ptr, xb.ptr, n, a, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert xb.input_ok() and yb.guards_ok()
    r = R.worst(yb.get().ravel() - R.axpy(y, x, a), R.axpy_bound(y, x, a))
    report('kpx_axpy_f32 n=%d a=%g' % (n, a), r)
    assert r <= 1.0


@pytest.mark.parametrize('n', R.FILL_N)
def test_fill_bit_for_bit(lib, dev, n):
    ob = blank(dev, max(n, 1))
    assert lib.kpx_fill_f32(ob.ptr, n, -2.5, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    if n == 0:
        assert ob.untouched()                                     # nothing launched
        assert lib.kpx_fill_f32(None, 4, 1.0, stream_of(dev)) == EINVAL
    else:
        assert ob.output_ok()
        same('kpx_fill_f32 n=%d' % n, ob.get(), np.full(n, -2.5, F32))


# ----------------------------------------------------------------------------------------------- capped grids: the second sweep
def on_device(dev, a, half=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev)
    return t.bfloat16() if half else t


def big_same(entry, out, want):
    got = out.view[:want.size].float().cpu().numpy()
    same(entry, got, want)


def test_fill_second_sweep(lib, dev):
    out = Big(dev, R.CAP_FILL)
    assert lib.kpx_fill_f32(out.ptr, R.CAP_FILL, 1.5, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert out.output_ok()
    n = int((out.view != 1.5).sum())
    print('differing kpx_fill_f32 second sweep %d' % n)
    assert n == 0


def test_resize_backward_second_sweep(lib, dev):
    """723 x 726 quads = 2048 x 256 + 610: the vector kernel's grid-stride loop makes a second, ragged trip."""
    h, w = R.CAP_HW
    dy = R.resize_gradient((1, h, w, 4))
    src, out = on_device(dev, dy), Big(dev, h * w * 4)
    assert lib.kpx_resize2x_bwd_f32(src.data_ptr(), 1, h, w, 4, 4, out.ptr, 4, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert out.output_ok() and torch.equal(src, on_device(dev, dy))
    big_same('kpx_resize2x_bwd_f32 second sweep', out, R.expect_resize_bwd(dy))


def test_maxpool_forward_second_sweep(lib, dev):
    h, w = 2 * R.CAP_HW[0] - 1, 2 * R.CAP_HW[1]
    x = R.normal('pool_big', (1, h, w, 4))
    src, out = on_device(dev, x), Big(dev, R.CAP_HW[0] * R.CAP_HW[1] * 4)
    assert lib.kpx_maxpool2_fwd_f32(src.data_ptr(), 1, h, w, 4, out.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert out.output_ok() and torch.equal(src, on_device(dev, x))
    big_same('kpx_maxpool2_fwd_f32 second sweep', out, R.maxpool2_fwd(x, F32))


def test_feature_gradient_second_sweep(lib, dev):
    shape = (1, 2 * R.CAP_HW[0] - 1, 2 * R.CAP_HW[1], 4)
    gt, pred = R.features('cont', shape)
    dyp = R.pooled_gradient(shape)
    f, p, g = on_device(dev, np.concatenate([gt.ravel(), pred.ravel()])), on_device(dev, dyp), on_device(dev, [R.GDEV])
    out = Big(dev, gt.size)
    assert lib.kpx_vgg_feat_bwd_f32(f.data_ptr(), gt.size, g.data_ptr(), R.GHOST, p.data_ptr(), *shape, out.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert out.output_ok() and torch.equal(p, on_device(dev, dyp))
    big_same('kpx_vgg_feat_bwd_f32 second sweep', out, R.expect_feat(gt, pred, R.GHOST, R.GDEV, dyp))


def test_cast_second_sweep(lib, dev):
    P = R.SWEEP + 77
    x = R.normal('cast_big', (P, 8)) * F32(3)
    src, out = on_device(dev, x), Big(dev, P * 4, half=True)
    assert lib.kpx_cast_channels(src.data_ptr(), 8, out.ptr, 8, P, 8, 0, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert out.output_ok() and torch.equal(src, on_device(dev, x))
    big_same('kpx_cast_channels kind=0 second sweep', out, R.to_bf16(x))


@pytest.mark.parametrize('half', [False, True])
def test_resize_forward_second_sweep(lib, dev, half):
    """2047 x 2051 input pixels of one quad (fp32) or one octet (bf16) = 16384 x 256 + 4093 items: the input-pixel kernels' second sweep, into
    about 270 MB of output.  Every element must be written; the rows of the last sweep (input rows 2045, 2046) and of the first block (input
    row 0) are compared with the restatement bit for bit."""
    h, w = R.CAP_FWD_HW
    c = 8 if half else 4
    gen = torch.Generator(device=dev)
    gen.manual_seed(2047)
    x = torch.randn((1, h, w, c), generator=gen, device=dev)
    x = x.bfloat16() if half else x
    keep = x.clone()
    out = Big(dev, 4 * h * w * c // (2 if half else 1), half)
    fn = lib.kpx_resize2x_fwd_bf16 if half else lib.kpx_resize2x_fwd_f32
    assert fn(x.data_ptr(), 1, h, w, c, c, out.ptr, c, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert out.output_ok() and torch.equal(x.view(torch.int16 if half else torch.int32), keep.view(torch.int16 if half else torch.int32))
    y = out.view[:4 * h * w * c].view(1, 2 * h, 2 * w, c)
    first = R.SWEEP_FWD // w                                     # the input row in which the second sweep begins
    assert first == h - 2
    tail = x[:, first:].float().cpu().numpy()
    same('kpx_resize2x_fwd_%s last sweep' % ('bf16' if half else 'f32'), y[:, 2 * first:].float().cpu().numpy(), R.expect_resize_fwd(tail, half))
    head = x[:, :2].float().cpu().numpy()
    same('kpx_resize2x_fwd_%s first block' % ('bf16' if half else 'f32'), y[:, :2].float().cpu().numpy(), R.expect_resize_fwd(head, half)[:, :2])


# ----------------------------------------------------------------------------------------------- graph replay
def test_graph_replay_equals_the_eager_launches(lib, dev):
    """A resize forward / backward pair and a pooled feature gradient captured once and replayed twice: the bits of the eager launches."""
    s = R.RESIZE_F32['quad_2x5x7x16_ldy24']
    n, h, w, c, ldx, ldy, _ = geometry(s)
    x, dy = R.resize_input(s['shape']), R.resize_gradient(s['shape'])
    shape = R.FEAT_F32[0]
    gt, pred = R.features('ties', shape)
    dyp = R.pooled_gradient(shape)
    xb, db = SBuf(dev, n * h * w, c, ldx, 0, x.reshape(-1, c)), SBuf(dev, 4 * n * h * w, c, ldy, 0, dy.reshape(-1, c))
    fb, pb, gb = flat(dev, np.concatenate([gt.ravel(), pred.ravel()])), flat(dev, dyp), flat(dev, [R.GDEV])
    outs = [SBuf(dev, 4 * n * h * w, c, ldy), SBuf(dev, n * h * w, c, ldx), blank(dev, gt.size)]
    codes = []

    def enqueue():
        st = stream_of(dev)
        codes.append(lib.kpx_resize2x_fwd_f32(xb.ptr, n, h, w, c, ldx, outs[0].ptr, ldy, st))
        codes.append(lib.kpx_resize2x_bwd_f32(db.ptr, n, h, w, c, ldy, outs[1].ptr, ldx, st))
        codes.append(lib.kpx_vgg_feat_bwd_f32(fb.ptr, gt.size, gb.ptr, R.GHOST, pb.ptr, *shape, outs[2].ptr, st))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()                                               # the eager launches (and the warm-up of the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize(dev)
    eager = [o.get().copy() for o in outs]
    want = [R.expect_resize_fwd(x), R.expect_resize_bwd(dy), R.expect_feat(gt, pred, R.GHOST, R.GDEV, dyp)]
    for e, wnt in zip(eager, want):
        assert R.differing(e, wnt.reshape(e.shape)) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    assert codes == [0] * 6
    for _ in range(2):
        for o in outs:
            o.buf.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize(dev)
        for i, (o, e) in enumerate(zip(outs, eager)):
            assert o.output_ok()
            same('graph replay output %d' % i, o.get(), e)
    assert xb.input_ok() and db.input_ok() and fb.input_ok() and pb.input_ok() and gb.input_ok()
