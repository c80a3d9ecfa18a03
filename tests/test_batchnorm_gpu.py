"""The batch-norm entries of csrc/pointwise.hip and the channel sums they share against float64 on every launch path: kpx_bn_train_{fwd,bwd}_f32
and _bf16 with and without ``tile_stats``, kpx_bn_apply_f32, kpx_bn_invstd_f32, kpx_bn_fold_conv_f32, kpx_chan_sum_{f32,bf16}.  Restatements,
seeded inputs and bounds live in tests/batchnorm_ref.py (its header lists every bound); tests/test_batchnorm_cpu.py derives the restatements
a second time, holds a sequential-fp32 evaluation to the same bounds and shows that the bounds reject the planted slips.

Everything runs through the C ABI.  Every buffer an entry writes has 8 sentinel words after it (and before it where a lead is used); a
strided output also keeps its gap channels between C and ld; the scratch is sized exactly by the *_scratch_bytes queries, with sentinels
behind it.  Inputs must keep their bits (their gap channels hold NaN: a kernel that reads one shows), every output element must be
written, a refused call must write nothing.  Each stage is judged on the state the entry itself saved.  Each test prints
``ratio <entry> <worst error/bound>``."""
import numpy as np
import pytest
import torch

import batchnorm_ref as R
from test_keypoints_gpu import EINVAL, GUARD, SENTINEL, report, stream_of

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
HALVES = np.array([SENTINEL & 0xffff, SENTINEL >> 16], dtype=np.uint16).view(np.int16)   # a sentinel word as two bf16 slots (little endian)


@pytest.fixture(scope='module')
def lib():
    from kpx_amd import _lib
    return _lib.lib


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


class Buf:
    """rows x C elements (fp32, or bf16 with ``half``) at leading dimension ld, ``lead`` words into a buffer of sentinel words that ends
    right behind the last element.  With ``data`` the gap channels hold NaN; without, every slot starts as a sentinel."""

    def __init__(self, dev, rows, C, ld, lead=0, data=None, half=False):
        n = (rows - 1) * ld + C
        assert not half or n % 2 == 0
        self.half, self.lead, self.words, self.shape = half, lead, n // 2 if half else n, (rows, C)
        self.buf = torch.full((lead + self.words + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        inner = self.buf[lead:lead + self.words]
        self.view = inner.view(torch.bfloat16) if half else inner.view(torch.float32)
        assert self.view.numel() == n and self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() == self.buf.data_ptr() + 4 * lead
        self.idx = (np.arange(rows)[:, None] * ld + np.arange(C)[None, :]).ravel()
        self.gap = np.ones(n, bool)
        self.gap[self.idx] = False
        self.pattern = HALVES[np.arange(n) % 2] if half else np.full(n, SENTINEL, np.int32)
        self.data = None
        if data is not None:
            self.data = np.ascontiguousarray(data, dtype=F32).reshape(rows, C)
            full = np.full(n, np.nan, F32)
            full[self.idx] = self.data.ravel()
            self.view.copy_(torch.from_numpy(full))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def raw(self):
        inner = self.buf[self.lead:self.lead + self.words]
        return (inner.view(torch.int16) if self.half else inner).cpu().numpy()

    def get(self):
        return self.view.float().cpu().numpy()[self.idx].reshape(self.shape)

    def guards_ok(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.lead] == SENTINEL) and np.all(b[self.lead + self.words:] == SENTINEL))

    def output_ok(self):
        """Guards and gap channels untouched, every element written."""
        r = self.raw()
        assert self.guards_ok(), 'a guard word was overwritten'
        assert np.all(r[self.gap] == self.pattern[self.gap]), 'a gap channel between C and ld was written'
        fresh = r[self.idx] != self.pattern[self.idx]
        if self.half:                                # -450 is the low half of a sentinel word; the high half is a NaN no kernel here stores
            fresh = fresh.reshape(-1, 2).any(axis=1)
        assert np.all(fresh), 'an output element was never written'
        return True

    def input_ok(self):
        got = self.get()
        assert self.guards_ok() and np.array_equal(got.view(np.uint32), self.data.view(np.uint32)), 'an input was written'
        return True

    def untouched(self):
        return bool(np.all(self.buf.cpu().numpy() == SENTINEL))


def vec(dev, data):
    data = np.asarray(data, F32).ravel()
    return Buf(dev, 1, data.size, data.size, data=data)


def blank(dev, n):
    return Buf(dev, 1, n, n)


def train_scratch(lib, dev, C, groups):
    nbytes = lib.kpx_bn_train_scratch_bytes(C, groups)
    assert nbytes == groups * (1024 * 2 * C * 8 + ((2 * C * 4 + 15) & ~15)) and nbytes == groups * lib.kpx_chan_reduce_scratch_bytes(C)
    return blank(dev, nbytes // 4)


def ptr(b):
    return None if b is None else b.ptr


class Run:
    """One case on guarded buffers: forward(), then backward() on the forward's own saved mean / invstd."""

    def __init__(self, lib, dev, c, kind='f32', y_f32=0, dy_f32=0, moving=True):
        self.lib, self.dev, self.c, self.half, self.y_f32, self.dy_f32 = lib, dev, c, kind == 'bf16', y_f32, dy_f32
        self.groups, self.P, self.C, self.ldx = c['shape']
        self.ldo, self.lead, self.dy_lead = c.get('ldo', self.ldx), c.get('lead', 0), c.get('lead', 0) + c.get('dy_lead', 0)
        rows = self.groups * self.P
        self.x = Buf(dev, rows, self.C, self.ldx, self.lead, c['x'].reshape(rows, self.C), self.half)
        self.gamma, self.beta = vec(dev, c['gamma']), vec(dev, c['beta'])
        self.mean, self.invstd = blank(dev, self.groups * self.C), blank(dev, self.groups * self.C)
        self.mm, self.mv = (vec(dev, c['mm0']), vec(dev, c['mv0'])) if moving else (None, None)
        self.sc = train_scratch(lib, dev, self.C, self.groups)
        self.y = Buf(dev, rows, self.C, self.ldo, self.lead, half=self.half and not y_f32)
        self.dy = Buf(dev, rows, self.C, self.ldo, self.dy_lead, c['dy'].reshape(rows, self.C), self.half and not dy_f32)
        self.dx = Buf(dev, rows, self.C, self.ldo, self.lead, half=self.half)
        self.dgamma, self.dbeta = vec(dev, c['pre_dgamma']), vec(dev, c['pre_dbeta'])

    def enqueue_fwd(self, act, ts=None, tpg=0):
        a = (self.x.ptr, self.P, self.groups, self.C, self.ldx, ptr(ts), tpg, R.EPS, self.gamma.ptr, self.beta.ptr, self.mean.ptr, self.invstd.ptr,
             ptr(self.mm), ptr(self.mv), R.DECAY, self.y.ptr, self.ldo)
        tail = (act, self.sc.ptr, stream_of(self.dev))
        if self.half:
            return self.lib.kpx_bn_train_fwd_bf16(*a, self.y_f32, *tail)
        return self.lib.kpx_bn_train_fwd_f32(*a, *tail)

    def enqueue_bwd(self, act, accumulate, ts=None, tpg=0):
        head = (self.dy.ptr, self.ldo) + ((self.dy_f32,) if self.half else ())
        a = (self.x.ptr, self.ldx, self.P, self.groups, self.C, self.mean.ptr, self.invstd.ptr, self.gamma.ptr, self.beta.ptr, act,
             self.dx.ptr, self.ldo, self.dgamma.ptr, self.dbeta.ptr, accumulate, ptr(ts), tpg, self.sc.ptr, stream_of(self.dev))
        return (self.lib.kpx_bn_train_bwd_bf16 if self.half else self.lib.kpx_bn_train_bwd_f32)(*head, *a)

    def forward(self, act, ts=None, tpg=0):
        assert self.enqueue_fwd(act, ts, tpg) == 0
        torch.cuda.synchronize(self.dev)
        assert self.x.input_ok() and self.gamma.input_ok() and self.beta.input_ok() and (ts is None or ts.input_ok())
        assert self.y.output_ok() and self.mean.output_ok() and self.invstd.output_ok() and self.sc.guards_ok()
        assert self.mm is None or (self.mm.guards_ok() and self.mv.guards_ok())
        shape = (self.groups, self.P, self.C)
        out = dict(mean=self.mean.get().reshape(self.groups, self.C), invstd=self.invstd.get().reshape(self.groups, self.C), y=self.y.get().reshape(shape))
        if self.mm is not None:
            out['mm'], out['mv'] = self.mm.get()[0], self.mv.get()[0]
        assert all(np.all(np.isfinite(v)) for v in out.values()), 'NaN or infinity'
        return out

    def backward(self, act, accumulate, ts=None, tpg=0):
        self.mean.data, self.invstd.data = self.mean.get(), self.invstd.get()       # the saved state is an input now
        assert self.enqueue_bwd(act, accumulate, ts, tpg) == 0
        torch.cuda.synchronize(self.dev)
        assert all(b.input_ok() for b in (self.x, self.dy, self.gamma, self.beta, self.mean, self.invstd)) and (ts is None or ts.input_ok())
        assert self.dx.output_ok() and self.dgamma.guards_ok() and self.dbeta.guards_ok() and self.sc.guards_ok()
        out = dict(dx=self.dx.get().reshape(self.groups, self.P, self.C), dgamma=self.dgamma.get()[0], dbeta=self.dbeta.get()[0])
        assert all(np.all(np.isfinite(v)) for v in out.values()), 'NaN or infinity'
        return out


def check_pair(lib, dev, c, label, act, accumulate, kind='f32', y_f32=0, dy_f32=0):
    """Forward and backward of one case against float64; the ReLU condition again on the saved state; the exact edges."""
    run = Run(lib, dev, c, kind, y_f32, dy_f32)
    half = kind == 'bf16'
    fwd = run.forward(act)
    assert not R.undecided(c['x'], fwd['mean'], fwd['invstd'], c['gamma'], c['beta']).any(), 'an element is undecided on the saved state'
    rf = R.forward_ratios(c, fwd, act, bf16_y=half)
    bwd = run.backward(act, accumulate)
    rb = R.backward_ratios(c, fwd['mean'], fwd['invstd'], bwd, act, accumulate, bf16_dx=half)
    suffix = '_bf16' if half else '_f32'
    report('kpx_bn_train_fwd%s %s act=%d %s' % (suffix, label, act, {k: round(v, 4) for k, v in rf.items()}), max(rf.values()))
    report('kpx_bn_train_bwd%s %s act=%d acc=%d %s' % (suffix, label, act, accumulate, {k: round(v, 4) for k, v in rb.items()}), max(rb.values()))
    assert max(rf.values()) <= 1.0, rf
    assert max(rb.values()) <= 1.0, rb
    ga, be = np.asarray(c['gamma']), np.asarray(c['beta'])
    const = [i for i, r in enumerate(c['regimes']) if r == 'constant'] if c['shape'][1] > 1 else list(range(c['shape'][2]))
    if const:                                        # a constant channel (every channel at P = 1): exact
        want = np.maximum(be[const], 0) if act else be[const]
        assert np.all(fwd['invstd'][:, const] == F32(1) / np.sqrt(F32(R.EPS), dtype=F32))
        if not half or y_f32:
            assert np.all(fwd['y'][:, :, const] == want), 'y != beta on a constant channel'
        if c['shape'][1] == 1:
            assert np.array_equal(fwd['mean'][0], c['x'][0, 0])
    if act:
        dead = (ga == 0) & (be == 0)
        assert np.all(bwd['dx'][:, :, ga == 0] == 0), 'gamma = 0 must give dx = 0 exactly'
        if dead.any() and not accumulate:
            assert np.all(bwd['dgamma'][dead] == 0) and np.all(bwd['dbeta'][dead] == 0)
    return run, fwd, bwd


SMALL = [n for n, s in R.CASES.items() if not s.get('big') and not n.startswith('g')]
GROUPS = [n for n in R.CASES if n.startswith('g')]


@pytest.mark.parametrize('name', SMALL)
@pytest.mark.parametrize('act', [1, 0])
def test_train_forward_and_backward_against_float64(lib, dev, name, act):
    """The vector and scalar paths of batchnorm_ref.CASES (the branch of each is noted there), ReLU and act = 0."""
    check_pair(lib, dev, R.case(name), name, act, accumulate=0)


@pytest.mark.parametrize('name', [n for n, s in R.CASES.items() if s.get('big')])
def test_train_at_the_block_caps(lib, dev, name):
    """8229 pixels: the reduction grid is capped at 1024 blocks, the strip grid (vector) and the element grid (scalar) at 2048; every loop
    makes a second, ragged trip."""
    check_pair(lib, dev, R.case(name), name, 1, accumulate=0)


@pytest.mark.parametrize('name', GROUPS)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_groups_moving_statistics_and_accumulate(lib, dev, name, accumulate):
    """4, 5, 6 groups: the finalize kernels make a second trip (5, 6: partly idle); every group against float64, the moving statistics
    after the in-order updates, dgamma / dbeta over pre-filled values with accumulate = 0 (replaced) and 1 (added to)."""
    c = R.case(name)
    run, fwd, bwd = check_pair(lib, dev, c, name, 1, accumulate)
    # a group's results do not depend on the groups beside it: group g alone gives the same bits
    g = c['shape'][0] - 1
    solo = dict(c, shape=(1,) + tuple(c['shape'][1:]), x=c['x'][g:g + 1], dy=c['dy'][g:g + 1])
    one = Run(lib, dev, solo)
    f1 = one.forward(1)
    b1 = one.backward(1, 0)
    assert np.array_equal(f1['y'].view(np.uint32), fwd['y'][g:g + 1].view(np.uint32)) and np.array_equal(f1['mean'][0], fwd['mean'][g])
    assert np.array_equal(b1['dx'].view(np.uint32), bwd['dx'][g:g + 1].view(np.uint32))


def test_forward_without_moving_statistics(lib, dev):
    c = R.case('g5x12')
    run = Run(lib, dev, c, moving=False)
    fwd = run.forward(0)
    r = R.forward_ratios(c, fwd, 0, with_moving=False)
    report('kpx_bn_train_fwd_f32 no moving statistics', max(r.values()))
    assert max(r.values()) <= 1.0, r


# ----------------------------------------------------------------------------------------------- tile_stats
@pytest.mark.parametrize('items', R.TILE_ITEMS)
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_tile_stats_forward_and_backward(lib, dev, items, kind):
    """Per-item sums in place of the reduction pass: 1 item, 255 / 256 / 257 (one thread's second trip) and 600 items per group, two groups;
    backward under ReLU with sum dz (y - beta) divided by gamma and two channels at gamma = 0."""
    half = kind == 'bf16'
    c = R.tile_case(items, bf16=half)
    groups, n, C = c['shape'][:3]
    run = Run(lib, dev, c, kind)
    ts = Buf(dev, groups * items * 2, C, C, data=c['ts_fwd'].reshape(-1, C))
    fwd = run.forward(1, ts, items)
    assert not R.undecided(c['x'], fwd['mean'], fwd['invstd'], c['gamma'], c['beta']).any()
    rf = R.forward_ratios(c, fwd, 1, ts=c['ts_fwd'], bf16_y=half)
    dz, xh = R.bn_dz(c['dy'], c['x'], fwd['mean'], fwd['invstd'], c['gamma'], c['beta'], 1)
    slab = R.tile_stats_bwd(dz, xh * np.asarray(c['gamma'], F64), c['cuts'])
    tb = Buf(dev, groups * items * 2, C, C, data=slab.reshape(-1, C))
    bwd = run.backward(1, 1, tb, items)
    rb = R.backward_ratios(c, fwd['mean'], fwd['invstd'], bwd, 1, 1, ts=slab, bf16_dx=half)
    report('kpx_bn_train_fwd_%s tile_stats items=%d %s' % (kind, items, {k: round(v, 4) for k, v in rf.items()}), max(rf.values()))
    report('kpx_bn_train_bwd_%s tile_stats items=%d %s' % (kind, items, {k: round(v, 4) for k, v in rb.items()}), max(rb.values()))
    assert max(rf.values()) <= 1.0, rf
    assert max(rb.values()) <= 1.0, rb
    dead = np.asarray(c['gamma']) == 0
    assert dead.sum() == 2 and np.all(bwd['dx'][:, :, dead] == 0)
    assert np.array_equal(bwd['dgamma'][dead], np.asarray(c['pre_dgamma'])[dead]), 'gamma = 0: the slab form adds exactly 0 to dgamma'


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_tile_stats_backward_refusals_write_nothing(lib, dev, kind):
    c = R.tile_case(1, bf16=kind == 'bf16')
    run = Run(lib, dev, c, kind)
    run.forward(1)
    ts = Buf(dev, 2 * 2, 16, 16, data=np.ones((4, 16), F32))
    pre = [run.dgamma.get().copy(), run.dbeta.get().copy()]
    assert run.enqueue_bwd(0, 0, ts, 1) == EINVAL               # act = 0: the slab form needs ReLU
    assert run.enqueue_bwd(1, 0, ts, 0) == EINVAL               # tiles_per_group = 0
    torch.cuda.synchronize(dev)
    assert run.dx.untouched() and np.array_equal(run.dgamma.get(), pre[0]) and np.array_equal(run.dbeta.get(), pre[1])


# ----------------------------------------------------------------------------------------------- bf16 entries
@pytest.mark.parametrize('name', list(R.CASES_BF16))
@pytest.mark.parametrize('y_f32,dy_f32', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_bf16_entries_against_float64(lib, dev, name, y_f32, dy_f32):
    """C = 8, 24, 2056 (second blockIdx.y slice), 16 with five groups; bf16 and fp32 outputs / gradients; ld > C in multiples of 8."""
    c = R.case(name, bf16=True, bf16_dy=not dy_f32)
    for act in (1, 0):
        check_pair(lib, dev, c, name, act, 0, kind='bf16', y_f32=y_f32, dy_f32=dy_f32)


def test_bf16_refusals_write_nothing(lib, dev):
    base = R.case('b_21x24_ld40', bf16=True)
    for change in (dict(shape=(2, 21, 20, 40)), dict(shape=(2, 21, 24, 36)), dict(ldo=36), dict(lead=1)):       # C % 8, ldx % 8, ldy % 8, 4-byte offset
        c = dict(base, **change)
        if c['shape'][2] != 24:
            c.update(x=base['x'][:, :, :20], dy=base['dy'][:, :, :20], gamma=base['gamma'][:20], beta=base['beta'][:20],
                     pre_dgamma=base['pre_dgamma'][:20], pre_dbeta=base['pre_dbeta'][:20], mm0=base['mm0'][:20], mv0=base['mv0'][:20])
        run = Run(lib, dev, c, 'bf16')
        assert run.enqueue_fwd(1) == EINVAL
        run.mean.view.fill_(0.0)
        run.invstd.view.fill_(1.0)
        assert run.enqueue_bwd(1, 0) == EINVAL
        torch.cuda.synchronize(dev)
        assert run.y.untouched() and run.dx.untouched() and run.sc.untouched() and run.mm.input_ok() and run.dgamma.input_ok()
        x = Buf(dev, 42, c['shape'][2], c['shape'][3], c.get('lead', 0), c['x'].reshape(42, -1), half=True)
        out, sc = blank(dev, c['shape'][2]), blank(dev, lib.kpx_chan_reduce_scratch_bytes(c['shape'][2]) // 4)
        if change != dict(ldo=36):
            assert lib.kpx_chan_sum_bf16(x.ptr, 42, c['shape'][2], c['shape'][3], out.ptr, sc.ptr, stream_of(dev)) == EINVAL
            torch.cuda.synchronize(dev)
            assert out.untouched() and sc.untouched()


# ----------------------------------------------------------------------------------------------- the small entries
@pytest.mark.parametrize('name', ['v_37x32', 'v_5x1028', 'v_19x64_ld96', 's_7x5', 's_3x257', 's_11x32_ld33', 's_11x32_lead', 'v_big', 's_big'])
def test_chan_sum_f32_against_float64(lib, dev, name):
    c = R.case(name)
    groups, n, C, ld = c['shape']
    rows = groups * n
    x2 = c['x'].reshape(rows, C)
    x = Buf(dev, rows, C, ld, c.get('lead', 0), x2)
    nbytes = lib.kpx_chan_reduce_scratch_bytes(C)
    assert nbytes == 1024 * 2 * C * 8 + ((2 * C * 4 + 15) & ~15)
    out, sc = blank(dev, C), blank(dev, nbytes // 4)
    assert lib.kpx_chan_sum_f32(x.ptr, rows, C, ld, out.ptr, sc.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert x.input_ok() and out.output_ok() and sc.guards_ok()
    r = R.worst(out.get()[0] - R.chan_sum(x2), R.chan_sum_bound(x2))
    report('kpx_chan_sum_f32 %s' % name, r)
    assert r <= 1.0
    assert lib.kpx_chan_sum_f32(x.ptr, rows, C, C - 1, out.ptr, sc.ptr, stream_of(dev)) == EINVAL


@pytest.mark.parametrize('name', list(R.CASES_BF16))
def test_chan_sum_bf16_against_float64(lib, dev, name):
    c = R.case(name, bf16=True)
    groups, n, C, ld = c['shape']
    rows = groups * n
    x2 = c['x'].reshape(rows, C)
    x = Buf(dev, rows, C, ld, 0, x2, half=True)
    out, sc = blank(dev, C), blank(dev, lib.kpx_chan_reduce_scratch_bytes(C) // 4)
    assert lib.kpx_chan_sum_bf16(x.ptr, rows, C, ld, out.ptr, sc.ptr, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert x.input_ok() and out.output_ok() and sc.guards_ok()
    r = R.worst(out.get()[0] - R.chan_sum(x2), R.chan_sum_bound(x2))
    report('kpx_chan_sum_bf16 %s' % name, r)
    assert r <= 1.0


@pytest.mark.parametrize('name', ['v_37x32', 'v_5x1028', 'v_19x64_ld96', 's_7x5', 's_11x32_ld33', 's_11x32_lead', 'v_big', 's_big'])
@pytest.mark.parametrize('act', [0, 1])
def test_bn_apply_f32_against_float64(lib, dev, name, act):
    """The inference pass on given statistics (the float64 batch statistics rounded to fp32), strip and scalar kernels, both capped grids."""
    c = R.case(name)
    _, rows, C, ld = c['shape']
    ldo, lead = c.get('ldo', ld), c.get('lead', 0)
    xs = c['x'][:1]                                              # the first group, on its float64 batch statistics rounded to fp32
    m, _, inv = R.bn_stats(xs)
    m, inv = m.astype(F32), inv.astype(F32)
    assert not R.undecided(xs, m, inv, c['gamma'], c['beta']).any()
    x, y = Buf(dev, rows, C, ld, lead, xs[0]), Buf(dev, rows, C, ldo, lead)
    ins = [vec(dev, a) for a in (m, inv, c['gamma'], c['beta'])]
    assert lib.kpx_bn_apply_f32(x.ptr, rows, C, ld, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, y.ptr, ldo, act, stream_of(dev)) == 0
    torch.cuda.synchronize(dev)
    assert x.input_ok() and all(i.input_ok() for i in ins) and y.output_ok()
    r = R.worst(y.get() - R.bn_y(xs, m, inv, c['gamma'], c['beta'], act)[0], R.y_bound(xs, m, inv, c['gamma'], c['beta'])[0])
    report('kpx_bn_apply_f32 %s act=%d' % (name, act), r)
    assert r <= 1.0
    y2 = Buf(dev, rows, C, ldo, lead)
    assert lib.kpx_bn_apply_f32(x.ptr, rows, C, ld, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, y2.ptr, ldo, 2, stream_of(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert y2.untouched()


def test_bn_invstd_f32_against_float64(lib, dev):
    rng = np.random.default_rng(11)
    for C in (1, 63, 64, 65, 1028):
        var = np.concatenate((rng.uniform(0, 2, C), [0.0, 1e-30, 1e30]))[-C:].astype(F32)
        v, out = vec(dev, var), blank(dev, C)
        assert lib.kpx_bn_invstd_f32(v.ptr, C, R.EPS, out.ptr, stream_of(dev)) == 0
        torch.cuda.synchronize(dev)
        assert v.input_ok() and out.output_ok()
        r = R.worst(out.get()[0] - R.bn_invstd(var), R.invstd_bound(var))
        report('kpx_bn_invstd_f32 C=%d' % C, r)
        assert r <= 1.0


@pytest.mark.parametrize('rows,C', [(37, 63), (9, 5), (2049, 257), (1, 1)])
@pytest.mark.parametrize('bias', [True, False])
def test_bn_fold_conv_f32_against_float64(lib, dev, rows, C, bias):
    """rows * C is no multiple of 256 (2049 x 257 = 526 593 elements: 2057 blocks -> the capped grid strides)."""
    rng = np.random.default_rng(rows * 1000 + C)
    w, b = rng.standard_normal((rows, C)).astype(F32), rng.standard_normal(C).astype(F32) if bias else None
    ga, be, mm = (rng.standard_normal(C).astype(F32) for _ in range(3))
    mv = rng.uniform(0, 2, C).astype(F32)
    mv[0] = 0
    ins = [vec(dev, a) for a in (w, ga, be, mm, mv)] + ([vec(dev, b)] if bias else [])
    wo, bo = blank(dev, rows * C), blank(dev, C)
    rc = lib.kpx_bn_fold_conv_f32(ins[0].ptr, ins[5].ptr if bias else None, rows, C, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, R.EPS, wo.ptr, bo.ptr,
                                  stream_of(dev))
    torch.cuda.synchronize(dev)
    assert rc == 0 and all(i.input_ok() for i in ins) and wo.output_ok() and bo.output_ok()
    ref, bnd = R.bn_fold(w, b, ga, be, mm, mv), R.fold_bounds(w, b, ga, be, mm, mv)
    r = max(R.worst(wo.get().reshape(rows, C) - ref[0], bnd[0]), R.worst(bo.get()[0] - ref[1], bnd[1]))
    report('kpx_bn_fold_conv_f32 %dx%d bias=%d' % (rows, C, bias), r)
    assert r <= 1.0


# ----------------------------------------------------------------------------------------------- determinism, graph replay, the wrapper
def test_two_runs_are_bit_equal(lib, dev):
    """The fixed-order reductions: a second run on fresh buffers gives the same bits (block caps and five groups)."""
    for name in ('s_big', 'g5x12'):
        c = R.case(name)
        res = []
        for _ in range(2):
            run = Run(lib, dev, c)
            f = run.forward(1)
            b = run.backward(1, 0)
            res.append([f[k] for k in ('mean', 'invstd', 'mm', 'mv', 'y')] + [b[k] for k in ('dx', 'dgamma', 'dbeta')])
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(*res))


def test_forward_and_backward_replayed_from_a_graph(lib, dev):
    c = R.case('g5x12')
    eager_run = Run(lib, dev, c)
    f = eager_run.forward(1)
    b = eager_run.backward(1, 0)
    eager = [f['mean'], f['invstd'], f['y'], b['dx'], b['dgamma'], b['dbeta'], f['mm'], f['mv']]
    run = Run(lib, dev, c)
    codes = []

    def enqueue():
        codes.append(run.enqueue_fwd(1))
        codes.append(run.enqueue_bwd(1, 0))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    assert codes == [0] * 4
    outs = (run.mean, run.invstd, run.y, run.dx, run.dgamma, run.dbeta, run.mm, run.mv)
    for _ in range(2):
        for o in outs[:4]:
            o.buf.fill_(SENTINEL)
        for o, a in zip(outs[4:], (c['pre_dgamma'], c['pre_dbeta'], c['mm0'], c['mv0'])):
            o.view.copy_(torch.from_numpy(np.array(a, F32)))
        graph.replay()
        torch.cuda.synchronize(dev)
        for o, e in zip(outs, eager):
            assert o.guards_ok() and np.array_equal(o.get().ravel().view(np.uint32), np.asarray(e, F32).ravel().view(np.uint32))
        assert run.sc.guards_ok()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_ops_batch_norm_against_float64(dev, dtype):
    """kpx.ops.batch_norm through autograd, groups = 2: the wrapper's scratch, statistics and gradient plumbing, same bounds."""
    from kpx_amd import ops
    half = dtype == 'bf16'
    c = R.case('b_21x24_ld40', bf16=True) if half else R.case('v_19x64_ld96')
    groups, n, C = c['shape'][:3]
    t = lambda a: torch.from_numpy(np.array(a, dtype=F32)).to(dev)
    x = t(c['x'].reshape(groups, 1, n, C))                       # NHWC with one image of n x 1 pixels per group
    x = (x.to(torch.bfloat16) if half else x).requires_grad_(True)
    gamma, beta = t(c['gamma']).requires_grad_(True), t(c['beta']).requires_grad_(True)
    mm, mv = t(c['mm0']), t(c['mv0'])
    y = ops.batch_norm(x, gamma, beta, mm, mv, train=True, act=ops.ACT_RELU, groups=groups)
    saved = y.grad_fn.saved_tensors                                # (x, gamma, beta, mean, invstd): the state the backward will run on
    mean, invstd = (s.detach().cpu().numpy().reshape(groups, C) for s in saved[3:5])
    y.backward(t(c['dy'].reshape(groups, 1, n, C)).to(y.dtype))
    torch.cuda.synchronize(dev)
    assert y.dtype == x.dtype and not R.undecided(c['x'], mean, invstd, c['gamma'], c['beta']).any()
    fwd = dict(mean=mean, invstd=invstd, mm=mm.cpu().numpy(), mv=mv.cpu().numpy(), y=y.detach().float().cpu().numpy().reshape(groups, n, C))
    bwd = dict(dx=x.grad.float().cpu().numpy().reshape(groups, n, C), dgamma=gamma.grad.cpu().numpy(), dbeta=beta.grad.cpu().numpy())
    assert ops.BN_EPS == R.EPS
    r = dict(R.forward_ratios(c, fwd, 1, bf16_y=half, decay=ops.BN_DECAY))
    r.update(R.backward_ratios(c, mean, invstd, bwd, 1, 0, bf16_dx=half))
    report('ops.batch_norm %s %s' % (dtype, {k: round(v, 4) for k, v in r.items()}), max(r.values()))
    assert max(r.values()) <= 1.0, r
