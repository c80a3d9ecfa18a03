"""The forward-only kernels FinalModel rolls out with, one by one: ops.tile_batch, ops.head_blend_tiled, ops.lstm_cell and ops.dense
(csrc/rollout.hip and the channel copy / 1x1-conv GEMM they compose).  Restatements, inputs and bounds: tests/loss_optim_ref.py.

Bounds (fixed before measuring):
  tile_batch        bit-exact against repeat_interleave; every element of the destination outside the written channel slice, and
                    64 floats after its last row, keep a sentinel bit pattern
  head_blend_tiled  final 16e(|im| mask + |raw|) + 1e-30 (the clamp is 1-Lipschitz, so the same bound with clip) ; mask 16e*mask ;
                    crude the bits of clamp(raw), or of raw with clip off ; with T = 1 and clip off within the same bounds of ops.head_blend
  lstm_cell, dense  rel-L2 < 1e-5 against float64, the bar of test_lstm_layer_over_32_steps_against_float64 for hs
Inputs are finite; what the clamp does with a NaN is not pinned here.  Each test prints ``ratio <entry> <value>``.
"""
import numpy as np
import pytest
import torch

import loss_optim_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 0x7fa5c3e1                   # a NaN bit pattern no kernel here produces
TAIL = 64


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


def report(entry, ratio):
    print('ratio %s %.4f' % (entry, ratio))
    return ratio


# ----------------------------------------------------------------------------------------------- tile_batch
def _tile_into(kpx, dev, x, t, ld, offset):
    """ops.tile_batch into channels [offset, offset + C) of a sentinel-filled [B*T, pix, ld] tensor with 64 more floats behind it.
    -> (rows as uint32 [B*T, pix, ld], the tail as uint32)."""
    b, pix, c = x.shape
    rows = b * t * pix * ld
    buf = torch.full((rows + TAIL,), SENTINEL, dtype=torch.int32, device=dev)
    out = buf[:rows].view(torch.float32).view(b * t, pix, ld)
    ret = kpx.ops.tile_batch(torch.from_numpy(x).to(dev), t, out=out, out_ld=ld, out_channel_offset=offset)
    torch.cuda.synchronize(dev)
    assert ret is out
    got = t2n(buf).view(np.uint32)
    return got[:rows].reshape(b * t, pix, ld), got[rows:]


def _tile_check(x, t, offset, rows, tail):
    c = x.shape[-1]
    assert np.array_equal(rows[..., offset:offset + c], bits(R.tile_batch(x, t)))
    assert np.all(rows[..., :offset] == SENTINEL) and np.all(rows[..., offset + c:] == SENTINEL), 'a channel outside the slice was written'
    assert np.all(tail == SENTINEL), 'the floats after the last row were written'


@pytest.mark.parametrize('b,t,pix,c', R.TILE_CASES)
def test_tile_batch_is_bit_exact(kpx, dev, b, t, pix, c):
    """C = 30 takes the scalar kernel (the K=15 points call), 80 and 128 the vector one; (3,32,256,128) is 786 432 vector items, past
    the cap of 2048 blocks."""
    x = R.tile_input(b, pix, c)
    want = torch.repeat_interleave(torch.from_numpy(x), t, dim=0).numpy()
    got = kpx.ops.tile_batch(torch.from_numpy(x).to(dev), t)              # the destination the op allocates itself
    assert got.shape == (b * t, pix, c) and np.array_equal(bits(t2n(got)), bits(want))
    _tile_check(x, t, 0, *_tile_into(kpx, dev, x, t, c, 0))


@pytest.mark.parametrize('offset', R.TILE_SLICE_OFFSETS)
def test_tile_batch_into_a_channel_slice(kpx, dev, offset):
    """The embedding call: 128 channels into a 160-wide tensor.  Offsets 0 and 4 keep the 16-byte alignment (vector kernel), offset 2
    falls back to the scalar kernel."""
    b, t, pix, c = R.TILE_SLICE_CASE
    x = R.tile_input(b, pix, c)
    _tile_check(x, t, offset, *_tile_into(kpx, dev, x, t, R.TILE_SLICE_LD, offset))


def test_tile_batch_refuses_a_destination_narrower_than_the_source(kpx, dev):
    from kpx_amd._lib import KpxError
    b, t, pix, c = 2, 3, 7, 6
    x = R.tile_input(b, pix, c)
    buf = torch.full((b * t * pix * c + TAIL,), SENTINEL, dtype=torch.int32, device=dev)
    out = buf[:b * t * pix * c].view(torch.float32)
    with pytest.raises(KpxError):
        kpx.ops.tile_batch(torch.from_numpy(x).to(dev), t, out=out, out_ld=c - 1)
    torch.cuda.synchronize(dev)
    assert np.all(t2n(buf) == SENTINEL)


# ----------------------------------------------------------------------------------------------- head_blend_tiled
@pytest.mark.parametrize('b,t,h,w', R.TILED_SHAPES)
@pytest.mark.parametrize('clip', [True, False])
def test_head_blend_tiled_against_float64(kpx, dev, b, t, h, w, clip):
    """Frame f blends image f // T (the images of different samples are independent draws, so f % T or a fixed image cannot pass); with
    clip both final and crude are clamped, and the inputs put a quarter of the blended and half of the raw values outside [-1, 1]."""
    im, raw, _ = R.blend_inputs(b, b * t, h, w, seed=R.TILED_SEED)
    unclipped = R.blend_tiled_fwd(im, raw, t, clip=False)
    assert np.mean(np.abs(unclipped[0]) > 1) >= 0.25 and np.mean(np.abs(unclipped[1]) > 1) >= 0.5
    assert b == 1 or not np.array_equal(im[0], im[1])
    fin, crude, mask = kpx.ops.head_blend_tiled(torch.from_numpy(im).to(dev), torch.from_numpy(raw).to(dev), t, clip=clip)
    want = R.blend_tiled_fwd(im, raw, t, clip=clip)
    bf, bm = R.blend_fwd_bounds(np.repeat(im, t, axis=0), raw)
    got_fin = t2n(fin)
    wf = report('head_blend_tiled final %s clip=%d' % ((b, t, h, w), clip), R.worst(got_fin - want[0], bf))
    wm = report('head_blend_tiled mask %s clip=%d' % ((b, t, h, w), clip), R.worst(t2n(mask) - want[2], bm))
    assert fin.shape == (b * t, h, w, 3) and crude.shape == (b * t, h, w, 3) and mask.shape == (b * t, h, w, 1)
    assert max(wf, wm) <= 1.0, (wf, wm)
    assert np.array_equal(bits(t2n(crude)), bits(np.clip(raw[..., :3], -1, 1) if clip else raw[..., :3]))
    if clip:
        assert np.abs(got_fin).max() <= 1.0 and np.mean(np.abs(got_fin) == 1.0) >= 0.2
    else:
        assert np.abs(got_fin).max() > 1.0
    if t == 1 and not clip:
        plain = kpx.ops.head_blend(torch.from_numpy(im).to(dev), torch.from_numpy(raw).to(dev))
        assert R.worst(t2n(plain[0]) - got_fin, bf) <= 1.0 and R.worst(t2n(plain[2]) - t2n(mask), bm) <= 1.0
        assert np.array_equal(bits(t2n(plain[1])), bits(t2n(crude)))


# ----------------------------------------------------------------------------------------------- lstm_cell, dense
@pytest.mark.parametrize('bsz,n_in,u', R.LSTM_CELL_SHAPES)
def test_lstm_cell_against_float64(kpx, dev, bsz, n_in, u):
    """One rollout step from a non-zero state: two channel copies into [x, h] (the second to a destination that is not 16-byte aligned
    when In = 30), the gate GEMM on the 1x1-conv kernel and the gate math."""
    x, h, c, kernel, bias = R.lstm_cell_inputs(bsz, n_in, u)
    h2, c2 = kpx.ops.lstm_cell(*(torch.from_numpy(a).to(dev) for a in (x, h, c, kernel, bias)))
    want_h, want_c = R.lstm_cell(x, h, c, kernel, bias)
    eh, ec = R.rel_l2(t2n(h2), want_h), R.rel_l2(t2n(c2), want_c)
    report('lstm_cell h %s' % ((bsz, n_in, u),), eh / 1e-5)
    report('lstm_cell c %s' % ((bsz, n_in, u),), ec / 1e-5)
    assert h2.shape == (bsz, u) and c2.shape == (bsz, u)
    assert eh < 1e-5 and ec < 1e-5, (eh, ec)


@pytest.mark.parametrize('rows,n_in,n_out', R.DENSE_SHAPES)
@pytest.mark.parametrize('act', R.DENSE_ACTS)
def test_dense_against_float64(kpx, dev, rows, n_in, n_out, act):
    x, w, b = R.dense_inputs(rows, n_in, n_out)
    y = kpx.ops.dense(*(torch.from_numpy(a).to(dev) for a in (x, w, b)), act=act)
    err = R.rel_l2(t2n(y), R.dense(x, w, b, act))
    report('dense %s act=%d' % ((rows, n_in, n_out), act), err / 1e-5)
    assert y.shape == (rows, n_out) and err < 1e-5, err
