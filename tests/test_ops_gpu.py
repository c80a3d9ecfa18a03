"""GPU parity tests: every HIP op (through the C ABI) against the CPU oracle on the same seeded inputs.

Tolerances (stated here once): conv / features / frames rel-L2 <= 1e-5 (north-star bar is 1e-4); gradients rel-L2 <= 1e-4;
key-points abs <= 2e-6 and heat-maps abs <= 2e-6 ("bit-pattern-close": the reduction order differs from numpy's).
"""
import os

import numpy as np
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def kpx():
    import kpx_amd
    return kpx_amd


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def t2n(t):
    return t.detach().cpu().numpy()


CONV_CASES = [
    # n, h, w, cin, cout, k, stride, pad, act
    (2, 16, 16, 32, 64, 3, 1, 0, 0),
    (2, 16, 16, 32, 64, 3, 2, 0, 0),       # SAME pad (0,1)
    (2, 17, 13, 16, 32, 3, 2, 0, 1),       # odd sizes, relu epilogue
    (2, 32, 32, 3, 32, 7, 1, 0, 0),        # encoder conv_1
    (2, 32, 32, 16, 15, 1, 1, 0, 0),       # 1x1 head, Cout=15
    (2, 32, 32, 3, 64, 4, 2, 1, 2),        # img_discr conv_0 (pad 1 + SAME), lrelu
    (2, 65, 65, 8, 16, 4, 2, 1, 2),        # img_discr conv_1 geometry: SAME (1,2)
    (2, 4, 4, 64, 1, 3, 1, 1, 0),          # D_logit: 4 -> 6
    (3, 8, 8, 158, 256, 3, 1, 0, 0),       # translator conv_1_0 channel count
    (2, 8, 8, 256, 128, 3, 1, 0, 0),
    (1, 32, 32, 64, 4, 3, 1, 0, 0),        # fused crude+mask head
    (5, 9, 9, 130, 130, 3, 1, 0, 0),       # ragged channel tiles
    (64, 4, 4, 128, 256, 4, 2, 1, 2),      # small-M / wide-N tile path
    (2, 4, 4, 256, 1, 3, 1, 1, 0),         # D_logit-shaped: wave-per-pixel small-Cout kernel
    (2, 6, 6, 512, 4, 3, 1, 0, 1),         # small-Cout kernel, Cout=4, relu
    (2, 20, 20, 3, 64, 3, 1, 0, 1),        # VGG conv1_1 shape (row-merged Cin=3)
    (4, 128, 128, 16, 16, 3, 1, 0, 0),     # pose conv_7_1: fwd + dgrad on the 16-cout kernel; wgrad on the tiny-filter 16 -> 16 variant (conv_wsmall.hip)
    (3, 48, 80, 32, 16, 3, 1, 0, 2),       # 16-cout kernel: two chunks, lrelu, non-square
    (4, 128, 128, 64, 16, 3, 1, 0, 1),     # same, two 32-channel input tiles per wave (pose conv_7_0); Winograd weight gradient
    (16, 64, 64, 128, 32, 3, 1, 0, 0),     # same, two channel tiles of 64 (pose conv_5_0); Winograd weight gradient
    (4, 128, 128, 64, 4, 3, 1, 0, 0),      # same, translator crude+mask head (forward: VALU kernel for few produced channels)
    (5, 128, 128, 32, 3, 3, 1, 0, 1),      # few-channel forward kernel, Cout = 3, relu, ragged tile count
    (3, 160, 144, 16, 4, 3, 1, 1, 2),      # same with an explicit pad (output 162 x 146), lrelu
    (2, 64, 64, 256, 128, 3, 1, 0, 0),     # Winograd weight gradient, 64 x 64 blocks, 4 x 2 of them (256 -> 128 channels)
    (4, 128, 128, 3, 32, 7, 1, 0, 0),      # encoder conv_1 at full resolution: wgrad on the tiny-filter 7x7 image-input variant (conv_wsmall.hip)
    (8, 8, 8, 512, 512, 3, 1, 0, 1),       # split-K forward/dgrad (VGG conv5 shape), relu epilogue in the reduce
    (16, 10, 10, 256, 512, 4, 2, 1, 2),    # split-K with stride-2 parity classes (img_discr conv_4 geometry)
    (2, 32, 48, 48, 96, 3, 1, 0, 2),       # fused Winograd F(2x2,3x3): non-square, 3 chunks of 16 channels, lrelu
    (3, 16, 16, 64, 32, 3, 1, 0, 1),       # Winograd, one 16x16 block per image, relu
    (2, 32, 32, 32, 48, 3, 1, 0, 0),       # Winograd with the produced channels padded to 64 in U and masked on store
    (2, 16, 16, 16, 16, 3, 1, 0, 1),       # Winograd, 16 -> 16 channels (pose conv_7_1 shape): two chunks, half-empty cout tile
    (1, 32, 32, 24, 40, 3, 1, 0, 2),       # Winograd, K = 24 (3 chunks), Nn = 40
    (8, 32, 64, 64, 128, 3, 1, 0, 0),      # Winograd weight gradient (64-channel tiles, non-square image, 64 splits)
    (16, 32, 32, 128, 16, 3, 1, 0, 0),     # Winograd weight gradient, 64 x 32 blocks with the 16 output channels masked (pose conv_7_0)
    (16, 32, 32, 32, 160, 3, 1, 0, 1),     # Winograd weight gradient, 32 x 64 blocks, Cout = 160 overhangs the last block
    (8, 64, 64, 64, 4, 3, 1, 0, 0),        # translator head shape: Winograd with 4 produced channels (fwd), 4 gathered channels (dgrad), wgrad on the tiny-filter 64 -> 4 variant
    (32, 64, 64, 128, 128, 3, 1, 0, 1),    # THE bench / roofline shape (translator conv_3_1 at B=32): 64-cout Winograd workgroups, 16 chunks, fwd + dgrad
    (64, 32, 32, 24, 64, 3, 1, 0, 2),      # 64-cout Winograd workgroups with a 3-chunk K loop (only the un-pipelined tail iterations run)
    (128, 8, 8, 64, 512, 3, 1, 0, 0),      # 64-cout Winograd workgroups on packed 8x8 images (VGG conv5 at a large batch)
    (8, 64, 64, 64, 40, 3, 1, 0, 0),       # 32-cout Winograd workgroups (Np = 64 but too few blocks), couts 40..63 masked, 8-chunk pipelined loop
    (3, 100, 72, 3, 64, 3, 1, 0, 1),       # image-input forward kernel (VGG conv1_1 shape), persistent workgroups over ragged 16x16 tiles, relu
    (2, 50, 70, 3, 24, 7, 1, 1, 2),        # same, 7x7 with an explicit pad, 24 of 32 output channels, lrelu
    (3, 70, 54, 3, 64, 4, 2, 1, 2),        # same kernel at stride 2 (img_discr conv_0: 4x4, explicit pad 1, 36 x 28 outputs), lrelu
    # tiny-filter weight gradients (conv_wsmall.hip: the whole filter gradient in one workgroup's 16x16 MFMA accumulators); (4,128,128,3,32,7)
    # and (8,64,64,64,4,3) above are its 7x7 image-input and 64 -> 4 head variants
    (2, 128, 128, 16, 16, 3, 1, 0, 1),     # pose conv_7_1 shape: 16 -> 16 at full resolution, nine 16-row blocks on three wavefronts
    (3, 100, 120, 16, 12, 3, 1, 0, 0),     # same variant, ragged: 25 x 2 tiles with a 56-column tail, 12 of 16 output channels
    (3, 104, 120, 3, 24, 7, 1, 0, 0),      # 7x7 image-input variant, ragged tiles, 24 of 32 output channels, 147 of 160 rows
    (8, 128, 128, 3, 64, 4, 2, 1, 2),      # img_discr conv_0: 4x4 stride 2 with the explicit pad, 65 x 65 outputs (one padded quad per row)
    (5, 96, 72, 64, 4, 3, 1, 0, 0),        # 64 -> 4 head variant on a non-square image (tile tails in both directions)
    (2, 128, 128, 32, 32, 3, 1, 0, 1),     # 32 -> 32 variant (encoder conv_2): 18 row blocks x 2 column blocks on six wavefronts
    (5, 100, 72, 32, 24, 3, 1, 0, 0),      # same, ragged tiles, 24 of 32 output channels
    # the two high-resolution row kernels of conv_wgrad.hip, which take what the tiny-filter variants and the Winograd weight gradient leave
    (4, 128, 128, 3, 16, 3, 1, 0, 0),      # row-merged multi-tap wgrad (conv_wgrad_rows_merged_kernel): image input, 3x3, 65 536 pixels
    (4, 128, 128, 16, 32, 3, 1, 0, 0),     # multi-tap small-channel wgrad (conv_wgrad_rows_kernel): 16 -> 32, one 32-channel block per wave
    (1, 32, 32, 128, 128, 3, 1, 0, 0),     # wgrad on the 8-wave 128x128 tiles of conv_wgrad_tap_rows_kernel (too few pixels for the Winograd weight gradient), two slabs
]

# One row per weight-gradient kernel family (enum KpxWgradFamily), the cheapest CONV_CASES row of each; test_wgrad_plan_cpu.py holds the
# plan of every one to its name.  GENERIC-MERGED: conv_wgrad_kernel's row-merged variant in a single slab (no workspace at all).
WGRAD_FAMILY_ROWS = {
    'WSMALL': (2, 128, 128, 16, 16, 3, 1, 0, 1),
    'WINO': (16, 32, 32, 128, 16, 3, 1, 0, 0),
    'ROWS_MERGED': (4, 128, 128, 3, 16, 3, 1, 0, 0),
    'ROWS': (4, 128, 128, 16, 32, 3, 1, 0, 0),
    'TAP_ROWS': (1, 32, 32, 64, 4, 3, 1, 0, 0),
    'GEMM3': (3, 48, 80, 32, 16, 3, 1, 0, 2),
    'GENERIC': (2, 32, 32, 16, 15, 1, 1, 0, 0),
    'GENERIC-MERGED': (2, 20, 20, 3, 64, 3, 1, 0, 1),
}


@pytest.mark.parametrize('n,h,w,cin,cout,k,s,pad,act', CONV_CASES)
def test_conv_fwd_dgrad_wgrad(kpx, dev, n, h, w, cin, cout, k, s, pad, act, gtol=1e-5):
    rs = np.random.RandomState(cin * 7 + cout)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    wt = (rs.randn(k, k, cin, cout) / np.sqrt(k * k * cin)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    # HIP forward first: the activation's backward mask (y > 0) is taken from ITS output for the oracle's backward too -- an
    # element whose pre-activation is ~1e-7 from zero may land on the other side in two correct fp32 implementations, and one
    # such flip alone moves a gradient's rel-L2 by ~1e-3 (seen with the Winograd forward, whose error is ~4e-7 instead of ~1e-7)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True); wg = torch.from_numpy(wt).to(dev).requires_grad_(True); bg = torch.from_numpy(b).to(dev).requires_grad_(True)
    yg = kpx.ops.conv2d(xg, wg, bg, stride=s, pad=pad, act=act)
    # oracle (+ autograd)
    xo = torch.from_numpy(x).requires_grad_(True); wo = torch.from_numpy(wt).requires_grad_(True); bo = torch.from_numpy(b).requires_grad_(True)
    zo = R.conv(xo, wo, bo, s, pad)
    yo = zo
    if act == 1: yo = torch.relu(zo)
    if act == 2: yo = torch.nn.functional.leaky_relu(zo, 0.01)
    assert tuple(yg.shape) == tuple(yo.shape)
    assert rel_l2(t2n(yg), t2n(yo)) < 1e-5
    gy = rs.randn(*yo.shape).astype(np.float32)
    if act:
        pos = yg.detach().cpu() > 0
        flips = int((pos != (zo.detach() > 0)).sum())
        assert flips <= 2 + 1e-5 * pos.numel(), flips                       # the two masks differ only on a handful of ~0 elements
        zo.backward(torch.from_numpy(gy) * torch.where(pos, torch.tensor(1.0), torch.tensor(0.0 if act == 1 else 0.01)))
    else:
        zo.backward(torch.from_numpy(gy))
    yg.backward(torch.from_numpy(gy).to(dev))
    assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < gtol
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < gtol
    assert rel_l2(t2n(bg.grad), t2n(bo.grad)) < gtol


@pytest.mark.parametrize('family', sorted(WGRAD_FAMILY_ROWS))
def test_wgrad_entry_stays_inside_the_planned_workspace(kpx, dev, family):
    """kpx_conv2d_wgrad_f32 called directly with a workspace of exactly the bytes kpx_conv2d_wgrad_plan names (none where the plan has one
    slab), followed by a guard of two slabs (a mistake in the split count is off by whole slabs): the guard keeps its bits, dw has the bits
    ops.conv_wgrad_raw gets with the query-sized scratch (the reduce is fixed-order), and is within 1e-5 rel-L2 of the oracle's."""
    import ctypes
    from kpx_amd._lib import lib
    n, h, w, cin, cout, k, s, pad, _ = WGRAD_FAMILY_ROWS[family]
    assert WGRAD_FAMILY_ROWS[family] in CONV_CASES
    pt, _, ho = kpx.ops.same_pad(h + 2 * pad, k, s)
    pl, _, wo = kpx.ops.same_pad(w + 2 * pad, k, s)
    pad_t, pad_l = pad + pt, pad + pl
    rs = np.random.RandomState(cin * 7 + cout)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    gy = rs.randn(n, ho, wo, cout).astype(np.float32)
    wo_ = torch.zeros(k, k, cin, cout, requires_grad=True)
    zo = R.conv(torch.from_numpy(x), wo_, None, s, pad)
    assert tuple(zo.shape) == gy.shape
    zo.backward(torch.from_numpy(gy))
    xg, dyg = torch.from_numpy(x).to(dev), torch.from_numpy(gy).to(dev)
    geom = (xg.data_ptr(), n, h, w, cin, cin, dyg.data_ptr(), ho, wo, cout, cout)
    fam, splits, need = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    arith = kpx.ops._arith()
    assert lib.kpx_conv2d_wgrad_plan(*geom, k, k, s, pad_t, pad_l, arith, ctypes.byref(fam), ctypes.byref(splits), ctypes.byref(need)) == 0
    slab = k * k * cin * cout
    assert need.value == (splits.value * slab * 4 if splits.value > 1 else 0)
    assert need.value <= lib.kpx_conv2d_wgrad_workspace_bytes(n, ho, wo, cin, cout, k, k)
    pattern = 0x5A5AA5A5                                      # a fixed bit pattern, as int32
    buf = torch.full((need.value // 4 + 2 * slab,), pattern, dtype=torch.int32, device=dev)
    dw = torch.full((k, k, cin, cout), float('nan'), dtype=torch.float32, device=dev)
    rc = lib.kpx_conv2d_wgrad_f32(*geom, dw.data_ptr(), k, k, s, pad_t, pad_l, arith, buf.data_ptr() if need.value else None, need.value, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[need.value // 4:] == pattern).all())
    via_ops = torch.full_like(dw, float('nan'))
    kpx.ops.conv_wgrad_raw(xg, cin, cin, dyg, cout, via_ops, s, pad_t, pad_l)
    torch.cuda.synchronize()
    assert torch.equal(dw.view(torch.int32), via_ops.view(torch.int32))
    assert rel_l2(t2n(dw), t2n(wo_.grad)) < 1e-5


def test_conv_reads_and_writes_channel_slices(kpx, dev):
    rs = np.random.RandomState(0)
    full = rs.randn(2, 8, 8, 160).astype(np.float32)
    wt = (rs.randn(3, 3, 158, 32) * 0.05).astype(np.float32)
    want = R.conv(torch.from_numpy(full[..., :158].copy()), torch.from_numpy(wt), None, 1)
    got = kpx.ops.conv2d(torch.from_numpy(full).to(dev), torch.from_numpy(wt).to(dev), None, stride=1, cin=158)
    assert rel_l2(t2n(got), t2n(want)) < 1e-5
    sl = torch.from_numpy(full).to(dev)[..., 16:48]          # a strided channel slice as input
    w2 = (rs.randn(3, 3, 32, 16) * 0.1).astype(np.float32)
    want2 = R.conv(torch.from_numpy(full[..., 16:48].copy()), torch.from_numpy(w2), None, 1)
    got2 = kpx.ops.conv2d(sl, torch.from_numpy(w2).to(dev), None, stride=1)
    assert rel_l2(t2n(got2), t2n(want2)) < 1e-5
    # Winograd-eligible geometry reading a channel slice of a wider buffer (translator conv_1_0-style joint buffer)
    full3 = rs.randn(2, 16, 16, 96).astype(np.float32)
    w3 = (rs.randn(3, 3, 64, 32) * 0.05).astype(np.float32)
    want3 = R.conv(torch.from_numpy(full3[..., 16:80].copy()), torch.from_numpy(w3), None, 1)
    got3 = kpx.ops.conv2d(torch.from_numpy(full3).to(dev)[..., 16:80], torch.from_numpy(w3).to(dev), None, stride=1)
    assert rel_l2(t2n(got3), t2n(want3)) < 1e-5
    # Winograd with a padded last channel chunk: 158 of 160 channels (translator conv_1_0); the two pad channels hold NaN and
    # must not reach the result
    full4 = rs.randn(2, 16, 16, 160).astype(np.float32)
    w4 = (rs.randn(3, 3, 158, 32) * 0.05).astype(np.float32)
    want4 = R.conv(torch.from_numpy(full4[..., :158].copy()), torch.from_numpy(w4), None, 1)
    full4[..., 158:] = np.nan
    got4 = kpx.ops.conv2d(torch.from_numpy(full4).to(dev), torch.from_numpy(w4).to(dev), None, stride=1, cin=158)
    assert rel_l2(t2n(got4), t2n(want4)) < 1e-5


def test_wgrad_of_a_158_channel_slice_ignores_the_pad_channels(kpx, dev):
    """Winograd wgrad with Cin = 158 read from a 160-channel buffer (translator conv_1_0): the two pad channels hold NaN."""
    rs = np.random.RandomState(5)
    full = rs.randn(8, 32, 32, 160).astype(np.float32)
    wt = (rs.randn(3, 3, 158, 64) * 0.05).astype(np.float32)
    gy = rs.randn(8, 32, 32, 64).astype(np.float32)
    xo = torch.from_numpy(full[..., :158].copy()); wo = torch.from_numpy(wt).requires_grad_(True)
    R.conv(xo, wo, None, 1).backward(torch.from_numpy(gy))
    full[..., 158:] = np.nan
    wg = torch.from_numpy(wt).to(dev).requires_grad_(True)
    y = kpx.ops.conv2d(torch.from_numpy(full).to(dev), wg, None, stride=1, cin=158)
    y.backward(torch.from_numpy(gy).to(dev))
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < 1e-5


@pytest.mark.parametrize('groups', [1, 2])
def test_batch_norm_train_fwd_bwd_and_moving(kpx, dev, groups):
    rs = np.random.RandomState(groups)
    n, h, w, c = 4, 9, 7, 32
    x = (rs.randn(n, h, w, c) * 2 + 0.5).astype(np.float32)
    g = (rs.rand(c) + 0.5).astype(np.float32); b = rs.randn(c).astype(np.float32)
    gy = rs.randn(n, h, w, c).astype(np.float32)
    xo = torch.from_numpy(x).requires_grad_(True); go = torch.from_numpy(g).requires_grad_(True); bo = torch.from_numpy(b).requires_grad_(True)
    ng = n // groups
    ys, stats = [], []
    for i in range(groups):
        y, mean, var = R.batch_norm_train(xo[i * ng:(i + 1) * ng], go, bo)
        ys.append(torch.relu(y)); stats.append((mean.detach(), var.detach()))
    yo = torch.cat(ys, 0)
    yo.backward(torch.from_numpy(gy))
    mm, mv = torch.zeros(c), torch.ones(c)
    for mean, var in stats:
        mm, mv = R.moving_update(mm, mv, mean, var, ng * h * w)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True); gg = torch.from_numpy(g).to(dev).requires_grad_(True); bg = torch.from_numpy(b).to(dev).requires_grad_(True)
    mmg, mvg = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    yg = kpx.ops.batch_norm(xg, gg, bg, mmg, mvg, train=True, act=1, groups=groups)
    assert rel_l2(t2n(yg), t2n(yo)) < 1e-5
    yg.backward(torch.from_numpy(gy).to(dev))
    assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < 1e-4
    assert rel_l2(t2n(gg.grad), t2n(go.grad)) < 1e-5
    assert rel_l2(t2n(bg.grad), t2n(bo.grad)) < 1e-5
    np.testing.assert_allclose(t2n(mmg), mm.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(t2n(mvg), mv.numpy(), rtol=1e-6)
    # inference mode uses the moving statistics
    yi = kpx.ops.batch_norm(xg.detach(), gg.detach(), bg.detach(), mmg, mvg, train=False, act=0)
    want = R.batch_norm_infer(torch.from_numpy(x), torch.from_numpy(g), torch.from_numpy(b), torch.from_numpy(t2n(mmg)), torch.from_numpy(t2n(mvg)))
    assert rel_l2(t2n(yi), t2n(want)) < 1e-5


def test_upsample_concat_fwd_bwd(kpx, dev):
    rs = np.random.RandomState(4)
    x = rs.randn(2, 5, 7, 16).astype(np.float32); sk = rs.randn(2, 10, 14, 8).astype(np.float32)
    xo = torch.from_numpy(x).requires_grad_(True); so = torch.from_numpy(sk).requires_grad_(True)
    yo = torch.cat([R.resize2x(xo), so], dim=-1)
    gy = rs.randn(*yo.shape).astype(np.float32)
    yo.backward(torch.from_numpy(gy))
    xg = torch.from_numpy(x).to(dev).requires_grad_(True); sg = torch.from_numpy(sk).to(dev).requires_grad_(True)
    yg = kpx.ops.upsample2x_concat(xg, sg)
    assert rel_l2(t2n(yg), t2n(yo)) < 1e-7
    yg.backward(torch.from_numpy(gy).to(dev))
    assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < 1e-6
    assert rel_l2(t2n(sg.grad), t2n(so.grad)) == 0.0
    y1 = kpx.ops.upsample2x_concat(torch.from_numpy(x).to(dev), None)
    assert rel_l2(t2n(y1), t2n(R.resize2x(torch.from_numpy(x)))) < 1e-7


@pytest.mark.parametrize('shape,scale', [((2, 128, 128, 15), 3.0), ((1, 24, 40, 5), 10.0), ((3, 32, 32, 40), 1.0)])
def test_keypoint_head_fwd_bwd(kpx, dev, shape, scale):
    rs = np.random.RandomState(shape[1])
    x = (rs.randn(*shape) * scale).astype(np.float32)
    xo = torch.from_numpy(x).requires_grad_(True)
    gy, _ = R.get_coord(xo, 2, shape[1]); gx, _ = R.get_coord(xo, 1, shape[2])
    muo = torch.stack([gx, gy], dim=2)
    gm = rs.randn(*muo.shape).astype(np.float32)
    muo.backward(torch.from_numpy(gm))
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    mug, py, px = kpx.ops.keypoint_head(xg)
    np.testing.assert_allclose(t2n(mug), t2n(muo), atol=2e-6, rtol=0)
    mug.backward(torch.from_numpy(gm).to(dev))
    assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < 1e-4


def test_cached_winograd_forms_die_with_their_filter(kpx, dev):
    """The pre-transformed filter cache is keyed by the filter's address.  A constant (VGG19 / inference-folded) filter that is freed
    without release_filters() must not serve its stale form to an unrelated filter that the allocator later places at the same address
    (seen as a wrong forward in a full test run: a dead store's folded filters, then a test tensor in the same block)."""
    rs = np.random.RandomState(77)
    x = rs.randn(2, 16, 16, 32).astype(np.float32)
    w_old = torch.from_numpy((rs.randn(3, 3, 32, 64) / 17.0).astype(np.float32)).to(dev)
    kpx.ops.register_constant_filter(w_old, 'stale/kernel')
    ptr = w_old.data_ptr()
    del w_old                                                     # owner gone, keys never released
    wn = (rs.randn(3, 3, 32, 64) / 17.0).astype(np.float32)
    w_new = torch.from_numpy(wn).to(dev)
    if w_new.data_ptr() != ptr:
        pytest.skip('the allocator did not reuse the block')
    y = kpx.ops.conv2d(torch.from_numpy(x).to(dev), w_new, None, stride=1)
    yo = R.conv(torch.from_numpy(x), torch.from_numpy(wn), None, 1, 0)
    assert rel_l2(t2n(y), t2n(yo)) < 1e-5
    # ... and a same-address filter of another shape is never matched either
    del w_new, y
    w_live = torch.from_numpy(wn).to(dev)
    kpx.ops.register_constant_filter(w_live, 'live/kernel')
    w_view = w_live.view(-1)[:3 * 3 * 16 * 128].view(3, 3, 16, 128)          # same address, different (Cin, Cout)
    x16 = rs.randn(2, 16, 16, 16).astype(np.float32)
    y = kpx.ops.conv2d(torch.from_numpy(x16).to(dev), w_view, None, stride=1)
    yo = R.conv(torch.from_numpy(x16), w_view.cpu(), None, 1, 0)
    assert rel_l2(t2n(y), t2n(yo)) < 1e-5
    kpx.ops.release_filters([(w_live.data_ptr(), 0), (w_live.data_ptr(), 1)])


@pytest.mark.parametrize('shape,k,scale', [((4, 128, 128, 16), 15, 1.0), ((1, 24, 40, 8), 5, 3.0), ((3, 32, 32, 32), 40, 0.5)])
def test_keypoint_head_folded_1x1_matches_conv_then_head(kpx, dev, shape, k, scale):
    """pose_encoder's 1x1 head + get_coord x2 as one op that never forms the logits (reference networks/__init__.py:54,68-72):
    key-points, profiles and all three gradients against the restatement run on conv-then-head, and against the unfused HIP pair."""
    rs = np.random.RandomState(shape[1] + k)
    c = shape[3]
    x = np.maximum(rs.randn(*shape), 0).astype(np.float32)                 # the head's input is a ReLU output
    w = (rs.randn(1, 1, c, k) * scale / np.sqrt(c)).astype(np.float32)
    bias = rs.randn(k).astype(np.float32)
    xo = torch.from_numpy(x).double().requires_grad_(True)
    wo = torch.from_numpy(w).double().requires_grad_(True)
    bo = torch.from_numpy(bias).double().requires_grad_(True)
    lo = xo @ wo[0, 0] + bo
    gy, pyo = R.get_coord(lo, 2, shape[1]); gx, pxo = R.get_coord(lo, 1, shape[2])
    muo = torch.stack([gx, gy], dim=2)
    gm = rs.randn(*muo.shape).astype(np.float32)
    muo.backward(torch.from_numpy(gm).double())
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    wg = torch.from_numpy(w).to(dev).requires_grad_(True)
    bg = torch.from_numpy(bias).to(dev).requires_grad_(True)
    mug, py, px = kpx.ops.keypoint_head_proj(xg, wg, bg)
    np.testing.assert_allclose(t2n(mug), t2n(muo), atol=2e-6, rtol=0)
    np.testing.assert_allclose(t2n(py), t2n(pyo), atol=1e-7, rtol=2e-5)
    np.testing.assert_allclose(t2n(px), t2n(pxo), atol=1e-7, rtol=2e-5)
    mug.backward(torch.from_numpy(gm).to(dev))
    assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < 1e-4
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < 1e-4
    # d(loss)/d(bias) is analytically zero (a per-channel constant cancels in both softmaxes): both sides hold rounding noise only
    assert np.abs(t2n(bo.grad)).max() < 1e-9
    assert np.abs(t2n(bg.grad)).max() < 1e-5 * max(1.0, np.abs(t2n(wg.grad)).max())
    # the unfused HIP pair (1x1 conv, then the head on the materialised logits) agrees to fp32 rounding
    xu = torch.from_numpy(x).to(dev).requires_grad_(True)
    wu = torch.from_numpy(w).to(dev).requires_grad_(True)
    bu = torch.from_numpy(bias).to(dev).requires_grad_(True)
    muu, _, _ = kpx.ops.keypoint_head(kpx.ops.conv2d(xu, wu, bu, stride=1))
    muu.backward(torch.from_numpy(gm).to(dev))
    kpx.ops.join_side_stream(dev)
    np.testing.assert_allclose(t2n(mug), t2n(muu), atol=2e-6, rtol=0)
    assert rel_l2(t2n(xg.grad), t2n(xu.grad)) < 1e-5
    assert rel_l2(t2n(wg.grad), t2n(wu.grad)) < 1e-5


def test_keypoint_head_and_renderer_match_reference_golden(kpx, dev, golden_dir):
    ref = np.load(os.path.join(golden_dir, 'model_utils_ref.npz'))
    for tag in ('a', 'b'):
        shape = tuple(ref['coord_%s_shape' % tag]); seed = int(ref['coord_%s_seed' % tag])
        x = (np.random.RandomState(seed).randn(*shape) * float(ref['coord_%s_scale' % tag])).astype(np.float32)
        mu, py, px = kpx.ops.keypoint_head(torch.from_numpy(x).to(dev))
        np.testing.assert_allclose(t2n(mu), ref['coord_%s_mu' % tag], atol=2e-6, rtol=0)
        np.testing.assert_allclose(t2n(py), ref['coord_%s_yprob' % tag], atol=1e-7, rtol=2e-5)
        np.testing.assert_allclose(t2n(px), ref['coord_%s_xprob' % tag], atol=1e-7, rtol=2e-5)
        gy, _ = kpx.model_utils.get_coord(torch.from_numpy(x).to(dev), 2, shape[1])
        np.testing.assert_allclose(t2n(gy), ref['coord_%s_mu' % tag][:, :, 1], atol=2e-6, rtol=0)
    for tag in ('lo', 'hi', 'rect'):
        mu = ref['gauss_%s_mu' % tag]; hw = [int(v) for v in ref['gauss_%s_hw' % tag]]
        got = kpx.model_utils.get_gaussian_maps(torch.from_numpy(mu).to(dev), hw)
        np.testing.assert_allclose(t2n(got), ref['gauss_%s_map' % tag], atol=2e-6, rtol=2e-5)


def test_gaussian_maps_bwd_and_joint_embedding(kpx, dev):
    rs = np.random.RandomState(9)
    b, k, hh, c = 2, 15, 32, 128
    cur = rs.uniform(-0.9, 0.9, (b, k, 2)).astype(np.float32); fut = rs.uniform(-0.9, 0.9, (b, k, 2)).astype(np.float32)
    emb = rs.randn(b, hh, hh, c).astype(np.float32)
    co = torch.from_numpy(cur).requires_grad_(True); fo = torch.from_numpy(fut).requires_grad_(True); eo = torch.from_numpy(emb).requires_grad_(True)
    jo = torch.cat([eo, R.get_gaussian_maps(co, [hh, hh]), R.get_gaussian_maps(fo, [hh, hh])], dim=-1)
    gy = rs.randn(b, hh, hh, 160).astype(np.float32)
    jo.backward(torch.from_numpy(gy[..., :158].copy()))
    cg = torch.from_numpy(cur).to(dev).requires_grad_(True); fg = torch.from_numpy(fut).to(dev).requires_grad_(True); eg = torch.from_numpy(emb).to(dev).requires_grad_(True)
    jg = kpx.ops.joint_embedding(eg, cg, fg)
    assert tuple(jg.shape) == (b, hh, hh, 160)
    np.testing.assert_allclose(t2n(jg)[..., :158], t2n(jo), atol=2e-6, rtol=2e-5)
    assert float(jg[..., 158:].abs().max()) == 0.0
    jg.backward(torch.from_numpy(gy).to(dev))
    assert rel_l2(t2n(cg.grad), t2n(co.grad)) < 1e-4
    assert rel_l2(t2n(fg.grad), t2n(fo.grad)) < 1e-4
    assert rel_l2(t2n(eg.grad), t2n(eo.grad)) == 0.0


def test_head_blend_xent_adam(kpx, dev):
    rs = np.random.RandomState(2)
    im = rs.uniform(-1, 1, (2, 8, 8, 3)).astype(np.float32); raw = rs.randn(2, 8, 8, 4).astype(np.float32)
    ro = torch.from_numpy(raw).requires_grad_(True)
    mask = torch.sigmoid(ro[..., 3:]); fo = torch.from_numpy(im) * mask + ro[..., :3] * (1 - mask)
    gy = rs.randn(2, 8, 8, 3).astype(np.float32)
    fo.backward(torch.from_numpy(gy))
    rg = torch.from_numpy(raw).to(dev).requires_grad_(True)
    fg, crude, mk = kpx.ops.head_blend(torch.from_numpy(im).to(dev), rg)
    assert rel_l2(t2n(fg), t2n(fo)) < 1e-6 and rel_l2(t2n(mk), t2n(mask)) < 1e-6
    fg.backward(torch.from_numpy(gy).to(dev))
    assert rel_l2(t2n(rg.grad), t2n(ro.grad)) < 1e-5
    # sigmoid xent, two label groups
    z = (rs.randn(144) * 3).astype(np.float32)
    zo = torch.from_numpy(z).requires_grad_(True)
    lo = R.sigmoid_xent(zo[:72], 1.0).mean() + R.sigmoid_xent(zo[72:], 0.0).mean()
    lo.backward()
    zg = torch.from_numpy(z).to(dev).requires_grad_(True)
    lg = kpx.ops.sigmoid_xent(zg, 72, 1.0, 72, 0.0)
    assert abs(float(lg[0]) - float(lo)) < 1e-6
    torch.autograd.backward([lg], [torch.tensor([1.0, 0.0, 0.0], device=dev)])
    assert rel_l2(t2n(zg.grad), t2n(zo.grad)) < 1e-6
    # Adam: 3 steps against the oracle's ApplyAdam restatement
    n = 1003
    p0 = rs.randn(n).astype(np.float32)
    params = {'w': torch.from_numpy(p0.copy())}
    opt = R.AdamTF(['w'], params)
    pad = (n + 3) // 4 * 4
    p = torch.zeros(pad, device=dev); p[:n] = torch.from_numpy(p0).to(dev)
    m = torch.zeros(pad, device=dev); v = torch.zeros(pad, device=dev)
    b1p, b2p = np.float32(0.5), np.float32(0.999)
    for _ in range(3):
        g = (rs.randn(n) * 0.1).astype(np.float32)
        opt.step(params, {'w': torch.from_numpy(g)}, 1e-4)
        gd = torch.zeros(pad, device=dev); gd[:n] = torch.from_numpy(g).to(dev)
        alpha = np.float32(np.float32(1e-4) * np.sqrt(np.float32(1) - b2p) / (np.float32(1) - b1p))
        kpx.ops.adam_tf_flat_(p, gd, m, v, alpha, 0.5, 0.999, 1e-8)
        b1p, b2p = np.float32(b1p * np.float32(0.5)), np.float32(b2p * np.float32(0.999))
        np.testing.assert_allclose(t2n(p)[:n], params['w'].numpy(), atol=3e-7, rtol=0)


def test_vgg_perceptual_loss_fwd_bwd(kpx, dev):
    rs = np.random.RandomState(7)
    vggw = kpx.synthetic_vgg19_weights(seed=19, width_div=8)
    gt = rs.uniform(-1, 1, (2, 32, 32, 3)).astype(np.float32); pred = rs.uniform(-1, 1, (2, 32, 32, 3)).astype(np.float32)
    vo = {k: (torch.from_numpy(w), torch.from_numpy(b)) for k, (w, b) in R.synthetic_vgg(seed=19, width_div=8).items()}
    po = torch.from_numpy(pred).requires_grad_(True)
    lo = R.perceptual_loss(vo, (torch.from_numpy(gt) + 1) / 2.0 * 255.0, (po + 1) / 2.0 * 255.0)
    lo.backward()
    vgg = kpx.Vgg19(weights=vggw, device=dev)
    pg = torch.from_numpy(pred).to(dev).requires_grad_(True)
    lg = vgg.perceptual_loss(torch.from_numpy(gt).to(dev), pg)
    assert abs(float(lg[0]) - float(lo)) < 1e-5 * abs(float(lo))
    lg.backward(torch.ones(1, device=dev))
    assert rel_l2(t2n(pg.grad), t2n(po.grad)) < 1e-4
    feats = vgg.build(torch.from_numpy(np.concatenate([gt, pred])).to(dev))
    fo = R.vgg19(vo, (torch.from_numpy(np.concatenate([gt, pred])) + 1) / 2.0 * 255.0)
    for a, b in zip(feats, fo):
        assert rel_l2(t2n(a), t2n(b)) < 1e-5


def _fuzz_cases():
    rs = np.random.RandomState(2024)
    cases = []
    for _ in range(28):
        k = int(rs.choice([1, 3, 3, 3, 4, 5, 7]))
        s = int(rs.choice([1, 1, 2])) if k > 1 else 1
        pad = int(rs.choice([0, 0, 1]))
        cin = int(rs.choice([1, 3, 4, 6, 16, 30, 32, 64, 130]))
        cout = int(rs.choice([1, 4, 15, 16, 32, 33, 64, 128]))
        h = int(rs.randint(max(2, k // 2), 24)); w = int(rs.randint(max(2, k // 2), 40))
        n = int(rs.randint(1, 5))
        act = int(rs.choice([0, 1, 2]))
        cases.append((n, h, w, cin, cout, k, s, pad, act))
    # shapes that reach the row-chunked / multi-tap / split-K paths with ragged channel counts
    cases += [(2, 64, 64, 36, 20, 3, 1, 0, 0), (3, 32, 96, 64, 64, 3, 1, 0, 1), (2, 64, 32, 128, 128, 3, 2, 0, 0),
              (32, 8, 8, 256, 192, 3, 1, 0, 2), (9, 12, 12, 320, 256, 4, 2, 1, 1), (1, 128, 128, 48, 8, 3, 1, 0, 0)]
    return cases


def _wino_fuzz_cases():
    """3x3 stride-1 SAME geometries around the Winograd eligibility rules (tile multiples, padded channel counts, 8x8 packing,
    weight-gradient block shapes and split counts)."""
    rs = np.random.RandomState(77)
    cases = []
    for _ in range(22):
        h = int(rs.choice([16, 32, 48, 64])); w = int(rs.choice([16, 32, 48, 64, 80]))
        n = int(rs.choice([1, 2, 3, 4, 8]))
        if rs.rand() < 0.2:
            h = w = 8; n = int(rs.choice([4, 8, 12]))
        cin = int(rs.choice([4, 8, 16, 24, 40, 64, 72, 96, 128, 160]))
        cout = int(rs.choice([4, 8, 16, 24, 32, 48, 64, 96, 128, 160]))
        cases.append((n, h, w, cin, cout, 3, 1, 0, int(rs.choice([0, 1, 2]))))
    cases += [(16, 32, 32, 64, 64, 3, 1, 0, 0), (4, 64, 64, 192, 64, 3, 1, 0, 1), (8, 32, 64, 96, 36, 3, 1, 0, 0)]     # wgrad splits / block shapes
    return cases


@pytest.mark.parametrize('n,h,w,cin,cout,k,s,pad,act', _wino_fuzz_cases())
def test_winograd_fuzz_against_oracle(kpx, dev, n, h, w, cin, cout, k, s, pad, act):
    test_conv_fwd_dgrad_wgrad(kpx, dev, n, h, w, cin, cout, k, s, pad, act, gtol=2e-5)


W43_CASES = [  # n, h, w, cin, cout, act
    (2, 16, 32, 16, 64, 0), (2, 32, 32, 64, 64, 1), (1, 16, 64, 24, 40, 2), (3, 48, 96, 136, 128, 0), (2, 32, 64, 64, 128, 1),
    (1, 16, 32, 256, 72, 0), (2, 128, 128, 64, 64, 1), (5, 32, 32, 40, 200, 2),
    (4, 16, 16, 64, 128, 1), (2, 16, 16, 256, 72, 0), (6, 16, 16, 40, 64, 2),          # 16x16 images, two to a workgroup
    (32, 64, 64, 128, 128, 1),          # THE bench / roofline launch (translator conv_3_1 at B=32): 2 048 workgroups, eight rounds of the chip
    (128, 16, 16, 512, 512, 1)]         # packed 16x16 images (VGG19 conv4_2 shape) on two rounds of the chip: 64 image pairs x 8 cout blocks = 512 workgroups


def _w43b_takes(h, w, k, nn):
    """Launch shapes of the bf16x3 form of F(4x4,3x3) (csrc/conv_wino43b.hip): 16 x 32-pixel regions or 16x16 images packed two to a workgroup
    (every such case here has an even image count), gathered channels a multiple of 4."""
    return ((h % 16 == 0 and w % 32 == 0) or (h == 16 and w == 16)) and k >= 16 and k % 4 == 0 and nn >= 33


@pytest.mark.parametrize('form', ['bf16x3', 'f32mfma'])
@pytest.mark.parametrize('n,h,w,cin,cout,act', W43_CASES)
def test_winograd_f43_forward_and_data_gradient_against_oracle(kpx, dev, monkeypatch, n, h, w, cin, cout, act, form):
    """The F(4x4,3x3) kernels through ops.conv2d with pre-transformed filters: forward and data gradient against the oracle convolution at
    the 1e-5 bar of a layer, ragged channel counts (K tail chunk / step, cout tail of a 64-wide block), all activations, and a check that
    it IS the kernel that ran.  form 'bf16x3': csrc/conv_wino43b.hip (the transform-domain GEMMs fp32-equivalent on the bf16 pipe) wherever
    it takes the shape, the fp32-MFMA kernel (csrc/conv_wino43.hip) on the rest; 'f32mfma': the latter everywhere (ops.WINO43B = False).
    Weight / bias gradients come from the shared wgrad kernel."""
    ops = kpx.ops
    if not ops.WINO43:
        pytest.skip('KPX_WINO43=0')
    monkeypatch.setattr(ops, 'WINO43_MIN_WORKGROUPS', 0)        # (the step only uses the kernel for launches of more than 128 workgroups)
    monkeypatch.setattr(ops, 'WINO43B', form == 'bf16x3')
    rs = np.random.RandomState(cin * 3 + cout)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) / np.sqrt(9 * cin)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True); wg = torch.from_numpy(wt).to(dev).requires_grad_(True); bg = torch.from_numpy(b).to(dev).requires_grad_(True)
    keys = ops.register_constant_filter(wg.detach(), 'test/f43')
    try:
        used, usedb = ops.conv_kernel_uses['wino43'], ops.conv_kernel_uses['wino43b']
        yg = ops.conv2d(xg, wg, bg, stride=1, pad=0, act=act)
        assert ops.conv_kernel_uses['wino43'] == used + 1
        assert ops.conv_kernel_uses['wino43b'] - usedb == (1 if form == 'bf16x3' and _w43b_takes(h, w, cin, cout) else 0)
        xo = torch.from_numpy(x).requires_grad_(True); wo = torch.from_numpy(wt).requires_grad_(True); bo = torch.from_numpy(b).requires_grad_(True)
        zo = R.conv(xo, wo, bo, 1, 0)
        yo = torch.relu(zo) if act == 1 else torch.nn.functional.leaky_relu(zo, 0.01) if act == 2 else zo
        assert rel_l2(t2n(yg), t2n(yo)) < 1e-5
        gy = rs.randn(*yo.shape).astype(np.float32)
        if act:
            pos = yg.detach().cpu() > 0
            assert int((pos != (zo.detach() > 0)).sum()) <= 2 + 1e-4 * pos.numel()
            zo.backward(torch.from_numpy(gy) * torch.where(pos, torch.tensor(1.0), torch.tensor(0.0 if act == 1 else 0.01)))
        else:
            zo.backward(torch.from_numpy(gy))
        yg.backward(torch.from_numpy(gy).to(dev))
        eligible_back = cout >= 16 and cin >= 33
        assert ops.conv_kernel_uses['wino43'] == used + (2 if eligible_back else 1)
        assert ops.conv_kernel_uses['wino43b'] - usedb == (form == 'bf16x3') * (int(_w43b_takes(h, w, cin, cout)) + int(eligible_back and _w43b_takes(h, w, cout, cin)))
    finally:
        ops.release_filters(keys)
    assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < 1e-5
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < 1e-5
    assert rel_l2(t2n(bg.grad), t2n(bo.grad)) < 1e-5


def test_winograd_f43_reads_a_channel_slice_and_writes_a_strided_destination(kpx, dev, monkeypatch):
    """K = 158 of a 160-wide joint buffer (translator conv_1_0) into a channel slice of a wider output, raw launcher."""
    ops = kpx.ops
    if not ops.WINO43:
        pytest.skip('KPX_WINO43=0')
    monkeypatch.setattr(ops, 'WINO43_MIN_WORKGROUPS', 0)
    rs = np.random.RandomState(5)
    full = rs.randn(2, 32, 32, 160).astype(np.float32)
    wt = (rs.randn(3, 3, 158, 96) * 0.03).astype(np.float32)
    xg = torch.from_numpy(full).to(dev); wg = torch.from_numpy(wt).to(dev)
    out = torch.full((2, 32, 32, 128), 7.0, device=dev)
    keys = ops.register_constant_filter(wg, 'test/slice')
    try:
        used = ops.conv_kernel_uses['wino43']
        ops.conv_fwd_raw(xg, 160, 158, wg, None, out[..., 16:], 128, 1, 1, 1, 0)
        assert ops.conv_kernel_uses['wino43'] == used + 1
    finally:
        ops.release_filters(keys)
    want = R.conv(torch.from_numpy(full[..., :158].copy()), torch.from_numpy(wt), None, 1)
    got = t2n(out)
    assert rel_l2(got[..., 16:112], t2n(want)) < 1e-5
    assert (got[..., :16] == 7.0).all() and (got[..., 112:] == 7.0).all()


@pytest.mark.parametrize('n,h,w,cin,cout', [(32, 64, 64, 128, 128), (32, 128, 128, 64, 64), (8, 64, 64, 256, 128), (8, 32, 32, 256, 256), (4, 64, 64, 64, 136)])
def test_wino43_bf16x3_entry_is_fp32_equivalent_against_float64(kpx, dev, n, h, w, cin, cout):
    """The bf16x3 form of F(4x4,3x3) is the fp32 configuration's arithmetic: every transform-domain operand is split EXACTLY into three bf16
    terms (U once per update in fp64 -> fp32 -> split; V in registers after the fp32 input transform), the six products of weight >= 2^-16 are
    exact in fp32 and accumulated in fp32.  Against a float64 convolution, on the profiled launches (translator conv_3_1 / conv_5_1 at B=32)
    and two wide-channel layers, its error must be no larger than 1.5x the fp32-MFMA F(4x4,3x3) kernel's (measured: 0.83-0.85x -- the MFMA's
    fp32 products round, these do not) -- forward and data gradient, through the C ABI."""
    lib, ops, check = kpx._lib.lib, kpx.ops, kpx._lib.check
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(3, 3, cin, cout, generator=g) / (9 * cin) ** 0.5
    dy = torch.randn(n, h, w, cout, generator=g)
    xg, wg, dyg = x.to(dev), wt.to(dev), dy.to(dev)

    def ref64(inp, f):
        return torch.nn.functional.conv2d(inp.double().permute(0, 3, 1, 2), f.double().permute(3, 2, 0, 1), None, padding=1).permute(0, 2, 3, 1)
    for dgrad, inp, k, nn, want in ((0, xg, cin, cout, ref64(x, wt)), (1, dyg, cout, cin, ref64(dy, wt.flip(0, 1).permute(0, 1, 3, 2)))):
        ub = torch.empty(lib.kpx_wino43b_u_bytes(cin, cout), dtype=torch.uint8, device=dev)
        uo = torch.empty(lib.kpx_wino43_u_bytes(cin, cout), dtype=torch.uint8, device=dev)
        check(lib.kpx_wino43b_filter_transform_f32(wg.data_ptr(), cin, cout, dgrad, ub.data_ptr(), ops._stream()), 'transform b')
        check(lib.kpx_wino43_filter_transform_f32(wg.data_ptr(), cin, cout, dgrad, uo.data_ptr(), ops._stream()), 'transform')
        yb = torch.empty(n, h, w, nn, device=dev); yo = torch.empty(n, h, w, nn, device=dev)
        check(lib.kpx_conv3x3_wino43b_f32(inp.data_ptr(), n, h, w, k, k, ub.data_ptr(), None, yb.data_ptr(), nn, nn, 0, None, 0, None, 0, None, None, 0, None, ops._stream()), 'conv b')
        check(lib.kpx_conv3x3_wino43_f32(inp.data_ptr(), n, h, w, k, k, uo.data_ptr(), None, yo.data_ptr(), nn, nn, 0, None, 0, None, 0, None, None, 0, None, ops._stream()), 'conv')
        eb = float((yb.cpu().double() - want).norm() / want.norm()); eo = float((yo.cpu().double() - want).norm() / want.norm())
        assert eb < 1e-5 and eb <= 1.5 * eo, (dgrad, eb, eo)


def test_wino43b_epilogue_options_through_the_c_abi(kpx, dev):
    """kpx_conv3x3_wino43b_f32's launch forms against torch on the same inputs: statistics strips (sum / sum of squares per 4 x 16-pixel strip
    of the stored output), the batch-norm-backward form (masked gradient + sum(dz), sum(dz (z - beta))), ReLU mask + 2x2 max-pool, a cout tail
    (Nn = 72: second 64-wide tile holds 8 channels), a channel slice of a wider buffer (K = 24 of ld 32), and the argument checks."""
    lib, ops, check = kpx._lib.lib, kpx.ops, kpx._lib.check
    g = torch.Generator().manual_seed(77)
    n, h, w, c = 2, 32, 64, 64

    def conv64(x, wt, b=None):
        return torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wt.double().permute(3, 2, 0, 1), b.double() if b is not None else None, padding=1).permute(0, 2, 3, 1)

    def run(x, k, ldx, wt, b, nn, act=0, mask=None, pool=False, stats=False, bn=None):
        u = torch.empty(lib.kpx_wino43b_u_bytes(wt.shape[2], wt.shape[3]), dtype=torch.uint8, device=dev)
        check(lib.kpx_wino43b_filter_transform_f32(wt.data_ptr(), wt.shape[2], wt.shape[3], 0, u.data_ptr(), ops._stream()), 'transform')
        y = torch.full((x.shape[0], x.shape[1], x.shape[2], nn), float('nan'), device=dev)
        slab = torch.empty(lib.kpx_conv3x3_wino43_stats_tiles(x.shape[0], x.shape[1], x.shape[2]) * 2 * nn, device=dev) if (stats or bn) else None
        py = torch.empty((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, nn), device=dev) if pool else None
        rc = lib.kpx_conv3x3_wino43b_f32(x.data_ptr(), x.shape[0], x.shape[1], x.shape[2], k, ldx, u.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), nn, nn, act,
                                         mask.data_ptr() if mask is not None else None, nn if mask is not None else 0, py.data_ptr() if pool else None, nn if pool else 0,
                                         slab.data_ptr() if slab is not None else None, bn[0].data_ptr() if bn else None, nn if bn else 0, bn[1].data_ptr() if bn else None, ops._stream())
        return rc, y, slab, py
    x = torch.randn(n, h, w, c, generator=g).to(dev); wt = (torch.randn(3, 3, c, c, generator=g) / 24).to(dev); b = torch.randn(c, generator=g).to(dev)
    want = conv64(x.cpu(), wt.cpu(), b.cpu())
    rc, y, slab, _ = run(x, c, c, wt, b, c, stats=True)
    assert rc == 0 and rel_l2(t2n(y), want.numpy()) < 1e-5
    s = slab.view(-1, 2, c).double().sum(0).cpu()
    np.testing.assert_allclose(s[0].numpy(), y.double().sum((0, 1, 2)).cpu().numpy(), rtol=1e-6, atol=1e-4)
    np.testing.assert_allclose(s[1].numpy(), (y.double() ** 2).sum((0, 1, 2)).cpu().numpy(), rtol=1e-6)
    strips = slab.view(n, h // 16, w // 32, 8, 2, c)            # strip (region, 4-row band r, 16-column half q): index 2 r + q
    band = y[0, 4:8, 16:32].double().sum((0, 1)).cpu().numpy()
    np.testing.assert_allclose(strips[0, 0, 0, 3, 0].cpu().numpy(), band, rtol=1e-5, atol=1e-5)
    m = torch.randn(n, h, w, c, generator=g).to(dev)
    rc, y2, _, py = run(x, c, c, wt, b, c, act=1, mask=m, pool=True)
    wm = torch.relu(want) * (m.cpu() > 0)
    assert rc == 0 and rel_l2(t2n(y2), wm.numpy()) < 1e-5
    assert rel_l2(t2n(py), torch.nn.functional.max_pool2d(wm.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()) < 1e-5
    z = torch.randn(n, h, w, c, generator=g).to(dev); beta = torch.randn(c, generator=g).to(dev)
    rc, dz, slab, _ = run(x, c, c, wt, None, c, bn=(z, beta))
    wdz = conv64(x.cpu(), wt.cpu()) * (z.cpu() > 0)
    assert rc == 0 and rel_l2(t2n(dz), wdz.numpy()) < 1e-5
    s = slab.view(-1, 2, c).double().sum(0).cpu()
    np.testing.assert_allclose(s[0].numpy(), wdz.sum((0, 1, 2)).numpy(), rtol=1e-4, atol=2e-4)
    np.testing.assert_allclose(s[1].numpy(), (wdz * (z.cpu().double() - beta.cpu().double())).sum((0, 1, 2)).numpy(), rtol=1e-4, atol=2e-4)
    # cout tail and a channel slice
    wt2 = (torch.randn(3, 3, 24, 72, generator=g) / 15).to(dev); b2 = torch.randn(72, generator=g).to(dev)
    xw = torch.randn(1, 16, 32, 32, generator=g).to(dev)
    rc, y3, _, _ = run(xw, 24, 32, wt2, b2, 72, act=2)
    w3 = torch.nn.functional.leaky_relu(conv64(xw.cpu()[..., :24], wt2.cpu(), b2.cpu()), 0.01)
    assert rc == 0 and rel_l2(t2n(y3), w3.numpy()) < 1e-5
    # 16x16 images, two to a workgroup (an even number of them): forward with mask + pool; no statistics from that form
    xp = torch.randn(4, 16, 16, c, generator=g).to(dev); mp = torch.randn(4, 16, 16, c, generator=g).to(dev)
    rc, yp, _, pp = run(xp, c, c, wt, b, c, act=1, mask=mp, pool=True)
    assert rc == 0
    wantp = torch.relu(conv64(xp.cpu(), wt.cpu(), b.cpu())) * (mp.cpu() > 0)
    assert rel_l2(t2n(yp), wantp.numpy()) < 1e-5
    assert rel_l2(t2n(pp), torch.nn.functional.max_pool2d(wantp.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()) < 1e-5
    assert lib.kpx_conv3x3_wino43_stats_tiles(4, 16, 16) == 0
    assert lib.kpx_conv3x3_wino43b_eligible(4, 16, 16, 64, 64, 64, x.data_ptr()) == 1 and lib.kpx_conv3x3_wino43b_eligible(3, 16, 16, 64, 64, 64, x.data_ptr()) == 0
    # rejected: statistics together with mask / pool, the batch-norm form with a bias, K % 4 != 0
    assert run(x, c, c, wt, b, c, mask=m, stats=True)[0] == -1
    assert run(x, c, c, wt, b, c, bn=(z, beta))[0] == -1
    assert lib.kpx_conv3x3_wino43b_eligible(2, 32, 32, 158, 64, 160, x.data_ptr()) == 0
    assert lib.kpx_conv3x3_wino43b_eligible(2, 32, 64, 64, 64, 64, x.data_ptr()) == 1


@pytest.mark.parametrize('n,h,w,cin,cout,k,s,pad,act', _fuzz_cases())
def test_conv_fuzz_against_oracle(kpx, dev, n, h, w, cin, cout, k, s, pad, act):
    """Seeded random geometries (ragged channels, odd sizes, strides, explicit pads) through fwd / dgrad / wgrad."""
    # gradients here can be single numbers made of cancelling terms (e.g. a 1x1x1x1 kernel): 1e-4 instead of 1e-5
    test_conv_fwd_dgrad_wgrad(kpx, dev, n, h, w, cin, cout, k, s, pad, act, gtol=1e-4)


def test_shared_variable_used_twice_accumulates_into_the_bucket(kpx, dev):
    """Two ops using the same variable inside one backward (the reference's two pose_encoder calls, made unbatched) must ADD
    their weight / BN gradients in the flat-bucket destination instead of overwriting each other."""
    rs = np.random.RandomState(11)
    x1 = rs.randn(2, 8, 8, 8).astype(np.float32); x2 = rs.randn(2, 8, 8, 8).astype(np.float32)
    wt = (rs.randn(3, 3, 8, 8) * 0.2).astype(np.float32); b = rs.randn(8).astype(np.float32)
    g = (rs.rand(8) + 0.5).astype(np.float32); be = rs.randn(8).astype(np.float32)
    to = lambda a: torch.from_numpy(a).requires_grad_(True)
    wo, bo, go, beo = to(wt), to(b), to(g), to(be)
    total = 0
    for x in (x1, x2):
        y = R.conv(torch.from_numpy(x), wo, bo, 1)
        y, _, _ = R.batch_norm_train(y, go, beo)
        total = total + torch.relu(y).square().sum()
    total.backward()
    W, Bv, G, Be = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (wt, b, g, be))
    bucket = {n: torch.full_like(t, 123.0).detach() for n, t in (('w', W), ('b', Bv), ('g', G), ('be', Be))}   # poisoned: must be overwritten
    mm, mv = torch.zeros(8, device=dev), torch.ones(8, device=dev)
    kpx.ops.begin_backward()
    tot = 0
    for x in (x1, x2):
        y = kpx.ops.conv2d(torch.from_numpy(x).to(dev), W, Bv, stride=1, w_grad_out=bucket['w'], b_grad_out=bucket['b'])
        y = kpx.ops.batch_norm(y, G, Be, mm, mv, train=True, act=1, g_grad_out=bucket['g'], b_grad_out=bucket['be'])
        tot = tot + y.square().sum()
    tot.backward()
    kpx.ops.join_side_stream()
    torch.cuda.synchronize()
    assert rel_l2(t2n(bucket['w']), t2n(wo.grad)) < 1e-5
    assert rel_l2(t2n(bucket['g']), t2n(go.grad)) < 1e-5
    assert rel_l2(t2n(bucket['be']), t2n(beo.grad)) < 1e-5
    np.testing.assert_allclose(t2n(bucket['b']), t2n(bo.grad), atol=1e-3)     # exactly zero in exact arithmetic (BN follows)


# ------------------------------------------------------------------------------------------------ bf16 configuration (BASELINE configs[2])
# Activation tensors are bf16 in HBM; arithmetic is bf16 x bf16 products accumulated in fp32.  Parity is stated in two parts:
#   * ARITHMETIC: on bf16-rounded operands the kernels must reproduce the oracle's fp32 result to the fp32 bar (rel-L2 <= 1e-5) -- checked on
#     the kernels' fp32-output forms (and on the fp32 weight gradients): nothing but the storage rounding separates the two configurations;
#   * STORAGE: a bf16 output must be the round-to-nearest of that fp32 result: rel-L2 vs the ROUNDED oracle <= 1e-3 (a few elements sit on a
#     rounding boundary and fall to the other side), vs the unrounded oracle <= 3e-3 (2^-9 per element).
BF16S_CASES = [
    # n, h, w, cin, cout, act
    (2, 16, 32, 32, 128, 1),         # one chunk, 128-cout tile
    (2, 32, 64, 64, 128, 0),
    (1, 32, 32, 160, 256, 1),        # five chunks, two cout tiles (translator conv_1_0's buffer width)
    (3, 16, 32, 16, 64, 0),          # K = 16: channel tail of the only chunk; 64-cout variant
    (2, 32, 32, 64, 32, 1),          # 32-cout variant
    (2, 32, 32, 32, 16, 0),          # 16 produced channels in a 32-wide block
    (4, 16, 16, 128, 128, 1),        # 16x16 images: two-row pixel blocks, images stacked in a tile
    (8, 8, 8, 64, 128, 0),           # 8x8 images: four-row blocks (VGG19 conv5_*)
    (2, 64, 64, 128, 128, 1),        # translator conv_3_1 shape
    (2, 16, 16, 256, 64, 2),         # leaky relu, 64-cout variant on 16x16 images
    (16, 8, 8, 32, 32, 0),
    (32, 64, 64, 128, 128, 1),       # THE roofline launch of the configuration (bench.py roofline_bf16_conv): 256 workgroups
    (16, 128, 128, 64, 64, 1),       # 512 tiles on 256 persistent workgroups: the tile boundary (next tile requested before the epilogue), 512 x 64 variant
    (12, 64, 64, 128, 256, 0),       # 256-pixel tiles x 2 cout tiles = 384 tiles, two per persistent workgroup (cout tile fastest)
]


def _bf16s_raw(kpx, dev, x16, w, bias, act, dgrad=False, out_f32=False, mask=None, stats=False):
    lib, ops = kpx._lib.lib, kpx.ops
    n, h, wd, _ = x16.shape
    cin, cout = w.shape[2], w.shape[3]
    kk, nn = (cout, cin) if dgrad else (cin, cout)
    wf = torch.empty(lib.kpx_conv3x3_bf16s_weights_bytes(kk, nn), dtype=torch.uint8, device=dev)
    kpx._lib.check(lib.kpx_conv3x3_bf16s_prepare_f32(w.data_ptr(), cin, cout, 1 if dgrad else 0, wf.data_ptr(), ops._stream()), 'prepare')
    out = torch.full((n, h, wd, nn), 7.0, dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    st = None
    if stats:
        st = torch.zeros(lib.kpx_conv3x3_bf16s_stats_tiles(n, h, wd, kk, nn) * 2 * nn, dtype=torch.float32, device=dev)
    kpx._lib.check(lib.kpx_conv3x3_bf16s(x16.data_ptr(), n, h, wd, kk, x16.stride(2), wf.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(), nn, nn,
                                         1 if out_f32 else 0, act, mask.data_ptr() if mask is not None else None, mask.shape[3] if mask is not None else 0,
                                         st.data_ptr() if st is not None else None, ops._stream()), 'kpx_conv3x3_bf16s')
    return out, st


@pytest.mark.parametrize('n,h,w,cin,cout,act', BF16S_CASES)
def test_bf16_storage_conv3x3_forward_data_and_weight_gradient(kpx, dev, n, h, w, cin, cout, act):
    """csrc/conv_bf16s.hip / conv_bf16s_wgrad.hip through the C ABI on bf16-rounded operands against the oracle convolution of the SAME
    rounded operands: fp32-output forward and data gradient and the fp32 weight gradient at the fp32 bar (1e-5), the bf16 output against the
    rounded oracle, the epilogue's batch-norm sums against float64 sums of the oracle's pre-activation output."""
    lib, ops = kpx._lib.lib, kpx.ops
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(n, h, w, cin, generator=g).bfloat16()
    wt = (torch.randn(3, 3, cin, cout, generator=g) / (9 * cin) ** 0.5).bfloat16().float()        # bf16-representable filter: the kernel's own rounding is exact
    b = torch.randn(cout, generator=g)
    dy = torch.randn(n, h, w, cout, generator=g).bfloat16()
    xo = x.float().requires_grad_(True); wo = wt.clone().requires_grad_(True)
    zo = R.conv(xo, wo, b, 1, 0)
    yo = torch.relu(zo) if act == 1 else torch.nn.functional.leaky_relu(zo, 0.01) if act == 2 else zo
    zo.backward(dy.float())
    xg, wg, bg, dyg = x.to(dev), wt.to(dev), b.to(dev), dy.to(dev)
    assert lib.kpx_conv3x3_bf16s_eligible(n, h, w, cin, cout, cin, xg.data_ptr())
    y32, _ = _bf16s_raw(kpx, dev, xg, wg, bg, act, out_f32=True)
    y16, st = _bf16s_raw(kpx, dev, xg, wg, bg, act, stats=True)
    assert rel_l2(t2n(y32), t2n(yo)) < 1e-5
    assert rel_l2(t2n(y16.float()), t2n(yo.detach().bfloat16().float())) < 1e-3
    assert rel_l2(t2n(y16.float()), t2n(yo)) < 3e-3
    z64 = zo.detach().double().reshape(-1, cout)
    sums = st.view(-1, 2, cout).double().sum(0).cpu()
    assert rel_l2(sums[0].numpy(), z64.sum(0).numpy()) < 1e-4 and rel_l2(sums[1].numpy(), (z64 * z64).sum(0).numpy()) < 1e-5
    if lib.kpx_conv3x3_bf16s_eligible(n, h, w, cout, cin, cout, dyg.data_ptr()) and cin % 4 == 0:
        dx32, _ = _bf16s_raw(kpx, dev, dyg, wg, None, 0, dgrad=True, out_f32=True)
        assert rel_l2(t2n(dx32), t2n(xo.grad)) < 1e-5
    if lib.kpx_conv3x3_wgrad_bf16_eligible(n, h, w, cin, cin, cout, cout, xg.data_ptr(), dyg.data_ptr()):
        dw = torch.full((3, 3, cin, cout), 7.0, device=dev)
        nbytes = lib.kpx_conv3x3_wgrad_bf16_workspace_bytes(n, h, w, cin, cout)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        kpx._lib.check(lib.kpx_conv3x3_wgrad_bf16(xg.data_ptr(), n, h, w, cin, cin, dyg.data_ptr(), cout, cout, dw.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), 'wgrad')
        assert rel_l2(t2n(dw), t2n(wo.grad)) < 1e-5
    else:
        assert w % 16 or (h % (128 // min(w, 32))) or cin <= 32 and cout <= 32, 'every shape of the path has a bf16 weight gradient'


def test_bf16_storage_conv_reads_a_channel_slice_gates_by_a_mask_and_writes_a_strided_destination(kpx, dev):
    """K = 158 of a 160-wide bf16 joint buffer (translator conv_1_0: the two pad channels meet zero filter rows), the ReLU-mask epilogue of
    the VGG19 data gradients, and a strided destination whose other channels must stay untouched."""
    ops, lib = kpx.ops, kpx._lib.lib
    g = torch.Generator().manual_seed(3)
    full = torch.randn(2, 32, 32, 160, generator=g).bfloat16()
    full[..., 158:] = 0
    wt = (torch.randn(3, 3, 158, 96, generator=g) * 0.03).bfloat16().float()
    m = torch.randn(2, 32, 32, 96, generator=g).bfloat16()
    xg, wg, mg = full.to(dev), wt.to(dev), m.to(dev)
    out = torch.full((2, 32, 32, 128), 7.0, dtype=torch.bfloat16, device=dev)
    used = ops.conv_kernel_uses_bf16s[0]
    assert ops.conv3x3_same(xg, 160, 158, wg, None, out, 128, 96, 0, False, mask=mg) is not None
    assert ops.conv_kernel_uses_bf16s[0] == used + 1
    want = R.conv(full[..., :158].float(), wt, None, 1) * (m.float() > 0)
    got = t2n(out.float())
    assert rel_l2(got[..., :96], t2n(want.bfloat16().float())) < 1e-3
    assert (got[..., 96:] == 7.0).all()


BF16_GATHER_CASES = [(4, 33, 64, 128, 4, 2, 1, 2), (4, 18, 256, 512, 4, 2, 1, 2), (2, 32, 32, 64, 3, 2, 0, 0), (8, 6, 1024, 2048, 4, 2, 1, 2), (2, 64, 64, 128, 3, 2, 0, 0)]


BF16_IMAGE_CASES = [(2, 128, 3, 32, 7, 1, 0, 0, False), (8, 128, 3, 64, 4, 2, 1, 2, True), (2, 128, 3, 64, 3, 1, 0, 1, True)]


@pytest.mark.parametrize('n,h,cin,cout,k,s,pad,act,xgrad', BF16_IMAGE_CASES)
def test_bf16_storage_image_input_layers_read_fp32_images_and_exchange_bf16(kpx, dev, n, h, cin, cout, k, s, pad, act, xgrad):
    """pose_encoder conv_1 (7x7x3 -> 32), img_discriminator conv_0 (4x4/s2, 3 -> 64) and a VGG19 conv1_1-shaped layer in the bf16
    configuration: the image stays fp32, the produced tensor and the incoming gradient are bf16 (kpx_conv_image_{fwd,dgrad,wgrad}_bf16: the
    LDS-resident image kernels with a bf16 store / load) -- against the oracle: outputs at the storage bound, the fp32 image and parameter
    gradients at the fp32 bar, and no detour through an fp32 kernel (the 3x3 layer's filter is a constant in the model: its weight gradient
    is the one allowed detour)."""
    ops = kpx.ops
    ops.set_compute_dtype('bf16')
    try:
        for key in ops.fallback_uses:
            ops.fallback_uses[key] = 0
        g = torch.Generator().manual_seed(k * 100 + cout)
        x = torch.randn(n, h, h, cin, generator=g)
        w = torch.randn(k, k, cin, cout, generator=g) / (k * k * cin) ** 0.5
        b = torch.randn(cout, generator=g)
        xg = x.to(dev).requires_grad_(xgrad); wg = w.to(dev).requires_grad_(True); bg = b.to(dev).requires_grad_(True)
        y = ops.conv2d(xg, wg, bg, stride=s, pad=pad, act=act)
        assert y.dtype == torch.bfloat16
        gy = torch.randn(*y.shape, generator=g).bfloat16()
        y.backward(gy.to(dev))
        ops.join_side_stream()
        assert ops.fallback_uses == {'conv_fwd': 0, 'conv_dgrad': 0, 'conv_wgrad': 1 if k == 3 else 0, 'other': 0}, ops.fallback_uses
    finally:
        ops.set_compute_dtype('f32')
    xo = x.clone().requires_grad_(xgrad); wo = w.clone().requires_grad_(True); bo = b.clone().requires_grad_(True)
    zo = R.conv(xo, wo, bo, s, pad)
    yo = torch.relu(zo) if act == 1 else torch.nn.functional.leaky_relu(zo, 0.01) if act == 2 else zo
    yk = y.detach().float().cpu()
    fac = torch.where(yk > 0, torch.tensor(1.0), torch.tensor(0.01 if act == 2 else 0.0)) if act else torch.ones_like(zo)
    zo.backward((gy.float() * fac).bfloat16().float() if act else gy.float())          # (the HIP path stores the gated gradient as bf16 too)
    assert rel_l2(t2n(y.float()), t2n(yo.detach().bfloat16().float())) < 1e-3           # fp32 arithmetic, ONE rounding at the store (boundary ties aside)
    if xgrad:
        assert xg.grad.dtype == torch.float32
        assert rel_l2(t2n(xg.grad), t2n(xo.grad)) < 1e-5
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < 1e-5
    assert rel_l2(t2n(bg.grad), t2n(bo.grad)) < 1e-5


def test_bf16_storage_four_channel_head_takes_its_fp32_gradient_through_the_bf16_kernels(kpx, dev):
    """The translator's head (3x3, 64 -> 4, fp32 output feeding the mask / crude image): its fp32 gradient is cast into a zero-padded
    8-channel bf16 operand (kpx_cast_channels kind 3) and both gradients run on the bf16 3x3 kernels -- no fp32 detour."""
    ops = kpx.ops
    n, h, cin, cout = 2, 64, 64, 4
    ops.set_compute_dtype('bf16')
    try:
        for key in ops.fallback_uses:
            ops.fallback_uses[key] = 0
        g = torch.Generator().manual_seed(64004)
        x = torch.randn(n, h, h, cin, generator=g).bfloat16()
        w = (torch.randn(3, 3, cin, cout, generator=g) / (9 * cin) ** 0.5).bfloat16().float()
        b = torch.randn(cout, generator=g)
        xg = x.to(dev).requires_grad_(True); wg = w.to(dev).requires_grad_(True); bg = b.to(dev).requires_grad_(True)
        y = ops.conv2d(xg, wg, bg, stride=1, pad=0, act=0, out_dtype=torch.float32)
        assert y.dtype == torch.float32
        gy = torch.randn(*y.shape, generator=g).bfloat16().float()
        y.backward(gy.to(dev))
        ops.join_side_stream()
        assert sum(ops.fallback_uses.values()) == 0, ops.fallback_uses
    finally:
        ops.set_compute_dtype('f32')
    xo = x.float().requires_grad_(True); wo = w.clone().requires_grad_(True); bo = b.clone().requires_grad_(True)
    yo = R.conv(xo, wo, bo, 1, 0)
    yo.backward(gy)
    assert rel_l2(t2n(y), t2n(yo.detach())) < 1e-5
    assert rel_l2(t2n(xg.grad.float()), t2n(xo.grad.bfloat16().float())) < 4e-3
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < 1e-5
    assert rel_l2(t2n(bg.grad), t2n(bo.grad)) < 1e-5


@pytest.mark.parametrize('n,h,cin,cout,k,s,pad,act', BF16_GATHER_CASES)
def test_bf16_storage_strided_layers_through_autograd(kpx, dev, n, h, cin, cout, k, s, pad, act):
    """The discriminator's 4x4 stride-2 layers and the encoders' stride-2 layers on bf16 tensors (kpx_conv2d_{fwd,dgrad,wgrad}_bf16: the
    bf16-pipe gather kernels with bf16 I/O) through ops.conv2d, against the oracle on the rounded operands: bf16 outputs at the storage
    bound, fp32 parameter gradients at 1e-5-class accuracy, and NO detour through an fp32 kernel."""
    ops = kpx.ops
    ops.set_compute_dtype('bf16')
    try:
        for key in ops.fallback_uses:
            ops.fallback_uses[key] = 0
        g = torch.Generator().manual_seed(cin + cout)
        x = torch.randn(n, h, h, cin, generator=g).bfloat16()
        w = (torch.randn(k, k, cin, cout, generator=g) / (k * k * cin) ** 0.5).bfloat16().float()
        b = torch.randn(cout, generator=g)
        xg = x.to(dev).requires_grad_(True); wg = w.to(dev).requires_grad_(True); bg = b.to(dev).requires_grad_(True)
        y = ops.conv2d(xg, wg, bg, stride=s, pad=pad, act=act)
        assert y.dtype == torch.bfloat16
        gy = torch.randn(*y.shape, generator=g).bfloat16()
        y.backward(gy.to(dev))
        assert sum(ops.fallback_uses.values()) == 0, ops.fallback_uses
    finally:
        ops.set_compute_dtype('f32')
    xo = x.float().requires_grad_(True); wo = w.clone().requires_grad_(True); bo = b.clone().requires_grad_(True)
    zo = R.conv(xo, wo, bo, s, pad)
    yo = torch.nn.functional.leaky_relu(zo, 0.01) if act == 2 else zo
    fac = torch.where(y.detach().float().cpu() > 0, torch.tensor(1.0), torch.tensor(0.01)) if act == 2 else torch.ones_like(zo)
    zo.backward((gy.float() * fac).bfloat16().float() if act else gy.float())          # (the HIP path stores the gated gradient as bf16 too)
    assert rel_l2(t2n(y.float()), t2n(yo.detach().bfloat16().float())) < 4e-3           # (the filter's TRUNCATION to bf16 is exact here: it is bf16 already)
    assert rel_l2(t2n(xg.grad.float()), t2n(xo.grad.bfloat16().float())) < 6e-3
    assert rel_l2(t2n(wg.grad), t2n(wo.grad)) < 1e-5
    assert rel_l2(t2n(bg.grad), t2n(bo.grad)) < 1e-5


@pytest.mark.parametrize('n,h,w,cin,cout,groups', [(4, 32, 32, 32, 64, 1), (4, 64, 64, 64, 128, 2), (8, 16, 16, 128, 128, 2), (2, 128, 128, 16, 16, 1)])
def test_bf16_storage_conv_batch_norm_relu_forward_and_backward(kpx, dev, monkeypatch, n, h, w, cin, cout, groups):
    """conv -> train-mode batch norm -> relu -> conv in the bf16 configuration: batch statistics from the conv epilogue's fp32 sums
    (kpx_conv3x3_bf16s + kpx_bn_train_fwd_bf16), backward sums from the data-gradient epilogue (kpx_conv3x3_bf16s_bnbwd + kpx_bn_train_bwd_bf16),
    per-call statistics for ``groups`` weight-sharing calls.  Against the fp32 oracle on the same (rounded) inputs at the configuration's
    storage tolerance, and the fused paths against the unfused ones (separate reduction passes over the bf16 tensors)."""
    ops = kpx.ops
    g = torch.Generator().manual_seed(cin + cout + groups)
    x = torch.randn(n, h, w, cin, generator=g).bfloat16()
    x[n // 2:] += 0.5
    w1 = (torch.randn(3, 3, cin, cout, generator=g) / (9 * cin) ** 0.5).bfloat16().float()
    w2 = (torch.randn(3, 3, cout, cout, generator=g) / (9 * cout) ** 0.5).bfloat16().float()
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    gy = torch.randn(n, h, w, cout, generator=g).bfloat16()

    def run(fuse):
        monkeypatch.setattr(ops, 'FUSE_BN_STATS', fuse)
        monkeypatch.setattr(ops, 'FUSE_BN_BWD', fuse)
        ops.set_compute_dtype('bf16')
        try:
            used = dict(ops.fused_bn_uses)
            xg = x.to(dev).requires_grad_(True)
            p = [t.to(dev).requires_grad_(True) for t in (w1, w2, gamma, beta)]
            mm, mv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
            z = ops.conv2d(xg, p[0], None, stride=1, pad=0, bn_stats=True)
            a = ops.batch_norm(z, p[2], p[3], mm, mv, train=True, act=ops.ACT_RELU, groups=groups)
            y = ops.conv2d(a, p[1], None, stride=1, pad=0)
            y.backward(gy.to(dev))
            d = {k: ops.fused_bn_uses[k] - used[k] for k in used}
            assert d == ({'stats_from_conv_epilogue': groups, 'backward_sums_from_dgrad_epilogue': groups} if fuse else {'stats_from_conv_epilogue': 0, 'backward_sums_from_dgrad_epilogue': 0}), d
            return [t2n(t.float()) for t in (y, xg.grad, p[0].grad, p[1].grad, p[2].grad, p[3].grad, mm, mv)]
        finally:
            ops.set_compute_dtype('f32')
    fused, plain = run(True), run(False)
    xo = x.float().requires_grad_(True)
    po = [t.clone().requires_grad_(True) for t in (w1, w2, gamma, beta)]
    zo = R.conv(xo, po[0], None, 1, 0)
    ng = n // groups
    ao = torch.cat([torch.relu(R.batch_norm_train(zo[i * ng:(i + 1) * ng], po[2], po[3])[0]) for i in range(groups)], 0)
    yo = R.conv(ao, po[1], None, 1, 0)
    yo.backward(gy.float())
    want = [t2n(t) for t in (yo, xo.grad, po[0].grad, po[1].grad, po[2].grad, po[3].grad)]
    for name, got in (('fused', fused), ('plain', plain)):
        for i, tol in enumerate((8e-3, 3e-2, 3e-2, 8e-3, 2e-2, 2e-2)):            # y, dx, dw1, dw2, dgamma, dbeta: ~4e-3 of bf16 storage per stage, 2-4 stacked stages
            assert rel_l2(got[i], want[i]) < tol, (name, i, rel_l2(got[i], want[i]))
    for i in range(8):                                                          # fused epilogue sums vs reduction passes: the same numbers up to storage rounding
        assert rel_l2(fused[i], plain[i]) < (4e-3 if i < 6 else 1e-3), (i, rel_l2(fused[i], plain[i]))      # (moving statistics: sums of the fp32 accumulators vs of the rounded tensor)


@pytest.mark.parametrize('n,h,cin,cout,groups', [(6, 8, 128, 128, 2), (2, 8, 128, 128, 2), (6, 16, 32, 64, 2), (8, 8, 64, 64, 2), (4, 8, 128, 128, 2)])
def test_bf16_storage_batch_norm_groups_with_packed_conv_tiles(kpx, dev, n, h, cin, cout, groups):
    """The bf16 3x3 kernel packs G images into one statistics tile on 8x8 (and narrow 16x16) layers.  With n / groups not a multiple of G a
    tile straddles two batch-norm groups: the tile sums must then be dropped for the separate reduction pass (round-5 advisor finding:
    int(ng * tiles_per_image) truncated and the group statistics were silently wrong, mean = var = 0 at n / groups = 1).  Forward output and
    all gradients against the fp32 oracle with per-group statistics, whichever path runs."""
    ops = kpx.ops
    g = torch.Generator().manual_seed(n * 100 + h + cin)
    x = torch.randn(n, h, h, cin, generator=g).bfloat16()
    x[n // 2:] += 0.75                                                        # the two groups have different statistics
    w1 = (torch.randn(3, 3, cin, cout, generator=g) / (9 * cin) ** 0.5).bfloat16().float()
    w2 = (torch.randn(3, 3, cout, cout, generator=g) / (9 * cout) ** 0.5).bfloat16().float()
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    gy = torch.randn(n, h, h, cout, generator=g).bfloat16()
    ops.set_compute_dtype('bf16')
    try:
        xg = x.to(dev).requires_grad_(True)
        p = [t.to(dev).requires_grad_(True) for t in (w1, w2, gamma, beta)]
        mm, mv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        z = ops.conv2d(xg, p[0], None, stride=1, pad=0, bn_stats=True)
        a = ops.batch_norm(z, p[2], p[3], mm, mv, train=True, act=ops.ACT_RELU, groups=groups)
        y = ops.conv2d(a, p[1], None, stride=1, pad=0)
        y.backward(gy.to(dev))
        got = [t2n(t.float()) for t in (y, xg.grad, p[0].grad, p[1].grad, p[2].grad, p[3].grad)]
    finally:
        ops.set_compute_dtype('f32')
    xo = x.float().requires_grad_(True)
    po = [t.clone().requires_grad_(True) for t in (w1, w2, gamma, beta)]
    zo = R.conv(xo, po[0], None, 1, 0)
    ng = n // groups
    ao = torch.cat([torch.relu(R.batch_norm_train(zo[i * ng:(i + 1) * ng], po[2], po[3])[0]) for i in range(groups)], 0)
    yo = R.conv(ao, po[1], None, 1, 0)
    yo.backward(gy.float())
    want = [t2n(t) for t in (yo, xo.grad, po[0].grad, po[1].grad, po[2].grad, po[3].grad)]
    for i, tol in enumerate((8e-3, 4e-2, 4e-2, 8e-3, 3e-2, 3e-2)):      # (8x8 / 16x16 layers of 2-8 images: dx 3.1e-2, dw1 3.0e-2, dgamma / dbeta 2.1e-2 measured)
        assert rel_l2(got[i], want[i]) < tol, (i, rel_l2(got[i], want[i]))


def test_bf16_storage_pointwise_kernels_against_torch_on_the_rounded_inputs(kpx, dev):
    """cast, channel-slice copy, bilinear x2 (+ backward), 2x2 max-pool, the one-pass VGG19 feature gradient, feature L1, bias-gradient sum:
    fp32 arithmetic on bf16 tensors -- the bf16 results must be the rounding of the fp32 oracle's on the same inputs (<= 1 ulp: rel-L2 1e-3)."""
    lib, ops, check = kpx._lib.lib, kpx.ops, kpx._lib.check
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 16, 24, 32, generator=g)
    xb = x.bfloat16()
    xg = xb.to(dev)
    assert torch.equal(ops.cast(x.to(dev), torch.bfloat16).cpu(), xb) and torch.equal(ops.cast(xg, torch.float32).cpu(), xb.float())
    # resize forward / backward
    up = torch.empty(3, 32, 48, 40, dtype=torch.bfloat16, device=dev)
    check(lib.kpx_resize2x_fwd_bf16(xg.data_ptr(), 3, 16, 24, 32, 32, up.data_ptr(), 40, ops._stream()), 'resize')
    want = R.resize2x(xb.float())
    assert rel_l2(t2n(up[..., :32].float()), t2n(want.bfloat16().float())) < 1e-3
    dup = torch.randn(3, 32, 48, 32, generator=g).bfloat16()
    xr = xb.float().requires_grad_(True)
    R.resize2x(xr).backward(dup.float())
    dx = torch.empty(3, 16, 24, 32, dtype=torch.bfloat16, device=dev)
    check(lib.kpx_resize2x_bwd_bf16(dup.to(dev).data_ptr(), 3, 16, 24, 32, 32, dx.data_ptr(), 32, ops._stream()), 'resize bwd')
    assert rel_l2(t2n(dx.float()), t2n(xr.grad.bfloat16().float())) < 1e-3
    # max-pool and the fused feature gradient (f = [gt ; pred])
    f = torch.relu(torch.randn(4, 16, 24, 32, generator=g)).bfloat16()
    pool = torch.empty(4, 8, 12, 32, dtype=torch.bfloat16, device=dev)
    check(lib.kpx_maxpool2_fwd_bf16(f.to(dev).data_ptr(), 4, 16, 24, 32, pool.data_ptr(), ops._stream()), 'pool')
    want_pool = torch.nn.functional.max_pool2d(f.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(pool.float().cpu(), want_pool)
    dyp = torch.randn(2, 8, 12, 32, generator=g).bfloat16()
    gsc = torch.tensor([0.37], device=dev)
    d = torch.empty(2, 16, 24, 32, dtype=torch.bfloat16, device=dev)
    half = f.numel() // 2
    check(lib.kpx_vgg_feat_bwd_bf16(f.to(dev).data_ptr(), half, gsc.data_ptr(), 0.01, dyp.to(dev).data_ptr(), 2, 16, 24, 32, d.data_ptr(), ops._stream()), 'feat bwd')
    fp = f[2:].float().requires_grad_(True)
    pooled = torch.nn.functional.max_pool2d(fp.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    ((pooled * dyp.float()).sum() + 0.37 * 0.01 * (f[:2].float() - fp).abs().sum()).backward()
    want_d = fp.grad * (fp.detach() > 0)
    ties = (t2n(d.float()) != t2n(want_d.bfloat16().float())).mean()
    assert ties < 0.02 and rel_l2(t2n(d.float()), t2n(want_d)) < 0.2          # (equal maxima inside a window: first-maximum rule vs torch's; rare on random data)
    loss = torch.empty(1, device=dev)
    sc = ops.scratch.get('l1', 8192, dev)
    check(lib.kpx_l1_pair_fwd_bf16(f.to(dev).data_ptr(), half, loss.data_ptr(), sc.data_ptr(), ops._stream()), 'l1')
    assert abs(float(loss.cpu()) - float((f[:2].float() - f[2:].float()).abs().mean())) < 1e-6
    s = torch.empty(32, device=dev)
    ops.chan_sum_raw(xg, 32, 3 * 16 * 24, 32, s)
    assert rel_l2(t2n(s), t2n(xb.float().reshape(-1, 32).sum(0))) < 1e-6


@pytest.mark.parametrize('n,h,w,cin,cout,groups', [(4, 32, 32, 32, 64, 1), (4, 16, 48, 64, 40, 2), (2, 64, 64, 128, 128, 1), (4, 16, 32, 24, 70, 2), (2, 32, 32, 16, 32, 1),
                                                     (2, 32, 32, 16, 16, 1), (4, 32, 48, 64, 16, 2)])      # the last two: 16-cout kernel (conv_c16.hip)
def test_batch_norm_statistics_from_the_conv_epilogue(kpx, dev, monkeypatch, n, h, w, cin, cout, groups):
    """conv -> train-mode batch norm with the per-tile channel sums written by the Winograd epilogue (kpx_conv3x3_wino(43)_f32 with tile_stats +
    kpx_bn_train_fwd_f32 taking them as tile_stats) against the oracle AND against the separate statistics pass: same normalised output, same
    moving-statistics update, per-call statistics for ``groups`` weight-sharing calls (reference detector_translator_model.py:166-167)."""
    ops = kpx.ops
    monkeypatch.setattr(ops, 'WINO43_MIN_WORKGROUPS', 0)        # small launches too: both kernels' epilogues are covered by the shape list
    rs = np.random.RandomState(cin + cout)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    x[n // 2:] += 0.5                                   # the two groups see different statistics
    wt = (rs.randn(3, 3, cin, cout) / np.sqrt(9 * cin)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    ga = rs.uniform(0.5, 1.5, cout).astype(np.float32); be = rs.randn(cout).astype(np.float32)
    xg, wg, bg = (torch.from_numpy(a).to(dev) for a in (x, wt, b))
    gg, beg = torch.from_numpy(ga).to(dev), torch.from_numpy(be).to(dev)
    keys = ops.register_constant_filter(wg)
    try:
        y = ops.conv2d(xg, wg, bg, stride=1, pad=0, act=0, bn_stats=True)
        f43 = ops.WINO43 and w % 32 == 0 and cin >= 16 and cout >= 33          # these shapes run the F(4x4,3x3) kernel: statistics per 4x16-pixel strip
        assert hasattr(y, '_kpx_tile_stats') and y._kpx_tile_stats[1] == ((h // 16) * (w // 32) * 8 if f43 else (h // 16) * (w // 16))
        mm1, mv1 = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        used = ops.fused_bn_uses['stats_from_conv_epilogue']
        out1 = ops.batch_norm(y, gg, beg, mm1, mv1, train=True, act=1, groups=groups)
        assert ops.fused_bn_uses['stats_from_conv_epilogue'] == used + groups
        y2 = y.detach().clone()                         # no tile statistics attached: the separate statistics pass
        mm2, mv2 = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
        out2 = ops.batch_norm(y2, gg, beg, mm2, mv2, train=True, act=1, groups=groups)
    finally:
        ops.release_filters(keys)
    assert rel_l2(t2n(out1), t2n(out2)) < 2e-6
    np.testing.assert_allclose(t2n(mm1), t2n(mm2), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(t2n(mv1), t2n(mv2), rtol=1e-6)
    zo = R.conv(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), 1, 0)
    ng = n // groups
    want = torch.cat([torch.relu(R.batch_norm_train(zo[g * ng:(g + 1) * ng], torch.from_numpy(ga), torch.from_numpy(be))[0]) for g in range(groups)])
    assert rel_l2(t2n(out1), t2n(want)) < 1e-5


@pytest.mark.parametrize('n,h,w,c0,c1,c2,groups,f43', [(4, 32, 32, 32, 64, 48, 1, False), (4, 16, 32, 64, 32, 64, 2, False), (2, 64, 64, 64, 128, 128, 1, False),
                                                      (4, 32, 32, 32, 64, 48, 1, True), (4, 16, 32, 64, 128, 64, 2, True), (2, 64, 64, 64, 128, 128, 1, True),
                                                      (2, 128, 128, 16, 64, 64, 2, True)])
def test_batch_norm_backward_sums_from_the_dgrad_epilogue(kpx, dev, n, h, w, c0, c1, c2, groups, f43):
    """conv_a -> BN+ReLU -> conv_b: the data gradient of conv_b (Winograd kernel) also reduces BN's backward sums in its epilogue --
    kpx_conv3x3_wino_f32 / kpx_conv3x3_wino43(b)_f32 with tile_stats + bn_y + bn_beta (F(4x4,3x3) also stores the ReLU-masked gradient) --
    and kpx_bn_train_bwd_f32 takes the per-tile sums instead of its reduction pass.  Gradients wrt the input, gamma, beta and conv_a's filter
    against torch autograd over the oracle, and against the path with the separate reduction pass."""
    ops = kpx.ops
    rs = np.random.RandomState(c0 + c1 + c2)
    x = rs.randn(n, h, w, c0).astype(np.float32)
    wa = (rs.randn(3, 3, c0, c1) / np.sqrt(9 * c0)).astype(np.float32); wb = (rs.randn(3, 3, c1, c2) / np.sqrt(9 * c1)).astype(np.float32)
    ga = rs.uniform(0.5, 1.5, c1).astype(np.float32); be = (rs.randn(c1) * 0.3).astype(np.float32)
    gy = rs.randn(n, h, w, c2).astype(np.float32)

    def run(fused):
        keep, keep43 = ops.FUSE_BN_BWD, ops.WINO43
        ops.FUSE_BN_BWD, ops.WINO43 = fused, f43   # (which Winograd kernel takes conv_b's data gradient)
        try:
            return _run(fused)
        finally:
            ops.FUSE_BN_BWD, ops.WINO43 = keep, keep43

    def _run(fused):
        t = {k_: torch.from_numpy(v).to(dev).requires_grad_(True) for k_, v in dict(x=x, wa=wa, wb=wb, ga=ga, be=be).items()}
        keys = ops.register_constant_filter(t['wa'].detach()) + ops.register_constant_filter(t['wb'].detach())
        try:
            ya = ops.conv2d(t['x'], t['wa'], None, stride=1, pad=0, act=0, bn_stats=True)
            mm, mv = torch.zeros(c1, device=dev), torch.ones(c1, device=dev)
            yb = ops.batch_norm(ya, t['ga'], t['be'], mm, mv, train=True, act=1, groups=groups)
            out = ops.conv2d(yb, t['wb'], None, stride=1, pad=0, act=0)
            ops.begin_backward()
            used, used43 = ops.fused_bn_uses['backward_sums_from_dgrad_epilogue'], ops.conv_kernel_uses['wino43']
            out.backward(torch.from_numpy(gy).to(dev))
            hit = ops.fused_bn_uses['backward_sums_from_dgrad_epilogue'] - used
            if fused:                            # the data gradient of conv_b ran on the kernel this case is about
                assert (ops.conv_kernel_uses['wino43'] - used43 >= 1) == (f43 and c1 % 64 == 0 and w % 32 == 0), (f43, ops.conv_kernel_uses['wino43'] - used43)
        finally:
            ops.release_filters(keys)
        return {k_: t2n(v.grad) for k_, v in t.items()}, t2n(out), hit, (yb.detach() > 0).cpu()
    g1, o1, hit1, mask1 = run(True)
    g0, o0, hit0, mask0 = run(False)   # the same kernels without the sums: batch norm makes its own reduction pass
    assert hit1 == groups and hit0 == 0 and bool((mask1 == mask0).all())
    to = {k_: torch.from_numpy(v).requires_grad_(True) for k_, v in dict(x=x, wa=wa, wb=wb, ga=ga, be=be).items()}
    za = R.conv(to['x'], to['wa'], None, 1, 0)
    ng = n // groups
    zpre = torch.cat([R.batch_norm_train(za[g * ng:(g + 1) * ng], to['ga'], to['be'])[0] for g in range(groups)])
    # The oracle's ReLU takes the HIP forward's mask: the two forwards agree to ~1e-6, so among ~1 M pre-activations about one lies close
    # enough to zero to be gated differently -- and ONE such element moves its channel's sum(dz) by ~1.5 % of the sum (these zero-mean test
    # tensors cancel to 1 % of their terms): 6e-4 of the input gradient for a forward that is closer to float64 than before (round 6: it
    # happened with the bf16x3 F(4x4,3x3) kernel on the 2 x 64 x 64 x 128 case).  With the same mask the gradients are functions of the data only.
    assert int((mask1 != (zpre.detach() > 0)).sum()) <= 2 + 2e-6 * mask1.numel()
    zb = zpre * mask1.to(zpre.dtype)
    oo = R.conv(zb, to['wb'], None, 1, 0)
    oo.backward(torch.from_numpy(gy))
    assert rel_l2(o1, t2n(oo)) < 1e-5
    # F(4x4,3x3)'s rounding error is input-correlated, and these zero-mean test tensors make the channel sums cancel to ~1 % of their terms:
    # the oracle bound is looser there; fused vs separate reduction on the SAME kernels is held tight either way
    tol = 2e-5 if f43 else 2e-6       # (measured: 3.3e-6 / 5.5e-7)
    for k_ in ('x', 'wa', 'wb', 'ga', 'be'):
        assert rel_l2(g1[k_], t2n(to[k_].grad)) < tol, (k_, rel_l2(g1[k_], t2n(to[k_].grad)))
        assert rel_l2(g1[k_], g0[k_]) < 2e-5, (k_, rel_l2(g1[k_], g0[k_]))


@pytest.mark.parametrize('b,h,w,c,pooled', [(2, 16, 16, 8, True), (3, 10, 14, 12, True), (2, 7, 9, 4, True), (2, 8, 8, 16, False)])
def test_vgg_feature_gradient_in_one_pass_equals_the_four_pass_chain(kpx, dev, b, h, w, c, pooled):
    """kpx_vgg_feat_bwd_f32 = ReLU backward of (max-pool backward + L1 backward), bit for bit against the separate kernels it replaces
    (kpx_maxpool2_bwd_f32, kpx_l1_pair_bwd_f32, the sum, the ReLU mask), ties (equal window maxima, zero differences, y = 0) included."""
    from kpx_amd._lib import lib, check
    ops = kpx.ops
    rs = np.random.RandomState(b * 100 + h)
    f = np.maximum(rs.randn(2 * b, h, w, c), 0).astype(np.float32)          # post-ReLU features: many exact zeros
    f[b:][rs.rand(b, h, w, c) < 0.2] = 0.5                                   # equal maxima inside windows
    f[0, 0, 0, :] = f[b, 0, 0, :]                                            # pred == gt: zero L1 gradient
    ho, wo = (h + 1) // 2, (w + 1) // 2
    fg = torch.from_numpy(f).to(dev)
    gdev = torch.tensor([0.7], dtype=torch.float32, device=dev)
    half = b * h * w * c
    got = torch.empty(b, h, w, c, device=dev)
    dyp = torch.from_numpy(rs.randn(b, ho, wo, c).astype(np.float32)).to(dev) if pooled else None
    check(lib.kpx_vgg_feat_bwd_f32(fg.data_ptr(), half, gdev.data_ptr(), 0.125, dyp.data_ptr() if pooled else None, b, h, w, c, got.data_ptr(), ops._stream()), 'fused')
    dl = torch.empty(b, h, w, c, device=dev)
    check(lib.kpx_l1_pair_bwd_f32(fg.data_ptr(), half, gdev.data_ptr(), 0.125, dl.data_ptr(), ops._stream()), 'l1')
    if pooled:
        dx = torch.empty(b, h, w, c, device=dev)
        check(lib.kpx_maxpool2_bwd_f32(dyp.data_ptr(), fg[b:].contiguous().data_ptr(), b, h, w, c, dx.data_ptr(), ops._stream()), 'pool')
        want = dx + dl
    else:
        want = dl
    want = torch.where(fg[b:] > 0, want, torch.zeros_like(want))
    assert torch.equal(got, want)


GEMM3_CASES = [  # n, h, w, cin, cout, k, stride, pad, act
    (4, 34, 34, 128, 256, 4, 2, 1, 2),      # img_discr conv_2 geometry
    (8, 65, 65, 64, 128, 4, 2, 1, 2),       # img_discr conv_1: SAME split (1, 2)
    (16, 6, 6, 1024, 2048, 4, 2, 1, 2),     # img_discr conv_5: small M, K = 16384 (split-K slabs + reduce)
    (4, 64, 64, 64, 128, 3, 2, 0, 0),       # encoder conv_5: 3x3 stride 2, SAME pad (0, 1)
    (2, 32, 32, 32, 64, 3, 2, 0, 1),        # encoder conv_3, 64 produced channels (BN = 64 tiles)
    (2, 64, 64, 16, 16, 1, 1, 0, 0),        # 1x1, half a K chunk, 16 produced channels
    (3, 17, 13, 40, 72, 3, 2, 0, 2),        # ragged: K = 40 (a partial chunk), 72 couts (masked tile columns), odd image sizes
    (2, 20, 20, 24, 20, 3, 1, 1, 0),        # explicit pad on a stride-1 3x3 (not the Winograd geometry), 20 couts
    (64, 18, 18, 256, 512, 4, 2, 1, 2),     # img_discr conv_3 at the PROFILED launch: N = 64 = real + generated halves of the bench batch
    (64, 10, 10, 512, 1024, 4, 2, 1, 2),    # img_discr conv_4 at the bench batch (multi-round split-K launch)
]


@pytest.mark.parametrize('n,h,w,cin,cout,k,s,pad,act', GEMM3_CASES)
def test_gemm3_bf16x3_is_fp32_equivalent_against_float64(kpx, dev, n, h, w, cin, cout, k, s, pad, act):
    """csrc/conv_gemm3.hip: forward and data gradient on the bf16 matrix pipe with every fp32 operand split exactly into three bf16 terms.
    Admissible in the fp32 configuration only if it is as close to a FLOAT64 convolution as the fp32-MFMA kernel it replaces: both run
    here on the same inputs (KPX_NO_GEMM3 flips the library back), and the bf16x3 error may not exceed 1.5x the fp32 kernel's (+1e-7)."""
    from kpx_amd._lib import lib
    rs = np.random.RandomState(cin + 3 * cout + k)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    wt = (rs.randn(k, k, cin, cout) / np.sqrt(k * k * cin)).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    x64 = torch.from_numpy(x).double().requires_grad_(True); w64 = torch.from_numpy(wt).double().requires_grad_(True)
    z64 = R.conv(x64, w64, torch.from_numpy(b).double(), s, pad)
    gy = rs.randn(*z64.shape).astype(np.float32)
    z64.backward(torch.from_numpy(gy).double())
    errs = {}
    for mode in ('gemm3', 'fp32'):
        if mode == 'fp32':
            os.environ['KPX_NO_GEMM3'] = '1'
        lib.kpx_reload_env()
        try:
            xg = torch.from_numpy(x).to(dev).requires_grad_(True); wg = torch.from_numpy(wt).to(dev).requires_grad_(True); bg = torch.from_numpy(b).to(dev)
            zg = kpx.ops.conv2d(xg, wg, bg, stride=s, pad=pad, act=0)
            zg.backward(torch.from_numpy(gy).to(dev))
            kpx.ops.join_side_stream()
            errs[mode] = (rel_l2(t2n(zg), t2n(z64)), rel_l2(t2n(xg.grad), t2n(x64.grad)), rel_l2(t2n(wg.grad), t2n(w64.grad)))
        finally:
            os.environ.pop('KPX_NO_GEMM3', None)
            lib.kpx_reload_env()
    print('conv %s: rel-L2 vs float64 fwd %.2e (fp32 MFMA %.2e), dgrad %.2e (fp32 MFMA %.2e), wgrad %.2e (fp32 MFMA %.2e)'
          % ((n, h, w, cin, cout, k, s), errs['gemm3'][0], errs['fp32'][0], errs['gemm3'][1], errs['fp32'][1], errs['gemm3'][2], errs['fp32'][2]))
    for i in (0, 1, 2):
        assert errs['gemm3'][i] <= 1.5 * errs['fp32'][i] + 1e-7, (i, errs)
        assert errs['gemm3'][i] < 2e-6
    assert errs['gemm3'][:2] != errs['fp32'][:2]          # the two kernels really are different code paths


@pytest.mark.parametrize('n,h,w,c,groups,with_tiles', [(4, 16, 16, 32, 2, False), (6, 8, 8, 20, 3, False), (4, 32, 32, 64, 2, True), (2, 16, 16, 6, 1, False),
                                                       (4, 8, 8, 6, 2, False)])          # ragged C with groups > 1: the scalar kernels' blockIdx.z
def test_batched_batch_norm_equals_one_call_per_group_bit_for_bit(kpx, dev, n, h, w, c, groups, with_tiles):
    """kpx_bn_train_fwd / _bwd (all weight-sharing calls of a batch in one launch per phase, a finalize workgroup per channel looping over the
    groups) against `groups` calls of the same entries with groups = 1, one per slice: same partial sums in the same order, so every output --
    y, mean, invstd, the moving statistics after the in-order updates, dx, dgamma, dbeta -- must be identical bit for bit.  The fp32 entries
    for every shape, the bf16 entries where C % 8 == 0."""
    from kpx_amd._lib import lib, check
    from kpx_amd import ops
    rs = np.random.RandomState(c + groups)
    x32 = torch.from_numpy(rs.randn(n, h, w, c).astype(np.float32)).to(dev)
    dy32 = torch.from_numpy(rs.randn(n, h, w, c).astype(np.float32)).to(dev)
    gamma = torch.from_numpy((rs.rand(c) + 0.5).astype(np.float32)).to(dev); beta = torch.from_numpy(rs.randn(c).astype(np.float32)).to(dev)
    ng, pix, st = n // groups, (n // groups) * h * w, ops._stream()
    for dt in (torch.float32, torch.bfloat16) if c % 8 == 0 else (torch.float32,):
        bf16 = dt == torch.bfloat16
        x, dy = x32.to(dt), dy32.to(dt)
        slab, tpi = None, 0
        if with_tiles:                                     # per-tile sums as a convolution epilogue would deliver them: 16x16-pixel tiles
            tiles = x.float().reshape(n, h // 16, 16, w // 16, 16, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, 256, c)
            slab = torch.stack([tiles.sum(1), (tiles * tiles).sum(1)], dim=1).contiguous()
            tpi = (h // 16) * (w // 16)
        out = {}
        for mode in ('per_group', 'batched'):
            mm, mv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
            mean, invstd = torch.empty(groups, c, device=dev), torch.empty(groups, c, device=dev)
            y, dx = torch.empty_like(x), torch.empty_like(x)
            dg, db = torch.full((c,), 7.0, device=dev), torch.full((c,), -3.0, device=dev)
            sc = ops.scratch.get('bn_test', lib.kpx_bn_train_scratch_bytes(c, groups), dev).data_ptr()
            calls = [(g, 1) for g in range(groups)] if mode == 'per_group' else [(0, groups)]      # (first group, groups) per call
            for g, k in calls:
                sl = slice(g * ng, (g + k) * ng)
                args = (x[sl].data_ptr(), pix, k, c, c, slab[g * ng * tpi:].data_ptr() if slab is not None else None, ng * tpi, 1e-5,
                        gamma.data_ptr(), beta.data_ptr(), mean[g].data_ptr(), invstd[g].data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.999, y[sl].data_ptr(), c)
                if bf16:
                    check(lib.kpx_bn_train_fwd_bf16(*args, 0, 1, sc, st), 'train_fwd_bf16')
                else:
                    check(lib.kpx_bn_train_fwd_f32(*args, 1, sc, st), 'train_fwd')
            for g, k in calls:
                sl = slice(g * ng, (g + k) * ng)
                args = (x[sl].data_ptr(), c, pix, k, c, mean[g].data_ptr(), invstd[g].data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1,
                        dx[sl].data_ptr(), c, dg.data_ptr(), db.data_ptr(), 1, None, 0, sc, st)
                if bf16:
                    check(lib.kpx_bn_train_bwd_bf16(dy[sl].data_ptr(), c, 0, *args), 'train_bwd_bf16')
                else:
                    check(lib.kpx_bn_train_bwd_f32(dy[sl].data_ptr(), c, *args), 'train_bwd')
            torch.cuda.synchronize()
            out[mode] = [t2n(t.float()).copy() for t in (y, mean, invstd, mm, mv, dx, dg, db)]
        for a, b, name in zip(out['per_group'], out['batched'], ('y', 'mean', 'invstd', 'moving_mean', 'moving_var', 'dx', 'dgamma', 'dbeta')):
            assert np.array_equal(a, b), (dt, name)


@pytest.mark.parametrize('n,h,c0,c1,c2,k,s,pad', [(4, 34, 16, 64, 128, 4, 2, 1),        # img_discr-shaped: 4x4 stride 2, implicit-GEMM kernels
                                                  (8, 10, 64, 256, 512, 4, 2, 1),       # small maps: the split-K data gradient + its reduce
                                                  (2, 6, 32, 48, 1, 3, 1, 1),           # D_logit-shaped: one produced channel (scalar-store kernel)
                                                  (2, 32, 16, 16, 32, 3, 1, 0)])        # 3x3 stride 1 on the specialised kernels: the extra pass over dx
def test_activation_backward_in_the_data_gradient_epilogue_equals_the_separate_pass(kpx, dev, n, h, c0, c1, c2, k, s, pad):
    """conv -> leaky_relu -> conv (reference networks/__init__.py:141-151) walked backwards: with act_bwd_by_consumer / input_act the
    leaky-ReLU backward of the first layer is applied in the epilogue of the second layer's data gradient (kpx_conv2d_dgrad_act_f32);
    every gradient must equal the separate kpx_act_bwd_f32 pass bit for bit (the same multiplication on the same sums)."""
    from kpx_amd import ops
    rs = np.random.RandomState(n + h + c1)
    x = rs.randn(n, h, h, c0).astype(np.float32)
    w1 = (rs.randn(k, k, c0, c1) / np.sqrt(k * k * c0)).astype(np.float32); b1 = rs.randn(c1).astype(np.float32)
    w2 = (rs.randn(k, k, c1, c2) / np.sqrt(k * k * c1)).astype(np.float32)
    outs = {}
    for fused in (False, True):
        xg = torch.from_numpy(x).to(dev).requires_grad_(True)
        w1g = torch.from_numpy(w1).to(dev).requires_grad_(True); b1g = torch.from_numpy(b1).to(dev).requires_grad_(True)
        w2g = torch.from_numpy(w2).to(dev).requires_grad_(True)
        y1 = ops.conv2d(xg, w1g, b1g, stride=s, pad=pad, act=ops.ACT_LRELU, act_bwd_by_consumer=fused)
        y2 = ops.conv2d(y1, w2g, None, stride=s, pad=pad, act=ops.ACT_NONE, input_act=ops.ACT_LRELU if fused else ops.ACT_NONE)
        if fused:
            assert y2.grad_fn.input_act == ops.ACT_LRELU and y1.grad_fn.act_bwd_by_consumer
        gy = torch.from_numpy(np.random.RandomState(7).randn(*y2.shape).astype(np.float32)).to(dev)
        y2.backward(gy)
        ops.join_side_stream()
        outs[fused] = [t2n(t) for t in (y2, xg.grad, w1g.grad, b1g.grad, w2g.grad)]
    for a, b in zip(outs[False], outs[True]):
        assert np.array_equal(a, b)
    # and against the float64 restatement (the unfused path is covered elsewhere; this pins the fused one directly)
    x64 = torch.from_numpy(x).double().requires_grad_(True); w164 = torch.from_numpy(w1).double().requires_grad_(True)
    z1 = R.conv(x64, w164, torch.from_numpy(b1).double(), s, pad)
    z2 = R.conv(torch.where(z1 > 0, z1, 0.01 * z1), torch.from_numpy(w2).double(), None, s, pad)
    z2.backward(torch.from_numpy(np.random.RandomState(7).randn(*z2.shape).astype(np.float32)).double())
    assert rel_l2(outs[True][1], t2n(x64.grad)) < 1e-5 and rel_l2(outs[True][2], t2n(w164.grad)) < 1e-5
