"""Stage-2 (motion generator) ops at the reference's sizes against float64.

The dense layers and LSTM gate GEMMs of stage 2 run as 1x1 "convolutions" over [rows,1,1,In]; at the reference's sizes (K=40 or 15
key-points, LSTM cells 1024, vae_dim 64, batch 16) they reach split-K, tanh-in-the-reduce, non-vector and small-Cout paths that the toy
model never does.  Every case here is compared with a float64 restatement; the LSTM layer also with a CPU fp32 one.

Bounds (fixed before measuring): GEMMs rel-L2 < 1e-5 against float64 on every output (this suite's conv bar), bf16x3 error <= 1.5x the
fp32-MFMA error + 1e-7; LSTM layer over T=32 steps: hs rel-L2 < 1e-5, gradients < 1e-4, and each at most 4x the CPU fp32 restatement's
error + 1e-7; pointwise kernels: 16 fp32 ulps of the magnitudes involved.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


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


# rows, In, Out, act, gemm3 expected somewhere in fwd / dgrad / wgrad
DENSE_CASES = [
    (16, 1104, 4096, 0, True),      # LSTM gates, encoder layer 0 at K=40 (In = 80 + 1024): split-K forward
    (16, 2048, 4096, 0, True),      # LSTM gates, layer 1 (and seq_discr layer 1 in the G-run)
    (32, 2048, 4096, 0, True),      # seq_discr layer 1 in the D-run (real + fake: B = 32)
    (32, 1104, 4096, 0, True),      # seq_discr layer 0 in the D-run
    (3, 1054, 4096, 0, False),      # LSTM gates at K=15 (In = 30 + 1024, pixel stride % 4 == 2): non-vector kernels
    (3, 2048, 4096, 0, True),       # LSTM gates, layer 1 at B=3
    (512, 2048, 4096, 0, True),     # the LSTM weight gradient shape: one GEMM over T*B = 512 rows
    (1024, 2048, 4096, 0, True),    # ... and over T*2B = 1024 rows (seq_discr in the D-run)
    (512, 1024, 80, 3, True),       # to_coord (tanh) at K=40 over T*B rows: split-K, tanh in the reduce
    (96, 1024, 30, 3, False),       # to_coord at K=15, B=3: 30 outputs, tanh in the epilogue
    (16, 1113, 128, 1, False),      # vae_encoder fully_connected (ReLU), K=40
    (3, 1063, 128, 1, False),       # ... K=15
    (16, 153, 32, 1, False),        # vae_decoder fully_connected (ReLU), K=40
    (3, 103, 32, 1, False),         # ... K=15
    (16, 1024, 1, 1, False),        # seq_discr fully_connected -> 1 (ReLU), G-run: small-Cout kernel
    (32, 1024, 1, 1, False),        # ... D-run
]


@pytest.mark.parametrize('m,k,n,act,g3', DENSE_CASES)
def test_stage2_dense_gemms_against_float64(kpx, dev, m, k, n, act, g3):
    """ops.dense_train forward, data, weight and bias gradient; once on the bf16x3 kernels, once with KPX_NO_GEMM3 (fp32 MFMA)."""
    from kpx_amd._lib import lib
    rs = np.random.RandomState(m + 7 * k + 3 * n + act)
    x = rs.randn(m, k).astype(np.float32)
    w = (rs.randn(k, n) / np.sqrt(k)).astype(np.float32)
    b = (rs.randn(n) * 0.5).astype(np.float32)
    gy = rs.randn(m, n).astype(np.float32)
    z64 = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    y64 = {0: z64, 1: np.maximum(z64, 0), 3: np.tanh(z64)}[act]
    errs, flips = {}, {}
    for mode in ('gemm3', 'fp32'):
        if mode == 'fp32':
            os.environ['KPX_NO_GEMM3'] = '1'
        lib.kpx_reload_env()
        try:
            xg = torch.from_numpy(x).to(dev).requires_grad_(True)
            wg = torch.from_numpy(w).to(dev).requires_grad_(True)
            bg = torch.from_numpy(b).to(dev).requires_grad_(True)
            yg = kpx.ops.dense_train(xg, wg, bg, act=act)
            yg.backward(torch.from_numpy(gy).to(dev))
            kpx.ops.join_side_stream()
            y = t2n(yg)
            if act == 1:
                # the ReLU mask of the backward is the kernel's own (y > 0); elements within rounding of 0 may fall either side
                pos = y > 0
                flips[mode] = int((pos != (z64 > 0)).sum())
                dz = gy * pos
            elif act == 3:
                dz = gy * (1.0 - np.tanh(z64) ** 2)
            else:
                dz = gy.astype(np.float64)
            dz = dz.astype(np.float64)
            want = (y64, dz @ w.astype(np.float64).T, x.astype(np.float64).T @ dz, dz.sum(0))
            errs[mode] = tuple(rel_l2(g, wv) for g, wv in zip((y, t2n(xg.grad), t2n(wg.grad), t2n(bg.grad)), want))
        finally:
            os.environ.pop('KPX_NO_GEMM3', None)
            lib.kpx_reload_env()
    print('dense %s act %d: rel-L2 vs float64  fwd %.2e (fp32 MFMA %.2e)  dgrad %.2e (%.2e)  wgrad %.2e (%.2e)  bias %.2e (%.2e)%s'
          % ((m, k, n), act, errs['gemm3'][0], errs['fp32'][0], errs['gemm3'][1], errs['fp32'][1], errs['gemm3'][2], errs['fp32'][2],
             errs['gemm3'][3], errs['fp32'][3], '  relu flips %s' % flips if act == 1 else ''))
    for i in range(4):
        assert errs['gemm3'][i] <= 1.5 * errs['fp32'][i] + 1e-7, (i, errs)
        assert errs['gemm3'][i] < 1e-5 and errs['fp32'][i] < 1e-5, (i, errs)
    if act == 1:
        assert max(flips.values()) <= 2 + 1e-5 * m * n, flips
    if g3:
        assert errs['gemm3'][:3] != errs['fp32'][:3]          # the two kernels really are different code paths


# ----------------------------------------------------------------------------------------------- LstmLayerFn over T=32
def _lstm_ref(x, kernel, bias, dhs, want_dx=True):
    """Autograd restatement of a zero-state LSTMCell layer over x [T,B,In] in the dtype of the inputs -> (hs, dx, dW, db)."""
    x = x.clone().requires_grad_(want_dx)
    kernel = kernel.clone().requires_grad_(True)
    bias = bias.clone().requires_grad_(True)
    t, bsz, _ = x.shape
    u = kernel.shape[1] // 4
    h = torch.zeros(bsz, u, dtype=x.dtype)
    c = torch.zeros(bsz, u, dtype=x.dtype)
    hs = []
    for s in range(t):
        i, j, f, o = torch.split(torch.cat([x[s], h], dim=1) @ kernel + bias, u, dim=1)
        c = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
        h = torch.tanh(c) * torch.sigmoid(o)
        hs.append(h)
    hs = torch.stack(hs)
    hs.backward(dhs)
    return hs.detach(), (x.grad if want_dx else None), kernel.grad, bias.grad


def _lstm_inputs(rs, t, bsz, n_in, u):
    lim = np.sqrt(6.0 / (n_in + 5 * u))                         # glorot_uniform of the [In+U, 4U] kernel
    x = rs.uniform(-1, 1, size=(t, bsz, n_in)).astype(np.float32)
    kernel = rs.uniform(-lim, lim, size=(n_in + u, 4 * u)).astype(np.float32)
    bias = (rs.randn(4 * u) * 0.1).astype(np.float32)
    dhs = rs.randn(t, bsz, u).astype(np.float32)
    return x, kernel, bias, dhs


@pytest.mark.parametrize('bsz,n_in,u,x_grad', [(16, 80, 1024, True), (32, 1024, 1024, True), (3, 30, 1024, True), (5, 7, 13, True),
                                               (16, 80, 1024, False)])
def test_lstm_layer_over_32_steps_against_float64(kpx, dev, bsz, n_in, u, x_grad):
    """ops.lstm_layer (kpx_lstm_layer_fwd/bwd_f32 + the one weight-gradient GEMM over T*B rows) against float64 autograd; x_grad=False
    is the dx = NULL branch of the backward (the encoder's and seq_discr's first layer read data, not a gradient-carrying tensor)."""
    t = 32
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    rs = np.random.RandomState(bsz * 100 + n_in + u)
    x, kernel, bias, dhs = _lstm_inputs(rs, t, bsz, n_in, u)
    ref64 = _lstm_ref(*(torch.from_numpy(a).double() for a in (x, kernel, bias, dhs)), want_dx=x_grad)
    ref32 = _lstm_ref(*(torch.from_numpy(a) for a in (x, kernel, bias, dhs)), want_dx=x_grad)
    xg = torch.from_numpy(x).to(dev).requires_grad_(x_grad)
    kg = torch.from_numpy(kernel).to(dev).requires_grad_(True)
    bg = torch.from_numpy(bias).to(dev).requires_grad_(True)
    kpx.ops.begin_backward()
    hs = kpx.ops.lstm_layer(xg, kg, bg)
    hs.backward(torch.from_numpy(dhs).to(dev))
    got = (t2n(hs), t2n(xg.grad) if x_grad else None, t2n(kg.grad), t2n(bg.grad))
    assert (xg.grad is None) == (not x_grad)
    names = ('hs', 'dx', 'dW', 'db')
    rep = []
    for i, name in enumerate(names):
        if got[i] is None:
            continue
        e_gpu, e_cpu = rel_l2(got[i], ref64[i].numpy()), rel_l2(ref32[i].numpy(), ref64[i].numpy())
        rep.append('%s %.2e (CPU fp32 %.2e)' % (name, e_gpu, e_cpu))
        assert e_gpu < (1e-5 if name == 'hs' else 1e-4), (name, e_gpu)
        assert e_gpu <= 4 * e_cpu + 1e-7, (name, e_gpu, e_cpu)
    print('lstm_layer T=%d B=%d In=%d U=%d: rel-L2 vs float64  %s' % (t, bsz, n_in, u, '  '.join(rep)))


def test_lstm_layer_accumulates_into_a_claimed_gradient_destination(kpx, dev):
    """w_grad_out / b_grad_out: written directly when first claimed in the backward epoch, added to (axpy) when already claimed."""
    t, bsz, n_in, u = 32, 4, 24, 64
    rs = np.random.RandomState(3)
    x, kernel, bias, dhs = _lstm_inputs(rs, t, bsz, n_in, u)
    ref = _lstm_ref(*(torch.from_numpy(a).double() for a in (x, kernel, bias, dhs)), want_dx=False)
    g0w = rs.randn(n_in + u, 4 * u).astype(np.float32)
    g0b = rs.randn(4 * u).astype(np.float32)
    for claimed in (False, True):
        wbuf = torch.from_numpy(g0w).to(dev)
        bbuf = torch.from_numpy(g0b).to(dev)
        kg = torch.from_numpy(kernel).to(dev).requires_grad_(True)
        bg = torch.from_numpy(bias).to(dev).requires_grad_(True)
        kpx.ops.begin_backward()
        if claimed:                       # another op already wrote this variable's gradient in this backward pass
            assert kpx.ops._claim_grad(wbuf) and kpx.ops._claim_grad(bbuf)
        hs = kpx.ops.lstm_layer(torch.from_numpy(x).to(dev), kg, bg, w_grad_out=wbuf, b_grad_out=bbuf)
        hs.backward(torch.from_numpy(dhs).to(dev))
        assert kg.grad is None and bg.grad is None          # the gradients went to the destinations only
        base_w, base_b = (g0w, g0b) if claimed else (0.0, 0.0)
        assert rel_l2(t2n(wbuf) - base_w, ref[2].numpy()) < 1e-5, claimed
        assert rel_l2(t2n(bbuf) - base_b, ref[3].numpy()) < 1e-5, claimed


# ----------------------------------------------------------------------------------------------- pointwise kernels through the C ABI
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _gates(rs, bsz, u):
    g = rs.randn(bsz, 4 * u) * 6.0
    g[:, ::7] = 40.0                                          # saturated gates, both signs
    g[:, 3::11] = -40.0
    g[:, 5::13] = rs.uniform(-40, 40, size=g[:, 5::13].shape)
    return g.astype(np.float32)


@pytest.mark.parametrize('bsz,u', [(16, 1024), (3, 13), (517, 1031)])        # 517 * 1031 > 2048 * 256: the grid-stride loop
def test_lstm_pointwise_fwd_bwd_against_float64(kpx, dev, bsz, u):
    from kpx_amd._lib import lib
    rs = np.random.RandomState(bsz + u)
    gates = _gates(rs, bsz, u)
    c_prev = (rs.randn(bsz, u) * 2).astype(np.float32)
    dh = rs.randn(bsz, u).astype(np.float32)
    dc_in = rs.randn(bsz, u).astype(np.float32)
    fb = 1.0
    g64, cp64 = gates.astype(np.float64), c_prev.astype(np.float64)
    i, j, f, o = (g64[:, q * u:(q + 1) * u] for q in range(4))
    si, sf, so, tj = _sig(i), _sig(f + fb), _sig(o), np.tanh(j)
    stream = torch.cuda.current_stream(dev).cuda_stream
    G = torch.from_numpy(gates).to(dev)
    # forward (c_prev = NULL is refused: the layer always passes a zero state)
    c_out = torch.empty(bsz, u, device=dev); h_out = torch.empty(bsz, u, device=dev)
    assert lib.kpx_lstm_pointwise_f32(G.data_ptr(), None, fb, c_out.data_ptr(), h_out.data_ptr(), bsz, u, stream) == -1
    CP = torch.from_numpy(c_prev).to(dev)
    assert lib.kpx_lstm_pointwise_f32(G.data_ptr(), CP.data_ptr(), fb, c_out.data_ptr(), h_out.data_ptr(), bsz, u, stream) == 0
    c64 = cp64 * sf + si * tj
    h64 = np.tanh(c64) * so
    torch.cuda.synchronize(dev)
    assert np.all(np.abs(t2n(c_out) - c64) <= 16 * EPS32 * (np.abs(cp64 * sf) + np.abs(si * tj) + 1e-30))
    assert np.all(np.abs(t2n(h_out) - h64) <= 16 * EPS32 * (np.abs(h64) + np.abs(cp64 * sf) + np.abs(si * tj)) + 1e-30)
    # backward: with / without c_prev, with / without dc_in
    DH, DC = torch.from_numpy(dh).to(dev), torch.from_numpy(dc_in).to(dev)
    for with_c, with_dc in ((True, True), (False, True), (True, False), (False, False)):
        cp = cp64 if with_c else np.zeros_like(cp64)
        c = cp * sf + si * tj
        tc = np.tanh(c)
        dct = (dc_in if with_dc else 0.0) + dh * so * (1 - tc * tc)
        want = np.concatenate([dct * tj * si * (1 - si), dct * si * (1 - tj * tj), dct * cp * sf * (1 - sf), dh * tc * so * (1 - so)], 1)
        want_dcp = dct * sf
        dg = torch.full((bsz, 4 * u), np.nan, device=dev); dcp = torch.full((bsz, u), np.nan, device=dev)
        rc = lib.kpx_lstm_pointwise_bwd_f32(G.data_ptr(), CP.data_ptr() if with_c else None, DH.data_ptr(), DC.data_ptr() if with_dc else None,
                                            fb, dg.data_ptr(), dcp.data_ptr(), bsz, u, stream)
        assert rc == 0
        torch.cuda.synchronize(dev)
        # scale of each term: |dct| (|dh| + |dc_in| bounds it) times the magnitude of the factors
        mag = np.abs(dh) + (np.abs(dc_in) if with_dc else 0.0)
        tol = 16 * EPS32 * np.concatenate([mag, mag, mag * (1 + np.abs(cp)), mag], 1) + 1e-30
        err = np.abs(t2n(dg) - want)
        assert np.all(err <= tol), (with_c, with_dc, float((err / tol).max()))
        assert np.all(np.abs(t2n(dcp) - want_dcp) <= 16 * EPS32 * mag + 1e-30), (with_c, with_dc)


@pytest.mark.parametrize('bsz,v', [(7, 53), (16, 64), (3, 64), (2, 5)])          # 371 = B*V > 256 and not a multiple of 256
def test_vae_sample_kl_fwd_bwd_against_float64(kpx, dev, bsz, v):
    from kpx_amd._lib import lib
    rs = np.random.RandomState(bsz * v)
    mu = np.maximum(rs.randn(bsz, v), 0).astype(np.float32)
    sd = np.abs(rs.randn(bsz, v)).astype(np.float32)
    sd.flat[::5] = 0.0                                           # the encoder's ReLU: exact zeros
    sd.flat[1::7] = 1e-6                                         # tiny: d kl / d s ~ -1/s
    sd.flat[2::11] = 40.0                                        # large
    eps = rs.randn(bsz, v).astype(np.float32)
    dz = rs.randn(bsz, v).astype(np.float32)
    logit = np.concatenate([mu, sd], 1)
    m64, s64, e64, dz64 = (a.astype(np.float64) for a in (mu, sd, eps, dz))
    stream = torch.cuda.current_stream(dev).cuda_stream
    L, E, DZ = (torch.from_numpy(a).to(dev) for a in (logit, eps, dz))
    z = torch.full((bsz, v), np.nan, device=dev); kl = torch.full((1,), np.nan, device=dev)
    assert lib.kpx_vae_sample_kl_fwd_f32(L.data_ptr(), E.data_ptr(), z.data_ptr(), kl.data_ptr(), bsz, v, stream) == 0
    z64 = m64 + s64 * e64
    terms = m64 ** 2 + s64 ** 2 - np.log(1e-8 + s64 ** 2) - 1
    kl64 = 0.5 * terms.sum() / bsz
    parts = m64 ** 2 + s64 ** 2 + np.abs(np.log(1e-8 + s64 ** 2)) + 1              # each term is summed in fp32, the terms in double
    torch.cuda.synchronize(dev)
    assert np.all(np.abs(t2n(z) - z64) <= EPS32 * np.abs(z64) + 1e-30)                     # one fused multiply-add: correctly rounded
    assert abs(float(t2n(kl)[0]) - kl64) <= 4 * EPS32 * 0.5 * parts.sum() / bsz
    gk_dev = torch.tensor([2.5], device=dev)
    for use_dz, use_dev, host in ((True, True, 1.0), (False, True, 1.0), (True, False, 0.7), (False, False, 1.3)):
        gk = host * (2.5 if use_dev else 1.0) / bsz
        d = dz64 if use_dz else 0.0
        want_mu = d + gk * m64
        want_sd = d * e64 + gk * (s64 - s64 / (1e-8 + s64 * s64))
        dl = torch.full((bsz, 2 * v), np.nan, device=dev)
        rc = lib.kpx_vae_sample_kl_bwd_f32(L.data_ptr(), E.data_ptr(), DZ.data_ptr() if use_dz else None, gk_dev.data_ptr() if use_dev else None,
                                           host, dl.data_ptr(), bsz, v, stream)
        assert rc == 0
        torch.cuda.synchronize(dev)
        got = t2n(dl)
        scale_mu = np.abs(d) + abs(gk) * np.abs(m64)
        scale_sd = np.abs(d * e64) + abs(gk) * (np.abs(s64) + np.abs(s64 / (1e-8 + s64 * s64)))
        assert np.all(np.abs(got[:, :v] - want_mu) <= 8 * EPS32 * scale_mu + 1e-30), (use_dz, use_dev)
        assert np.all(np.abs(got[:, v:] - want_sd) <= 8 * EPS32 * scale_sd + 1e-30), (use_dz, use_dev)
