"""Stage-2 training (MotionGeneratorModel) against the CPU restatement (oracle.motion_train_step) on a small configuration."""
import os

import numpy as np
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu
K, A, CELLS, VAE, DISCR = 5, 9, (32, 32), 8, (32, 32)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _make(dev, k=K, cells=CELLS, vae=VAE, discr=DISCR, b=3):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': b},
           'model': {'n_pts': k, 'n_action': A, 'cell_info': list(cells), 'vae_dim': vae}, 'paths': {'log_dir': '/tmp/kpx_motion'}}
    model = kpx_amd.MotionGeneratorModel(cfg, device=dev, discr_cells=discr)
    model.build()
    return model


def test_manifest_and_train_steps_match_oracle():
    dev = torch.device('cuda:0')
    model = _make(dev)
    manifest = R.motion_generator_manifest(K, A, CELLS, VAE, DISCR)
    assert {n: tuple(model.store.vars[n].shape) for n in model.store.vars} == {n: tuple(s) for n, s in manifest.items()}
    params = R.init_motion_generator(K, A, CELLS, VAE, DISCR, seed=5)
    model.store.load_numpy(params, strict=True)
    st = R.MotionTrainState(params, K, A, CELLS, VAE, DISCR)
    rs = np.random.RandomState(1)
    b = 3
    for step in range(2):
        kp = (rs.rand(b, K, 2) * 1.6 - 0.8).astype(np.float32)
        seq = (rs.rand(b, 32, K, 2) * 1.6 - 0.8).astype(np.float32)
        ac = np.eye(A, dtype=np.float32)[rs.randint(0, A, size=b)]
        e_d, e_g = rs.randn(b, VAE).astype(np.float32), rs.randn(b, VAE).astype(np.float32)
        want = R.motion_train_step(st, kp, seq, ac, e_d, e_g)
        feed = {k: torch.from_numpy(v).to(dev) for k, v in dict(keypoints=kp, real_seq=seq, action_code=ac, eps_D=e_d, eps_G=e_g).items()}
        model.train_step(None, feed, step, b)
        got = model.loss_values()
        for key in ('loss_D', 'loss_G', 'loss_G_recon', 'loss_G_kl', 'loss_G_adv'):
            assert abs(got[key] - want[key]) <= 2e-5 * max(1.0, abs(want[key])), (step, key, got[key], want[key])
        assert rel_l2(model.last['pred_seq'].cpu().numpy(), want['pred_seq'].numpy()) < 1e-5
        # gradients of the G bucket still hold this step's values
        for n, g in want['grads_G'].items():
            if float(g.abs().max()) > 1e-7:
                assert rel_l2(model.store.grad(n).cpu().numpy(), g.numpy()) < 2e-4, (step, n)
        # the G-run freezes seq_discr (no gradient destination), so the D bucket still holds the D-run's gradients
        assert set(want['grads_D']) == {n for n in model.store.vars if 'discr' in n}
        for n, g in want['grads_D'].items():
            if float(g.abs().max()) > 1e-7:
                assert rel_l2(model.store.grad(n).cpu().numpy(), g.numpy()) < 2e-4, (step, n)
        # parameters after Adam: elements whose gradient is rounding noise may flip sign (+-lr), like in stage 1
        exp = model.store.export_numpy(include_slots=False)
        for n, p in st.params.items():
            diff = np.abs(exp[n] - p.numpy())
            assert diff.max() <= (step + 1) * 2.05e-4 and np.mean(diff > 1e-5) < 0.02, (step, n, float(diff.max()), float(np.mean(diff > 1e-5)))


def test_checkpoint_names_and_sampling():
    dev = torch.device('cuda:0')
    model = _make(dev)
    arrays = model.checkpoint_arrays()
    for name in ('vae_encoder/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel', 'vae_encoder/fully_connected/weights',
                 'vae_decoder/multi_rnn_cell/cell_1/basic_lstm_cell/bias', 'vae_decoder/fully_connected/W', 'seq_discr/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel',
                 'seq_discr/fully_connected/biases', 'seq_discr/fully_connected/weights/Adam', 'vae_decoder/fully_connected/b/Adam_1', 'global_step', 'beta2_power_1'):
        assert name in arrays, name
    assert np.asarray(arrays['global_step']).dtype == np.int32      # tf.Variable(0) (reference train.py:30) is DT_INT32
    kp = torch.rand(4, K, 2, device=dev) * 1.6 - 0.8
    ac = torch.eye(A, device=dev)[:4].contiguous()
    z = torch.randn(4, VAE, device=dev)
    seq = model.sample(kp, ac, z)
    want = R.vae_decoder({k: torch.from_numpy(np.asarray(v)) for k, v in model.store.export_numpy(include_slots=False).items()},
                         z.cpu(), kp.reshape(4, -1).cpu(), ac.cpu(), CELLS, K)
    assert tuple(seq.shape) == (4, 32, 2 * K) and rel_l2(seq.cpu().numpy(), want.numpy()) < 1e-5


# ----------------------------------------------------------------------------------------------- the reference's sizes (configs/penn.yaml)
def _relu_inputs(p, kp, seq, ac, eps, k, cells, vae, discr, fake):
    """Pre-activations of the three ReLU'd fully_connected layers of one run of the restatement: encoder [B,2V], decoder [B,32],
    seq_discr logits of the real and the generated sequences [2B] (the dtype of ``p``)."""
    b = kp.shape[0]
    real = seq.reshape(b, 32, 2 * k)
    out = R._dynamic_rnn(p, 'vae_encoder/rnn', real, cells)
    enc = torch.cat([out[:, -1], kp.reshape(b, -1), ac], 1) @ p['vae_encoder/fully_connected/weights'] + p['vae_encoder/fully_connected/biases']
    z = torch.relu(enc[:, :vae]) + torch.relu(enc[:, vae:]) * eps
    dec = torch.cat([z, kp.reshape(b, -1), ac], 1) @ p['vae_decoder/fully_connected/weights'] + p['vae_decoder/fully_connected/biases']
    logits = [R._dynamic_rnn(p, 'seq_discr/rnn', x, discr)[:, -1] @ p['seq_discr/fully_connected/weights'] + p['seq_discr/fully_connected/biases']
              for x in (real, fake)]
    return enc, dec, torch.cat(logits).reshape(-1)


def _run_grads(p, names, kp, seq, ac, eps, k, cells, vae, discr, loss):
    p = {n: (t.clone().requires_grad_(True) if n in names else t) for n, t in p.items()}
    out = R.motion_generator_losses(p, kp, seq, ac, eps, k, cells, vae, discr)
    gs = torch.autograd.grad(out[loss], [p[n] for n in names])
    return {n: g.detach() for n, g in zip(names, gs)}, out


@pytest.mark.parametrize('k,b', [(40, 16), (15, 3)])
def test_reference_size_train_step_against_oracle_and_float64(k, b):
    """One stage-2 train step at configs/penn.yaml's sizes (2x LSTM 1024, vae_dim 64, seq_discr 2x 1024; K=40 at the batch 16 and
    K=15 at B=3, whose 30-wide rows take the non-vector kernels) against the fp32 oracle, as the toy test does, and a float64 arbiter:
    per variable the GPU's gradient error against float64 may be at most 4x the CPU fp32 oracle's + 2e-6.  The arbiter's G-run uses
    the discriminator the GPU's D-run produced (the G-run reads the updated D), so the only difference is arithmetic."""
    cells, vae, discr = (1024, 1024), 64, (1024, 1024)
    dev = torch.device('cuda:0')
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    model = _make(dev, k, cells, vae, discr, b)
    params = R.init_motion_generator(k, A, cells, vae, discr, seed=5)
    model.store.load_numpy(params, strict=True)
    rs = np.random.RandomState(1)
    kp = (rs.rand(b, k, 2) * 1.6 - 0.8).astype(np.float32)
    seq = (rs.rand(b, 32, k, 2) * 1.6 - 0.8).astype(np.float32)
    ac = np.eye(A, dtype=np.float32)[rs.randint(0, A, size=b)]
    e_d, e_g = rs.randn(b, vae).astype(np.float32), rs.randn(b, vae).astype(np.float32)
    st = R.MotionTrainState(params, k, A, cells, vae, discr)
    want = R.motion_train_step(st, kp, seq, ac, e_d, e_g)
    feed = {n: torch.from_numpy(v).to(dev) for n, v in dict(keypoints=kp, real_seq=seq, action_code=ac, eps_D=e_d, eps_G=e_g).items()}
    model.train_step(None, feed, 0, b)
    got = model.loss_values()
    grads = {n: model.store.grad(n).cpu().numpy() for n in list(want['grads_D']) + list(want['grads_G'])}
    exp = model.store.export_numpy(include_slots=False)

    # ---- float64 arbiter on this step
    d_names, g_names = list(want['grads_D']), list(want['grads_G'])
    args = {dt: tuple(torch.from_numpy(a).to(dt) for a in (kp, seq, ac)) for dt in (torch.float32, torch.float64)}
    cfg = (k, cells, vae, discr)
    p64 = {n: torch.from_numpy(v).double() for n, v in params.items()}
    g64_d, _ = _run_grads(p64, d_names, *args[torch.float64], torch.from_numpy(e_d).double(), *cfg, 'loss_D')
    p_g = {n: torch.from_numpy(exp[n] if n in d_names else params[n]) for n in params}          # G params before, D params after the D update
    g64_g, out64 = _run_grads({n: t.double() for n, t in p_g.items()}, g_names, *args[torch.float64], torch.from_numpy(e_g).double(), *cfg, 'loss_G')
    g32_g, _ = _run_grads(p_g, g_names, *args[torch.float32], torch.from_numpy(e_g), *cfg, 'loss_G')
    cpu32 = {**want['grads_D'], **g32_g}
    ref64 = {**g64_d, **g64_g}

    # ill-conditioned elements, reported rather than absorbed in a bound: ReLU inputs closer to zero than 100x the largest fp32 rounding
    # error of their layer (measured here: CPU fp32 vs float64), which two correct fp32 runs may put on either side of 0; and stddev > 0
    # near zero, where d kl / d stddev ~ -1/(B*stddev) amplifies the stddev's rounding error
    with torch.no_grad():
        fake = out64['pred_seq']
        pre = _relu_inputs({n: t.double() for n, t in p_g.items()}, *args[torch.float64], torch.from_numpy(e_g).double(), *cfg, fake)
        pre32 = _relu_inputs(p_g, *args[torch.float32], torch.from_numpy(e_g), *cfg, fake.float())
    near = {}
    for name, t64, t32 in zip(('encoder fc', 'decoder fc', 'seq_discr fc'), pre, pre32):
        tol = 100 * float((t32.double() - t64).abs().max())
        near[name] = (int((t64.abs() < tol).sum()), '%.1e' % float(t64.abs().min()), '%.1e' % tol)
    sd = out64['stddev'].detach()
    small_sd = sorted(float(v) for v in sd[(sd > 0) & (sd < 1e-3)])
    print('K=%d B=%d: ReLU inputs (count within 100x the fp32 error of 0, min |input|, 100x error): %s; stddev in (0, 1e-3): %s'
          % (k, b, near, ['%.3e' % v for v in small_sd]))
    assert all(v[0] == 0 for v in near.values()), near

    rep, amplified = [], []
    for n in d_names + g_names:
        e_gpu, e_cpu = rel_l2(grads[n], ref64[n].numpy()), rel_l2(cpu32[n].numpy(), ref64[n].numpy())
        rep.append('%s %.2e (CPU fp32 %.2e)' % (n, e_gpu, e_cpu))
        assert e_gpu <= 4 * e_cpu + 2e-6, (n, e_gpu, e_cpu)
        if e_cpu > 5e-5:
            amplified.append(n)
    print('K=%d B=%d gradient rel-L2 vs float64:\n  %s' % (k, b, '\n  '.join(rep)))
    # only the encoder sits upstream of the stddev's KL gradient; where the fp32 ORACLE itself is off float64 by more than a quarter of the
    # 2e-4 bar, that comes from a near-zero stddev above, and the variable is judged by the arbiter alone
    assert all(n.startswith('vae_encoder/') for n in amplified) and (not amplified or small_sd), (amplified, small_sd)

    # ---- against the fp32 oracle, with the toy test's bounds
    for key in ('loss_D', 'loss_G', 'loss_G_recon', 'loss_G_kl', 'loss_G_adv'):
        assert abs(got[key] - want[key]) <= 2e-5 * max(1.0, abs(want[key])), (key, got[key], want[key])
    assert rel_l2(model.last['pred_seq'].cpu().numpy(), want['pred_seq'].numpy()) < 1e-5
    for n, g in list(want['grads_D'].items()) + list(want['grads_G'].items()):
        if float(g.abs().max()) > 1e-7 and n not in amplified:
            assert rel_l2(grads[n], g.numpy()) < 2e-4, n
    for n, p in st.params.items():
        diff = np.abs(exp[n] - p.numpy())
        assert diff.max() <= 2.05e-4 and np.mean(diff > 1e-5) < 0.02, (n, float(diff.max()), float(np.mean(diff > 1e-5)))
