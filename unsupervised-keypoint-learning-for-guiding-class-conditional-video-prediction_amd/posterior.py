"""The approximate posterior of the sequence VAE at inference (csrc/posterior.hip, include/kpx.h): FinalModel.encode, evaluate.py --posterior,
animate.py --interpolate / --motion-from.

``networks.vae_encoder`` maps a real motion to logit = [mu | sigma] [B, 2V].  ``latent_stats_add`` accumulates a set of such rows per class
and latent dimension, deterministically (a set fed in pieces leaves the bits of one call); ``latent_sample`` is z = mu + tau sigma eps
(tau = 0: z = mu, the reconstruction); ``latent_path`` walks between two z values on a line or a great circle.  ``summarise_posterior``
turns the accumulated state into the ``posterior`` block of metrics.json on the host (numpy only), ``state_numpy`` restates the kernel's
sums from stored rows, and ``python -m kpx_amd.posterior posterior.npz`` re-summarises the rows a run stored.  Definitions, to the bit, in
include/kpx.h and DESIGN.md section 2.  These are this project's own diagnostics: nothing here is comparable with published figures.
"""
import json
import sys

import numpy as np

# mirrors of include/kpx.h (tests/test_posterior_cpu.py holds them equal to the header)
LATENT_MAX_DIM, LATENT_STATE_FIELDS, LATENT_PATH_MAX_STEPS, LATENT_PATH_MIN_SIN = 1024, 8, 64, 1e-6
LATENT_PATH_MODES = {'lerp': 0, 'slerp': 1}                      # = KPX_LATENT_PATH_*
STATE_FIELDS = ('sum_mu', 'sum_mu2', 'sum_sigma', 'sum_sigma2', 'sum_kl', 'n_mu_zero', 'n_sigma_zero', 'n')
COUNT_FIELDS = ('rows', 'non_finite', 'bad_group')
AU_THRESHOLD = 0.01                                              # Burda et al. 2016: a unit is active when Var_b mu_d exceeds it

DEFINITION = (
    'posterior: the stage-2 encoder q(z | real motion, first pose, class) of this checkpoint, read at inference. logit = [mu | sigma] = '
    'vae_encoder(pseudo labels of the 32 real future frames, pseudo label of the first frame, class), the training graph\'s inputs; the reference passes the head through a ReLU, so '
    'mu >= 0 and sigma >= 0. kl_per_dim[d] = mean over the n samples of 0.5 (mu^2 + sigma^2 - log(1e-8 + sigma^2) - 1), the training '
    'loss\'s term in fp64 (a sigma of exactly 0 costs 0.5 (-log 1e-8 - 1) = 8.71 nats); kl_total = its sum over d. mu_mean, mu_var '
    '(population variance over the samples), sigma_mean per dimension; dead_mu_share / dead_sigma_share = the share of samples whose mu / '
    'sigma is exactly 0. active_units = the number of d with mu_var[d] > au_threshold (0.01, Burda et al. 2016: a definition, not a '
    'measurement). agg_kl_per_dim[d] = KL(N(m, s2) || N(0, 1)) = 0.5 (m^2 + s2 - log s2 - 1) with m = mu_mean[d] and s2 = mu_var[d] + mean '
    'sigma[d]^2, the moment-matched marginal of the aggregate posterior against the prior the rollouts draw z from (null where s2 = 0); '
    'agg_kl_total = its sum over the dimensions where it is defined. per_class: the same figures over the samples of one class. counts: '
    'rows added, rows left out for a non-finite value, rows left out for a class outside [0, n_action). recon: frame (and key-point) '
    'scores of the rollout at z = mu, between --drive labels (the translator given the true key points) and the prior draws of --samples; '
    'z_skill = (model - hold) / (posterior - hold) per score when --drive hold ran: the share of the gain over a frozen pose that the '
    'prior draws keep of what knowing z gives. transfer (--posterior-transfer): sample b\'s image, first pose and class decoded at the mu '
    'of sample (b + 1) mod B, which was encoded with that sample\'s own first pose and class. The real motion is this project\'s own '
    'pseudo labels, the output of its own detector: these figures are not comparable with published figures, and no published figure for '
    'this dataset is quoted.')


def _error(msg):
    from ._lib import KpxError
    return KpxError(msg)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _logit_sizes(what, logit):
    """(B, V) of a logit by its shape alone, before anything looks at a device: the limits are refused on any tensor"""
    import torch
    if not isinstance(logit, torch.Tensor) or logit.dim() != 2 or logit.shape[1] % 2:
        raise _error('%s: logit must be an fp32 tensor [B, 2V] (got %s)'
                     % (what, list(logit.shape) if isinstance(logit, torch.Tensor) else type(logit).__name__))
    b, v = int(logit.shape[0]), int(logit.shape[1]) // 2
    if b < 1 or not 1 <= v <= LATENT_MAX_DIM or b * 2 * v >= 2 ** 31:
        raise _error('%s: logit needs B >= 1, 1 <= V <= %d and B*2V < 2^31 (got B = %d, V = %d)' % (what, LATENT_MAX_DIM, b, v))
    return b, v


def new_state(groups, v, device):
    """(state fp64 [G, V, 8], counts int64 [G, 3]) of an empty set on ``device``"""
    import torch
    return (torch.zeros((groups, v, LATENT_STATE_FIELDS), dtype=torch.float64, device=device),
            torch.zeros((groups, len(COUNT_FIELDS)), dtype=torch.int64, device=device))


def latent_stats_add(logit, state, counts, group=None, kl_rows=None):
    """kpx_latent_stats_add_f64.  logit fp32 [B, 2V] = [mu | sigma]; state fp64 [G, V, 8] and counts int64 [G, 3], both updated in place
    (STATE_FIELDS, COUNT_FIELDS); group int32 [B] or None (then G = 1) -> kl_rows fp64 [B]: sum_v kl of each row, NaN for a row left out
    (a non-finite value: counts[g, 1]; a group outside [0, G): counts[0, 2]).  Each column is summed in ascending b from what ``state``
    held: pieces of any sizes leave the bits of one call.  1 <= V <= 1024, B*2V < 2^31.  One launch on the current stream, capturable."""
    import torch
    from ._args import OPTIONAL, _ptr, _stream, check_out, check_tensors
    from ._lib import lib, check
    b, v = _logit_sizes('latent_stats_add', logit)
    if not isinstance(state, torch.Tensor) or state.dim() != 3 or state.shape[0] < 1:
        raise _error('latent_stats_add: state must be an fp64 tensor [G, V, %d] with G >= 1 (got %s)'
                     % (LATENT_STATE_FIELDS, list(state.shape) if isinstance(state, torch.Tensor) else type(state).__name__))
    g = int(state.shape[0])
    if group is None and g != 1:
        raise _error('latent_stats_add: group is needed for a state of G = %d groups (None stands for G = 1)' % g)
    if g * v * LATENT_STATE_FIELDS >= 2 ** 31:
        raise _error('latent_stats_add: state would hold G*V*8 = %d values, the launch takes fewer than 2^31' % (g * v * LATENT_STATE_FIELDS))
    dev = check_tensors('latent_stats_add', [('logit', logit, torch.float32, (b, 2 * v), 4), ('state', state, torch.float64, (g, v, LATENT_STATE_FIELDS), 8),
                                             ('counts', counts, torch.int64, (g, len(COUNT_FIELDS)), 8), ('group', group, torch.int32, (b,), *OPTIONAL)])
    kl_rows = check_out('latent_stats_add', 'kl_rows', kl_rows, torch.float64, (b,), dev)
    check(lib.kpx_latent_stats_add_f64(logit.data_ptr(), b, v, _ptr(group), g, state.data_ptr(), counts.data_ptr(), kl_rows.data_ptr(), _stream()),
          'kpx_latent_stats_add_f64')
    return kl_rows


def latent_sample(logit, eps=None, tau=1.0, out=None):
    """kpx_latent_sample_f32.  logit fp32 [B, 2V] = [mu | sigma], eps fp32 [B, V] or None -> z fp32 [B, V] = fmaf(fl32(tau sigma), eps, mu).
    eps None or tau == 0: z is mu bit for bit (sigma and eps are not read); tau == 1: the z of ``ops.vae_sample_kl`` bit for bit.  One
    launch on the current stream, capturable; no random numbers are drawn here."""
    import torch
    from ._args import OPTIONAL, _ptr, _stream, check_out, check_tensors
    from ._lib import lib, check
    if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)) or not np.isfinite(tau):
        raise _error('latent_sample: tau must be a finite number (got %r)' % (tau,))
    b, v = _logit_sizes('latent_sample', logit)
    dev = check_tensors('latent_sample', [('logit', logit, torch.float32, (b, 2 * v), 4), ('eps', eps, torch.float32, (b, v), *OPTIONAL)])
    out = check_out('latent_sample', 'out', out, torch.float32, (b, v), dev)
    check(lib.kpx_latent_sample_f32(logit.data_ptr(), _ptr(eps), float(tau), out.data_ptr(), b, v, _stream()), 'kpx_latent_sample_f32')
    return out


def latent_path(za, zb, steps, mode='slerp', out=None):
    """kpx_latent_path_f32.  za, zb fp32 [B, V] -> fp32 [steps, B, V]: step 0 is za and step steps - 1 is zb, bit for bit; step s between
    them stands at t = s / (steps - 1), in fp64 and rounded once.  'lerp': (1 - t) a + t b.  'slerp': per row on the great circle, sin((1 - t)
    w) / sin w and sin(t w) / sin w with w the angle between the rows; a row falls back to 'lerp' when either norm is 0 or sin w < 1e-6:
    a = b, and also a = -b, whose path is then the straight line through 0.  2 <= steps <= 64, 1 <= V <= 1024, steps*B*V < 2^31."""
    import torch
    from ._args import _stream, check_out, check_tensors
    from ._lib import lib, check
    if mode not in LATENT_PATH_MODES:
        raise _error('latent_path: mode must be one of %s (got %r)' % (sorted(LATENT_PATH_MODES), mode))
    if not _is_int(steps) or not 2 <= steps <= LATENT_PATH_MAX_STEPS:
        raise _error('latent_path: steps must be an integer in [2, %d] (got %r)' % (LATENT_PATH_MAX_STEPS, steps))
    if not isinstance(za, torch.Tensor) or za.dim() != 2:
        raise _error('latent_path: za must be an fp32 tensor [B, V] (got %s)' % (list(za.shape) if isinstance(za, torch.Tensor) else type(za).__name__))
    b, v = int(za.shape[0]), int(za.shape[1])
    if b < 1 or not 1 <= v <= LATENT_MAX_DIM or int(steps) * b * v >= 2 ** 31:
        raise _error('latent_path: needs B >= 1, 1 <= V <= %d and steps*B*V < 2^31 (got B = %d, V = %d, steps = %d)' % (LATENT_MAX_DIM, b, v, steps))
    dev = check_tensors('latent_path', [('za', za, torch.float32, (b, v), 4), ('zb', zb, torch.float32, (b, v), 4)])
    out = check_out('latent_path', 'out', out, torch.float32, (int(steps), b, v), dev)
    check(lib.kpx_latent_path_f32(za.data_ptr(), zb.data_ptr(), int(steps), LATENT_PATH_MODES[mode], out.data_ptr(), b, v, _stream()), 'kpx_latent_path_f32')
    return out


# ------------------------------------------------------------------------------------------------ host side: numpy only
def kl_terms(mu, sigma):
    """The kernel's kl per element in float64 from float32 values, operation by operation (include/kpx.h)"""
    m, s = np.asarray(mu, np.float32).astype(np.float64), np.asarray(sigma, np.float32).astype(np.float64)
    s2 = s * s
    with np.errstate(all='ignore'):
        return 0.5 * ((((m * m) + s2) - np.log(np.float64(np.float32(1e-8)) + s2)) - 1.0)


def state_numpy(logit, group=None, groups=1, state=None, counts=None):
    """``latent_stats_add`` on the CPU: a sequential float64 loop over the rows, the kernel's order -> (state [G, V, 8], counts [G, 3],
    kl_rows [B]).  The polynomial sums and the counters have the kernel's bits; the kl fields agree with it to the rounding of ``log``
    (and kl_rows to the order of its sum over v, which is numpy's here)."""
    logit = np.asarray(logit, np.float32)
    b, v = logit.shape[0], logit.shape[1] // 2
    state = np.zeros((groups, v, LATENT_STATE_FIELDS), np.float64) if state is None else state
    counts = np.zeros((groups, len(COUNT_FIELDS)), np.int64) if counts is None else counts
    kl_rows = np.full((b,), np.nan, np.float64)
    for i in range(b):
        g = 0 if group is None else int(group[i])
        if not 0 <= g < groups:
            counts[0, 2] += 1
            continue
        if not np.isfinite(logit[i]).all():
            counts[g, 1] += 1
            continue
        mu, sd = logit[i, :v], logit[i, v:]
        m, s = mu.astype(np.float64), sd.astype(np.float64)
        kl = kl_terms(mu, sd)
        for f, term in enumerate((m, m * m, s, s * s, kl, (mu == 0).astype(np.float64), (sd == 0).astype(np.float64), np.ones(v))):
            state[g, :, f] = state[g, :, f] + term
        counts[g, 0] += 1
        kl_rows[i] = kl.sum()
    return state, counts, kl_rows


def _figures(cols):
    """The figures of one set from its summed columns [V, 8] (n > 0)"""
    n = cols[:, 7]
    with np.errstate(all='ignore'):
        mu_mean, sigma_mean = cols[:, 0] / n, cols[:, 2] / n
        mu_var = np.maximum(cols[:, 1] / n - mu_mean * mu_mean, 0.0)
        mu_var = np.where(n > 1, mu_var, 0.0)                          # one sample has no spread: 0, not the rounding of a difference
        s2 = mu_var + cols[:, 3] / n
        agg = np.where(s2 > 0, 0.5 * (mu_mean * mu_mean + s2 - np.log(np.where(s2 > 0, s2, 1.0)) - 1.0), np.nan)
    return {'kl_per_dim': cols[:, 4] / n, 'mu_mean': mu_mean, 'mu_var': mu_var, 'sigma_mean': sigma_mean,
            'dead_mu_share': cols[:, 5] / n, 'dead_sigma_share': cols[:, 6] / n, 'agg_kl_per_dim': agg}


def _block(cols, au_threshold):
    num = lambda x: None if not np.isfinite(x) else float(x)
    n = int(cols[0, 7]) if cols.shape[0] else 0
    if n < 1:
        return {'n': 0}
    f = _figures(cols)
    out = {'n': n}
    for key, val in f.items():
        out[key] = [num(x) for x in val]
    out['kl_total'] = float(f['kl_per_dim'].sum())
    out['active_units'] = int((f['mu_var'] > au_threshold).sum())
    defined = np.isfinite(f['agg_kl_per_dim'])
    out['agg_kl_total'] = float(f['agg_kl_per_dim'][defined].sum()) if defined.any() else None
    return out


def summarise_posterior(state, counts, au_threshold=AU_THRESHOLD):
    """The ``posterior`` block of metrics.json (DEFINITION) from the accumulated ``state`` [G, V, 8] and ``counts`` [G, 3]: the figures over
    all groups (their columns added in ascending g) and per group; numpy only.  A set without rows gives {'n': 0} and no figures; a figure
    that is not a finite number is null."""
    state, counts = np.asarray(state, np.float64), np.asarray(counts, np.int64)
    if state.ndim != 3 or state.shape[2] != LATENT_STATE_FIELDS or counts.shape != (state.shape[0], len(COUNT_FIELDS)):
        raise ValueError('summarise_posterior: state [G, V, %d] and counts [G, %d] (got %s and %s)'
                         % (LATENT_STATE_FIELDS, len(COUNT_FIELDS), state.shape, counts.shape))
    if not np.isfinite(au_threshold) or au_threshold < 0:
        raise ValueError('summarise_posterior: au_threshold must be a finite number >= 0 (got %r)' % (au_threshold,))
    total = np.zeros(state.shape[1:], np.float64)
    for g in range(state.shape[0]):
        total = total + state[g]
    out = {'definition': DEFINITION, 'vae_dim': int(state.shape[1]), 'au_threshold': float(au_threshold),
           'counts': {name: int(counts[:, i].sum()) for i, name in enumerate(COUNT_FIELDS)}}
    out.update(_block(total, au_threshold))
    out['per_class'] = {str(g): dict(_block(state[g], au_threshold), non_finite=int(counts[g, 1])) for g in range(state.shape[0])}
    return out


def main(argv=None):
    """python -m kpx_amd.posterior posterior.npz [--au T]: the ``posterior`` block of the rows a run of evaluate.py --posterior stored,
    summarised again on the CPU from the stored state (numpy) and printed as JSON.  This project's own quantities: not comparable with
    published figures."""
    argv = sys.argv[1:] if argv is None else list(argv)
    au = None
    if '--au' in argv:
        at = argv.index('--au')
        try:
            au = float(argv[at + 1])
        except (IndexError, ValueError):
            argv = []
        else:
            del argv[at:at + 2]
    if len(argv) != 1 or (au is not None and not (np.isfinite(au) and au >= 0)):
        print('usage: python -m kpx_amd.posterior posterior.npz [--au T >= 0]', file=sys.stderr)
        return 2
    with np.load(argv[0]) as f:
        state, counts = f['state'], f['counts']
        stored = float(f['au_threshold']) if 'au_threshold' in f.files else AU_THRESHOLD
    print(json.dumps(summarise_posterior(state, counts, stored if au is None else au), indent=1, allow_nan=False))
    return 0


if __name__ == '__main__':
    sys.exit(main())
