"""tests/batchnorm_ref.py checked on the CPU: every restatement derived a second time with torch float64 autograd, the sequential-fp32
evaluation held to every bound on every case (so every bound is reachable by correct fp32 code), each planted slip rejected by at least
one case, and no case with an element whose ReLU mask fp32 could take either way."""
import numpy as np
import pytest
import torch

import batchnorm_ref as R

F32, F64 = np.float32, np.float64
SMALL = [n for n, s in R.CASES.items() if not s.get('big')]
BIG = [n for n, s in R.CASES.items() if s.get('big')]


def _torch_chain(c, act):
    """Train-mode batch norm per group in torch float64, gradients by autograd of sum(dy * y)."""
    x = torch.tensor(np.asarray(c['x'], F64), requires_grad=True)
    ga = torch.tensor(np.asarray(c['gamma'], F64), requires_grad=True)
    be = torch.tensor(np.asarray(c['beta'], F64), requires_grad=True)
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)             # two-pass: another route to the biased variance
    y = (x - mean) / torch.sqrt(var + float(F32(R.EPS))) * ga + be
    if act:
        y = torch.relu(y)
    (y * torch.tensor(np.asarray(c['dy'], F64))).sum().backward()
    return mean[:, 0].detach().numpy(), var[:, 0].detach().numpy(), y.detach().numpy(), x.grad.numpy(), ga.grad.numpy(), be.grad.numpy()


def _close(a, b, tol=1e-9, floor=0.0):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(np.abs(b), floor) + 1e-300))


@pytest.mark.parametrize('name', ['v_37x32', 'v_19x64_ld96', 's_7x5', 'g5x12', 'g6x6', 'v_1x8'])
@pytest.mark.parametrize('act', [0, 1])
def test_restatements_agree_with_torch_autograd(name, act):
    c = R.case(name)
    n = c['shape'][1]
    m, v, y, dx, dg, db = _torch_chain(c, act)
    fwd, bwd, _ = R.evaluate(c, act, accumulate=0)
    sd = np.sqrt(v + 1e-5)
    # sum x^2 / n - m^2 against the two-pass variance: the one-pass form loses (m/sd)^2 digits, in float64 still 1e-16 (m^2 + v)
    assert _close(fwd['mean'], m, 1e-12, 1e-30)
    _, v1, _ = R.bn_stats(c['x'])
    assert np.all(np.abs(v1 - v) <= 1e-13 * (m * m + v) + 1e-300)
    tame = (np.abs(m) <= 1e2 * sd)[:, None, :] * np.ones_like(y, bool)      # channels where float64's one-pass variance keeps 9 digits
    assert _close(fwd['y'][tame], y[tame], 1e-7, 1e-3)
    scale = np.abs(np.asarray(c['gamma'], F64)) / sd
    assert np.all(np.abs(bwd['dx'] - dx)[tame] <= 1e-7 * (scale[:, None, :] * np.ones_like(y))[tame] * 10)
    tc = tame[:, 0, :].all(0)
    assert _close(bwd['dgamma'][tc], dg[tc], 1e-6, 1.0) and _close(bwd['dbeta'], db, 1e-9, 1.0)
    # moving statistics: torch's closed form moving * decay^g + ... equals the in-order recurrence
    d = float(F32(R.DECAY))
    mm, mv = torch.tensor(np.asarray(c['mm0'], F64)), torch.tensor(np.asarray(c['mv0'], F64))
    for g in range(c['shape'][0]):
        mm = d * mm + (1 - d) * torch.tensor(m[g])
        mv = d * mv + (1 - d) * torch.tensor(v1[g]) * (n / max(n - 1, 1))
    assert _close(fwd['mm'], mm.numpy(), 1e-12, 1e-3) and _close(fwd['mv'], mv.numpy(), 1e-12, 1e-3)
    if n == 1:
        assert np.all(v1 == 0) and np.all(fwd['invstd'] == 1.0 / np.sqrt(F64(F32(R.EPS))))


def test_small_restatements_agree_with_torch():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((70, 12)).astype(F32)
    assert _close(R.chan_sum(x), torch.tensor(x, dtype=torch.float64).sum(0).numpy(), 1e-13, 1e-3)
    var = rng.uniform(0, 2, 12).astype(F32)
    assert _close(R.bn_invstd(var), torch.rsqrt(torch.tensor(var, dtype=torch.float64) + float(F32(R.EPS))).numpy(), 1e-14)
    # the fold: batch norm of (a w + b) with the moving statistics equals a w' + b'
    w, b = rng.standard_normal((9, 12)).astype(F32), rng.standard_normal(12).astype(F32)
    ga, be, mm = (rng.standard_normal(12).astype(F32) for _ in range(3))
    a = torch.tensor(rng.standard_normal((5, 9)))
    for bias in (b, None):
        wf, bf = R.bn_fold(w, bias, ga, be, mm, var)
        z = a @ torch.tensor(w, dtype=torch.float64) + (torch.tensor(bias, dtype=torch.float64) if bias is not None else 0.0)
        want = (z - torch.tensor(mm, dtype=torch.float64)) * torch.rsqrt(torch.tensor(var, dtype=torch.float64) + float(F32(R.EPS))) \
            * torch.tensor(ga, dtype=torch.float64) + torch.tensor(be, dtype=torch.float64)
        assert _close((a @ torch.tensor(wf) + torch.tensor(bf)).numpy(), want.numpy(), 1e-11, 1e-2)


@pytest.mark.parametrize('items', R.TILE_ITEMS)
def test_tile_forms_agree_with_the_direct_forms(items):
    """Unrounded per-item sums give the direct statistics and backward sums back; the rounded slab moves them by u per item at most."""
    c = R.tile_case(items)
    groups, n = c['shape'][0], c['shape'][1]
    assert c['ts_fwd'].shape == (groups * items, 2, 16) and c['cuts'][0] == 0 and c['cuts'][-1] == n and np.all(np.diff(c['cuts']) >= 1)
    m, v, _ = R.bn_stats(c['x'])
    mt, vt, _ = R.bn_stats_tiles(c['ts_fwd'], groups, n)
    xd = np.asarray(c['x'], F64)
    assert np.all(np.abs(mt - m) <= 2 * R.U * np.mean(np.abs(xd), 1)) and np.all(np.abs(vt - v) <= 4 * R.U * (np.mean(xd * xd, 1) + m * m) + items * R.DEN)   # (tiny: the per-item sum x^2 is a denormal float)
    inv = R.bn_stats(c['x'])[2]
    dz, xh = R.bn_dz(c['dy'], c['x'], m, inv, c['gamma'], c['beta'], 1)
    s0, s1 = R.bn_bwd_sums(dz, xh)
    ts = R.tile_stats_bwd(dz, xh * np.asarray(c['gamma'], F64), c['cuts'])
    t0, t1 = R.bn_bwd_sums_tiles(ts, groups, c['gamma'])
    live = np.asarray(c['gamma']) != 0              # at gamma = 0 the slab form has lost xhat: it gives 0 by definition (dx is 0 there anyway)
    assert np.all(np.abs(t0 - s0) <= 2 * R.U * np.abs(dz).sum(1)) and np.all((np.abs(t1 - s1) <= 2 * R.U * np.abs(dz * xh).sum(1))[:, live])
    assert np.all(t1[:, np.asarray(c['gamma']) == 0] == 0) and np.any(np.asarray(c['gamma']) == 0)


def _all_ratios(c, fwd, bwd, act, accumulate, ts_fwd=None, ts_bwd=None, bf16=False):
    r = dict(R.forward_ratios(c, fwd, act, ts=ts_fwd, bf16_y=bf16))
    r.update(R.backward_ratios(c, fwd['mean'], fwd['invstd'], bwd, act, accumulate, ts=ts_bwd, bf16_dx=bf16))
    return r


@pytest.mark.parametrize('name', SMALL)
@pytest.mark.parametrize('act,accumulate', [(1, 0), (0, 1)])
def test_sequential_fp32_meets_every_bound(name, act, accumulate):
    c = R.case(name)
    fwd, bwd, _ = R.evaluate(c, act, accumulate, dtype=F32)
    r = _all_ratios(c, fwd, bwd, act, accumulate)
    print('ratios', name, act, {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    # the float64 reference itself sits far inside (its own statistics are not the saved fp32 ones: only the stages on saved state)
    f64, b64, _ = R.evaluate(c, act, accumulate)
    assert max(R.backward_ratios(c, f64['mean'], f64['invstd'], b64, act, accumulate).values()) <= 1e-3


@pytest.mark.parametrize('name', BIG)
def test_sequential_fp32_meets_every_bound_at_the_capped_sizes(name):
    c = R.case(name)
    fwd, bwd, _ = R.evaluate(c, 1, 0, dtype=F32)
    r = _all_ratios(c, fwd, bwd, 1, 0)
    print('ratios', name, {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize('items', R.TILE_ITEMS)
def test_sequential_fp32_meets_the_tile_bounds(items):
    c = R.tile_case(items)
    fwd, bwd, ts_b = R.evaluate(c, 1, 1, dtype=F32, ts_items=items)
    r = _all_ratios(c, fwd, bwd, 1, 1, ts_fwd=c['ts_fwd'], ts_bwd=ts_b)
    print('ratios tiles', items, {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize('name', list(R.CASES_BF16))
@pytest.mark.parametrize('bf16_dy', [True, False])
def test_sequential_fp32_meets_the_bf16_bounds(name, bf16_dy):
    """The bf16 entries' bounds with outputs rounded to bf16: the fp32 evaluation followed by a bf16 store."""
    c = R.case(name, bf16=True, bf16_dy=bf16_dy)
    assert np.array_equal(R.to_bf16(c['x']), c['x']) and (not bf16_dy or np.array_equal(R.to_bf16(c['dy']), c['dy']))
    for act in (0, 1):
        fwd, bwd, _ = R.evaluate(c, act, 0, dtype=F32)
        fwd['y'], bwd['dx'] = R.to_bf16(fwd['y']), R.to_bf16(bwd['dx'])
        r = _all_ratios(c, fwd, bwd, act, 0, bf16=True)
        assert max(r.values()) <= 1.0, r


def test_small_entries_fp32_meets_bounds():
    c = R.case('v_37x32')
    x = c['x'][0]
    assert R.worst(R.chan_sum(x, F32) - R.chan_sum(x), R.chan_sum_bound(x)) <= 1.0
    rng = np.random.default_rng(11)
    var = np.concatenate((rng.uniform(0, 2, 60), [0.0, 1e-30, 1e30])).astype(F32)
    assert R.worst(R.bn_invstd(var, dtype=F32) - R.bn_invstd(var), R.invstd_bound(var)) <= 1.0
    w, b = rng.standard_normal((37, 63)).astype(F32), rng.standard_normal(63).astype(F32)
    ga, be, mm = (rng.standard_normal(63).astype(F32) for _ in range(3))
    for bias in (b, None):
        got, ref, bnd = R.bn_fold(w, bias, ga, be, mm, var, dtype=F32), R.bn_fold(w, bias, ga, be, mm, var), R.fold_bounds(w, bias, ga, be, mm, var)
        assert R.worst(got[0] - ref[0], bnd[0]) <= 1.0 and R.worst(got[1] - ref[1], bnd[1]) <= 1.0


SLIP_CASES = ['v_37x32', 'g5x12', 's_7x5']


@pytest.mark.parametrize('slip', R.SLIPS)
def test_every_planted_slip_is_rejected(slip):
    """The float64 evaluation with one mistake planted misses a bound on at least one case (and 'sumsq_f32' on the offset channels)."""
    worst_by_case = {}
    for name in SLIP_CASES:
        c = R.case(name)
        fwd, bwd, _ = R.evaluate(c, 1, 1, slip=slip)
        clean = R.evaluate(c, 1, 1)[0]
        if slip in ('dgamma_x', 'drop_xhat_term', 'mean_over_all', 'relu_ge', 'accumulate_ignored'):
            r = R.backward_ratios(c, clean['mean'], clean['invstd'], bwd, 1, 1)
        else:
            r = R.forward_ratios(c, fwd, 1)
        worst_by_case[name] = r
    top = max(max(r.values()) for r in worst_by_case.values())
    assert top > 1.0, (slip, worst_by_case)
    if slip == 'sumsq_f32':
        c = R.case('v_37x32')
        fwd = R.evaluate(c, 1, 1, slip=slip)[0]
        _, _, inv = R.bn_stats(c['x'])
        _, _, dis, _ = R.stats_bounds_x(c['x'])
        off = [i for i, r in enumerate(c['regimes']) if r.startswith('offset')]
        assert all(R.worst((fwd['invstd'] - inv)[:, i], dis[:, i]) > 1.0 for i in off), 'fp32 sum x^2 must fail on the offset channels'


@pytest.mark.parametrize('name', list(R.CASES))
def test_no_relu_mask_is_undecided(name):
    c = R.case(name)
    m, _, inv = R.bn_stats(c['x'])
    assert not R.undecided(c['x'], m, inv, c['gamma'], c['beta']).any()
    # nor on the statistics an fp32 evaluation saves
    m32, _, inv32 = R.bn_stats(c['x'], dtype=F32)
    assert not R.undecided(c['x'], m32, inv32, c['gamma'], c['beta']).any()


@pytest.mark.parametrize('bf16_dy', [True, False])
def test_no_relu_mask_is_undecided_in_the_bf16_and_tile_cases(bf16_dy):
    for c in [R.case(n, bf16=True, bf16_dy=bf16_dy) for n in R.CASES_BF16]:
        m, _, inv = R.bn_stats(c['x'], dtype=F32)
        assert not R.undecided(c['x'], m, inv, c['gamma'], c['beta']).any()
    for c in [R.tile_case(i, bf16=bf16_dy) for i in R.TILE_ITEMS]:          # on the statistics of the slab, which are the ones the entry saves
        m, _, inv = R.bn_stats_tiles(c['ts_fwd'], c['shape'][0], c['shape'][1], dtype=F32)
        assert not R.undecided(c['x'], m, inv, c['gamma'], c['beta']).any()


def test_exact_edges():
    """Constant channel: y == beta, invstd == 1/sqrtf(eps), in fp32 as in float64.  gamma = beta = 0 under ReLU: dx, dgamma, dbeta exactly 0;
    gamma = 0, beta > 0: dx exactly 0."""
    c = R.case('g5x12')
    ga, be = np.asarray(c['gamma']), np.asarray(c['beta'])
    assert ga[8] == 0 and be[8] == 0 and ga[9] == 0 and be[9] > 0
    const = [i for i, r in enumerate(c['regimes']) if r == 'constant']
    for dtype in (F64, F32):
        fwd, bwd, _ = R.evaluate(c, 1, 0, dtype=dtype)
        assert np.all(fwd['y'][:, :, const] == np.maximum(be[const], 0).astype(dtype))
        assert np.all(fwd['invstd'][:, const] == (dtype(1) / np.sqrt(dtype(F32(R.EPS)))))
        assert np.all(bwd['dx'][:, :, 8] == 0) and bwd['dgamma'][8] == 0 and bwd['dbeta'][8] == 0
        assert np.all(bwd['dx'][:, :, 9] == 0)
