"""The restatements and bounds of tests/keypoints_ref.py, checked without a GPU.

Independent derivation: torch float64 autograd of mean -> softmax -> expectation, of x @ w + b followed by the same, and of the maps
agrees with the float64 restatements, gradients and saved-state backward formulas included, to 1e-12 relative plus 1e-15.
Reachability: the sequential-fp32 evaluation of every restatement stays inside every bound at every shape and regime the GPU file uses,
under both fp32 forms of linspace.
Planted slips: each mistake a kernel could make lands outside a bound on at least one listed shape.  (A dropped bias is not among them:
softmax ignores a per-channel constant, so no output of the folded head depends on the bias; that invariance is asserted instead.  A
missing max subtraction is rejected on 'huge' alone: on 'wide' no profile mean of the listed shapes reaches 88.7, where the fp32
exponential overflows, and below that the slip changes no result beyond rounding.)
Refusals: the argument checks of the six entries through the C ABI; every case is rejected by the entry's first statement, before a
stream is looked up or a kernel launched, so no device is needed.
"""
import ctypes

import numpy as np
import pytest
import torch

import keypoints_ref as R

F32, F64 = np.float32, np.float64
T64 = torch.float64
FORMS = ('two', 'fma')


def close(a, b, rel=1e-12, abs_=1e-15):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b) + abs_))


def t_head(x):
    """torch float64: logits [B,H,W,K] -> mu [B,K,2], py, px."""
    h, w = x.shape[1], x.shape[2]
    py = torch.softmax(x.mean(dim=2), dim=1)
    px = torch.softmax(x.mean(dim=1), dim=1)
    mu_y = (py * torch.linspace(-1, 1, h, dtype=T64)[None, :, None]).sum(dim=1)
    mu_x = (px * torch.linspace(-1, 1, w, dtype=T64)[None, :, None]).sum(dim=1)
    return torch.stack([mu_x, mu_y], dim=-1), py, px


def t_gauss(mu, h, w, inv_std):
    # tf.linspace's start + step * i: torch.linspace mirrors its upper half (end - step * j), 1e-16 away, which x - mu amplifies to 1e-8
    # where mu is an fp32 grid value
    ys = (-1.0 + (2.0 / (h - 1)) * torch.arange(h, dtype=T64))[None, :, None, None]
    xs = (-1.0 + (2.0 / (w - 1)) * torch.arange(w, dtype=T64))[None, None, :, None]
    d = (ys - mu[:, None, None, :, 1]) ** 2 + (xs - mu[:, None, None, :, 0]) ** 2
    return torch.exp(-d * float(R.inv2_of(inv_std)))


# ----------------------------------------------------------------------------------------------- independent derivation
@pytest.mark.parametrize('shape', [(2, 13, 21, 5), (1, 8, 12, 129), (1, 2, 2, 1)])
@pytest.mark.parametrize('regime', ['normal', 'wide', 'flat'])
def test_head_and_its_saved_state_backward_are_torch_autograd(shape, regime):
    x = R.head_logits(shape, regime)
    dmu = R.head_dmu(shape)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    mu_t, py_t, px_t = t_head(xt)
    mu_t.backward(torch.from_numpy(dmu).double())
    mu, py, px = R.head(x)
    assert close(mu, mu_t.detach().numpy()) and close(py, py_t.detach().numpy()) and close(px, px_t.detach().numpy())
    assert close(R.head_bwd(dmu, mu, py, px, shape[1], shape[2]), xt.grad.numpy())


@pytest.mark.parametrize('shape,bias', [((2, 13, 21, 8, 5), True), ((9, 8, 12, 8, 17), True), ((2, 24, 40, 8, 5), False)])
def test_folded_head_and_its_backward_are_torch_autograd_of_conv_then_head(shape, bias):
    b, h, w, c, k = shape
    x, wk, bk = R.proj_inputs(shape, bias)
    dmu = R.head_dmu((b, h, w, k))
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt = torch.from_numpy(wk).double().requires_grad_(True)
    bt = torch.from_numpy(bk if bias else np.zeros(k, F32)).double().requires_grad_(True)
    mu_t, py_t, px_t = t_head(xt @ wt + bt)
    mu_t.backward(torch.from_numpy(dmu).double())
    mu, py, px, xs_y, xs_x = R.head_proj(x, wk, bk)
    assert close(mu, mu_t.detach().numpy()) and close(py, py_t.detach().numpy()) and close(px, px_t.detach().numpy())
    assert close(xs_y, x.astype(F64).sum(axis=2)) and close(xs_x, x.astype(F64).sum(axis=1))
    dx, dw, db = R.head_proj_bwd(dmu, mu, py, px, xs_y, xs_x, wk, h, w)
    assert close(dx, xt.grad.numpy()) and close(dw, wt.grad.numpy())
    assert close(db, bt.grad.numpy(), abs_=1e-14) and np.all(np.abs(db) < 1e-14)       # analytically zero


def test_no_output_of_the_folded_head_depends_on_the_bias():
    shape = (2, 13, 21, 8, 5)
    x, wk, bk = R.proj_inputs(shape, True)
    for a, b in zip(R.head_proj(x, wk, bk), R.head_proj(x, wk, None)):
        assert close(a, b, rel=1e-12)


@pytest.mark.parametrize('inv_std', R.INV_STDS)
@pytest.mark.parametrize('regime', R.MU_REGIMES)
def test_gaussian_maps_and_their_gradient_are_torch_autograd(inv_std, regime):
    b, k, h, w = 2, 5, 9, 14
    mu = R.gauss_mu(b, k, h, w, regime)
    dm = R.gauss_dmaps(b, h, w, k)
    mt = torch.from_numpy(mu).double().requires_grad_(True)
    g = t_gauss(mt, h, w, inv_std)
    g.backward(torch.from_numpy(dm).double())
    assert close(R.gauss(mu, h, w, inv_std), g.detach().numpy(), abs_=1e-300)
    assert close(R.gauss_with_bound(mu, h, w, inv_std)[0], g.detach().numpy(), abs_=1e-300)
    assert close(R.gauss_bwd(dm, mu, h, w, inv_std), mt.grad.numpy())
    idx = (np.array([0, 1]), np.array([3, 8]), np.array([13, 0]), np.array([4, 2]))
    assert close(R.gauss_at(mu, h, w, inv_std, *idx)[0], g.detach().numpy()[idx], abs_=1e-300)


def test_fused_linspace_is_the_singly_rounded_value():
    for n in (2, 13, 21, 70, 130, 512):
        exact = np.arange(n) * F64(F32(2) / F32(n - 1)) - 1.0
        fma, two = R.linspace(n, F32, 'fma'), R.linspace(n, F32, 'two')
        assert fma.dtype == F32 and two.dtype == F32
        assert np.all(np.abs(fma.astype(F64) - exact) <= 0.5 * np.spacing(np.abs(fma)).astype(F64) + 1e-300)
        assert np.all(np.abs(two.astype(F64) - R.linspace(n)) <= R.E * (1 + R.linspace(n)) + R.U * np.abs(R.linspace(n)))
    assert R.linspace(13, F32, 'fma')[6] != 0 and R.linspace(13)[6] == 0           # the case the e (1 + lin) term exists for


# ----------------------------------------------------------------------------------------------- reachability
@pytest.mark.parametrize('shape', R.HEAD_SHAPES)
@pytest.mark.parametrize('regime', R.HEAD_REGIMES)
def test_fp32_head_stays_inside_its_bounds(shape, regime):
    x = R.head_logits(shape, regime)
    dmu = R.head_dmu(shape)
    ref, bnd = R.head(x), R.head_bounds(x)
    h, w = shape[1], shape[2]
    for form in FORMS:
        got = R.head(x, F32, form)
        assert all(np.all(np.isfinite(g)) for g in got), 'NaN or infinity in the fp32 head (%s)' % regime
        for name, g, r, b in zip(('mu', 'py', 'px'), got, ref, bnd):
            assert R.worst(g - r, b) <= 1.0, (name, form, R.worst(g - r, b))
        mu, py, px = got
        r = R.worst(R.head_bwd(dmu, mu, py, px, h, w, F32, form) - R.head_bwd(dmu, mu, py, px, h, w), R.head_bwd_bound(dmu, mu, py, px, h, w))
        assert r <= 1.0, ('bwd', form, r)
        if regime in ('spike', 'huge'):
            assert R.head_one_hot_margin(x) > 104 and R.head_one_hot_ok(x, *got)
    if regime == 'spike':                                       # exactly one-hot in float64: mu is a grid value
        assert np.all(np.sort(ref[1], axis=1)[:, -1] == 1.0) and np.all(np.sort(ref[1], axis=1)[:, :-1] == 0.0)
        assert np.all(ref[0][..., 1] == R.linspace(h)[h // 2]) and np.all(ref[0][..., 0] == R.linspace(w)[w // 2])


@pytest.mark.parametrize('shape', R.HEAD_SHAPES[:2])
@pytest.mark.parametrize('regime', R.HEAD_REGIMES[:4])
def test_fp32_head_gradient_stays_inside_forward_plus_backward_bound(shape, regime):
    x = R.head_logits(shape, regime)
    dmu = R.head_dmu(shape)
    h, w = shape[1], shape[2]
    want = R.head_bwd(dmu, *R.head(x), h, w)
    for form in FORMS:
        mu, py, px = R.head(x, F32, form)
        bound = R.head_bwd_bound(dmu, mu, py, px, h, w) + R.head_bwd_forward_part(dmu, x)
        assert R.worst(R.head_bwd(dmu, mu, py, px, h, w, F32, form) - want, bound) <= 1.0


@pytest.mark.parametrize('shape,bias', R.PROJ_SHAPES)
@pytest.mark.parametrize('regime', ['normal', 'wide', 'spike'])
def test_fp32_folded_head_stays_inside_its_bounds(shape, bias, regime):
    b, h, w, c, k = shape
    x, wk, bk = R.proj_inputs(shape, bias, regime)
    dmu = R.head_dmu((b, h, w, k))
    x64 = x.astype(F64)
    ref = R.head(x64 @ wk.astype(F64) + (0.0 if bk is None else bk.astype(F64))) + (x64.sum(axis=2), x64.sum(axis=1))
    bnd = R.head_proj_bounds(x, wk, bk)
    for form in FORMS:
        got = R.head_proj(x, wk, bk, F32, form)
        for name, g, r, bb in zip(('mu', 'py', 'px', 'xs_y', 'xs_x'), got, ref, bnd):
            assert R.worst(g - r, bb) <= 1.0, (name, form, R.worst(g - r, bb))
        want = R.head_proj_bwd(dmu, *got, wk, h, w)
        g32 = R.head_proj_bwd(dmu, *got, wk, h, w, F32, form)
        for name, g, r, bb in zip(('dx', 'dw', 'db'), g32, want, R.head_proj_bwd_bounds(dmu, *got, wk, h, w)):
            assert R.worst(g - r, bb) <= 1.0, (name, form, R.worst(g - r, bb))


def _small_gauss_cases():
    return [(dims, inv) for dims, _, invs, _ in R.GAUSS_CASES if dims[0] < 512 and dims[1] * dims[2] * dims[3] < (1 << 23) for inv in invs]


@pytest.mark.parametrize('dims,inv_std', _small_gauss_cases())
def test_fp32_gaussian_maps_stay_inside_their_bound_under_both_linspace_forms(dims, inv_std):
    b, k, h, w = dims
    for regime in R.MU_REGIMES:
        mu = R.gauss_mu(b, k, h, w, regime)
        g, bound = R.gauss_with_bound(mu, h, w, inv_std)
        for form in FORMS:
            assert R.worst(R.gauss(mu, h, w, inv_std, F32, form) - g, bound) <= 1.0, (regime, form)


@pytest.mark.parametrize('dims', [c[0] for c in R.GAUSS_CASES if c[0][0] == 512 or c[0][1] * c[0][2] * c[0][3] >= (1 << 23)])
def test_fp32_gaussian_maps_of_the_large_cases_on_samples(dims):
    b, k, h, w = dims
    mu = R.gauss_mu(b, k, h, w, 'inside')
    for img in (0, b - 1):
        g, bound = R.gauss_with_bound(mu[img:img + 1, :, :], h, w, 14.3) if h * w * k < (1 << 21) else (None, None)
        if g is None:
            rng = np.random.RandomState(5)
            idx = (np.full(4096, img), rng.randint(0, h, 4096), rng.randint(0, w, 4096), rng.randint(0, k, 4096))
            g, bound = R.gauss_at(mu, h, w, 14.3, *idx)
            got = [R.gauss(mu, h, w, 14.3, F32, f)[idx] for f in FORMS]
        else:
            got = [R.gauss(mu[img:img + 1], h, w, 14.3, F32, f) for f in FORMS]
        for a in got:
            assert R.worst(a - g, bound) <= 1.0


@pytest.mark.parametrize('k,h,w', R.GAUSS_BWD_CASES)
@pytest.mark.parametrize('inv_std', R.GAUSS_BWD_INV_STDS)
def test_fp32_gaussian_gradient_stays_inside_its_bound(k, h, w, inv_std):
    for regime in R.MU_REGIMES:
        mu = R.gauss_mu(2, k, h, w, regime)
        dm = R.gauss_dmaps(2, h, w, k)
        want, bound = R.gauss_bwd(dm, mu, h, w, inv_std), R.gauss_bwd_bound(dm, mu, h, w, inv_std)
        for form in FORMS:
            assert R.worst(R.gauss_bwd(dm, mu, h, w, inv_std, F32, form) - want, bound) <= 1.0, (regime, form)


@pytest.mark.parametrize('case', R.GAUSS_CASES)
def test_gaussian_launch_paths_are_the_ones_the_table_names(case):
    (b, k, h, w), path, _, offset = case
    got = R.gauss_path(b, k, h, w, aligned=not offset)
    assert got[0] == path, got
    assert R.gauss_path(b, k, h, w, ldy=k + 3)[0] == 'strided'
    facts = {((2, 15, 32, 32), 0): (480, 1, 0), ((2, 4, 6, 6), 0): (384, 1, 36), ((1, 512, 2, 2), 0): (512, 1, 0),
             ((512, 15, 34, 32), 0): (480, 9, 240), ((1, 40, 16, 64), 0): (320, 1, 0), ((1, 260, 8, 8), 0): (260, 1, 0)}
    if ((b, k, h, w), offset) in facts:
        assert got[1:] == facts[((b, k, h, w), offset)], got
    if (b, k, h, w) == (1, 16, 8, 33):
        assert got[3] != 0
    if (b, k, h, w) == (512, 40, 12, 63):
        assert got[0] == 'reg' and got[2] > 1 and got[3] != 0, got


# ----------------------------------------------------------------------------------------------- planted slips
def _head_ratio(shape, regime, mutate=None, slip=None, post=None):
    """Worst error/bound of a float64 head with a planted mistake against the true head's bounds."""
    x = R.head_logits(shape, regime)
    ref, bnd = R.head(x), R.head_bounds(x)
    xm = x.astype(F64).copy()
    if mutate:
        mutate(xm)
    with np.errstate(all='ignore'):
        got = R.head(xm, slip=slip)
    if post:
        got = post(got)
    return max(R.worst(g - r, b) for g, r, b in zip(got, ref, bnd))


def _zero_last_row(x):
    x[:, -1] = 0


def _zero_last_col(x):
    x[:, :, -1] = 0


HEAD_SLIPS = {
    'last row of a partial stripe dropped': ((2, 13, 21, 5), 'normal', dict(mutate=_zero_last_row)),
    'last column dropped': ((2, 13, 21, 5), 'normal', dict(mutate=_zero_last_col)),
    'division by the wrong axis length': ((2, 13, 21, 5), 'normal', dict(slip='axis')),
    'linspace step 2/n': ((2, 13, 21, 5), 'normal', dict(slip='step')),
    'x and y swapped': ((2, 13, 21, 5), 'normal', dict(post=lambda o: (o[0][..., ::-1], o[1], o[2]))),
    'no max subtraction (huge)': ((2, 13, 21, 5), 'huge', dict(slip='nomax')),
    'channel k read as k + 1 mod K': ((2, 13, 21, 5), 'normal', dict(post=lambda o: (np.roll(o[0], -1, axis=1), np.roll(o[1], -1, axis=2),
                                                                                      np.roll(o[2], -1, axis=2)))),
}


@pytest.mark.parametrize('name', sorted(HEAD_SLIPS))
def test_head_bounds_reject_the_slip(name):
    shape, regime, kw = HEAD_SLIPS[name]
    assert _head_ratio(shape, regime) == 0.0
    assert _head_ratio(shape, regime, **kw) >= 50, name


def test_folded_head_bounds_reject_a_shifted_channel_and_a_missing_partial_row():
    shape = (9, 8, 12, 8, 17)
    b, h, w, c, k = shape
    x, wk, bk = R.proj_inputs(shape, True)
    dmu = R.head_dmu((b, h, w, k))
    ref = R.head_proj(x, wk, bk)
    bnd = R.head_proj_bounds(x, wk, bk)
    got = R.head_proj(x, np.roll(wk, -1, axis=1), np.roll(bk, -1))
    assert max(R.worst(g - r, bb) for g, r, bb in zip(got[:3], ref[:3], bnd[:3])) >= 50
    state = R.head_proj(x, wk, bk, F32)
    want = R.head_proj_bwd(dmu, *state, wk, h, w)
    bounds = R.head_proj_bwd_bounds(dmu, *state, wk, h, w)
    slipped = R.head_proj_bwd(dmu, *state, wk, h, w, slip='dw_row')
    assert R.worst(slipped[1] - want[1], bounds[1]) >= 50 and R.worst(slipped[0] - want[0], bounds[0]) == 0.0


@pytest.mark.parametrize('inv_std', [14.3, 40.0])
def test_gaussian_bounds_reject_the_slips(inv_std):
    b, k, h, w = 2, 15, 32, 32
    mu = R.gauss_mu(b, k, h, w, 'inside')
    g, bound = R.gauss_with_bound(mu, h, w, inv_std)
    assert R.worst(R.gauss(mu, h, w, inv_std, slip='inv') - g, bound) >= 50                 # inv_std where inv_std**2 belongs
    assert R.worst(R.gauss(np.roll(mu, -1, axis=1), h, w, inv_std) - g, bound) >= 50        # mu of the next channel
    assert R.worst(R.gauss(mu[..., ::-1], h, w, inv_std) - g, bound) >= 50                  # x and y swapped
    kk, hh, ww = 15, 9, 14
    mu = R.gauss_mu(2, kk, hh, ww, 'inside')
    dm = R.gauss_dmaps(2, hh, ww, kk)
    want, bb = R.gauss_bwd(dm, mu, hh, ww, inv_std), R.gauss_bwd_bound(dm, mu, hh, ww, inv_std)
    assert R.worst(0.5 * want - want, bb) >= 50                                             # the gradient without its factor 2
    last = dm.copy()
    last[:, -1] = 0                                                                         # the last row never summed
    assert R.worst(R.gauss_bwd(last, mu, hh, ww, 14.3) - R.gauss_bwd(dm, mu, hh, ww, 14.3), R.gauss_bwd_bound(dm, mu, hh, ww, 14.3)) >= 50


# ----------------------------------------------------------------------------------------------- refusals through the C ABI
EINVAL = -1


@pytest.fixture(scope='module')
def abi():
    from kpx_amd import _lib
    buf = ctypes.create_string_buffer(64)                       # every pointer argument: non-null, never dereferenced by a refused call
    return _lib.lib, ctypes.addressof(buf), buf


@pytest.mark.parametrize('dims', [(1, 513, 8, 4), (1, 8, 513, 4), (1, 8, 8, 257), (1, 1, 8, 4), (1, 8, 1, 4), (0, 8, 8, 4), (1, 8, 8, 0)])
def test_head_forward_refuses(abi, dims):
    lib, p, _ = abi
    assert lib.kpx_keypoint_head_fwd_f32(p, *dims, p, p, p, p, None) == EINVAL
    assert lib.kpx_keypoint_head_fwd_f32(None, 1, 8, 8, 4, p, p, p, p, None) == EINVAL


@pytest.mark.parametrize('dims', [(1, 1, 8, 4), (1, 8, 1, 4), (0, 8, 8, 4), (1, 8, 8, 0)])
def test_head_backward_refuses(abi, dims):
    lib, p, _ = abi
    assert lib.kpx_keypoint_head_bwd_f32(p, p, p, p, *dims, p, None) == EINVAL
    assert lib.kpx_keypoint_head_bwd_f32(p, p, p, p, 1, 8, 8, 4, None, None) == EINVAL


@pytest.mark.parametrize('dims', [(1, 8, 8, 6, 4), (1, 8, 8, 8, 65), (1, 481, 2, 32, 32), (1, 2, 481, 32, 32), (1, 513, 2, 4, 1), (1, 8, 8, 260, 1),
                                  (1, 1, 8, 8, 4), (0, 8, 8, 8, 4)])
def test_folded_head_refuses_in_both_directions(abi, dims):
    lib, p, _ = abi
    assert not R.proj_eligible(*dims) and lib.kpx_keypoint_head_proj_eligible(*dims) == 0
    assert lib.kpx_keypoint_head_proj_fwd_f32(p, p, p, *dims, p, p, p, p, p, p, None) == EINVAL
    assert lib.kpx_keypoint_head_proj_bwd_f32(p, p, p, p, p, p, p, *dims, p, p, p, 0, p, None) == EINVAL


def test_folded_head_eligibility_is_the_restated_rule():
    lib = __import__('kpx_amd._lib', fromlist=['lib']).lib
    assert R.proj_eligible(1, 480, 2, 32, 32) and (480 * 32 + 32 * 32) * 4 == 65536 and not R.proj_eligible(1, 481, 2, 32, 32)
    n = 0
    for b in (0, 1, 3):
        for h in (1, 2, 13, 480, 481, 512, 513):
            for w in (1, 2, 21, 512, 513):
                for c in (0, 4, 6, 8, 32, 128, 256, 260):
                    for k in (0, 1, 5, 32, 64, 65):
                        assert lib.kpx_keypoint_head_proj_eligible(b, h, w, c, k) == int(R.proj_eligible(b, h, w, c, k)), (b, h, w, c, k)
                        n += 1
    assert n > 5000
    # the second LDS limit (n K + C K floats, the backward's) binds where the first does not
    assert not R.proj_eligible(1, 512, 512, 4, 64) and (512 * 4 + 4 * 64) * 4 <= 65536 < (512 * 64 + 4 * 64) * 4
    assert lib.kpx_keypoint_head_proj_eligible(1, 512, 512, 4, 64) == 0


def test_gaussian_entries_refuse(abi):
    lib, p, _ = abi
    assert lib.kpx_gaussian_maps_fwd_f32(p, 1, 5, 8, 8, 14.3, p, 4, None) == EINVAL                 # ldy < K
    for dims in ((0, 5, 8, 8), (1, 0, 8, 8), (1, 5, 1, 8), (1, 5, 8, 1)):
        assert lib.kpx_gaussian_maps_fwd_f32(p, *dims, 14.3, p, 5, None) == EINVAL
    assert lib.kpx_gaussian_maps_fwd_f32(p, 1, 5, 8, 8, 14.3, None, 5, None) == EINVAL
    assert lib.kpx_gaussian_maps_bwd_f32(p, 257, p, 1, 257, 8, 8, 14.3, p, None) == EINVAL          # K = 257
    assert lib.kpx_gaussian_maps_bwd_f32(p, 4, p, 1, 5, 8, 8, 14.3, p, None) == EINVAL              # lddy < K
    assert lib.kpx_gaussian_maps_bwd_f32(p, 5, p, 1, 5, 1, 8, 14.3, p, None) == EINVAL
    assert lib.kpx_gaussian_maps_bwd_f32(p, 5, p, 1, 5, 8, 8, 14.3, None, None) == EINVAL
