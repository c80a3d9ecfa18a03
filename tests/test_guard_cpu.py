"""CPU: the step guard's float64 restatements (tests/guard_ref.py) agree with plain numpy and with loss_optim_ref.adam_step, the planted
inputs are what they claim to be, the new entries refuse bad arguments before any device call, and train.py refuses bad flag values."""
import numpy as np
import pytest

import guard_ref as G
import loss_optim_ref as L


def test_health_of_a_clean_vector_equals_plain_numpy_sums():
    for n in G.SIZES[:-1]:
        g = G.health_clean(n)
        bad, sumsq, maxabs = G.health(g)
        d = g.astype(np.float64)
        assert bad == 0 and maxabs == np.float32(np.max(np.abs(g)))
        assert abs(sumsq - np.sum(d * d)) <= G.sumsq_bound(n, sumsq) and sumsq == pytest.approx(float(np.dot(d, d)), rel=1e-12)
        ref = G.health(g, np.longdouble)[1]
        assert abs(np.longdouble(sumsq) - ref) <= G.sumsq_bound(n, ref)


def test_clean_inputs_span_sixty_decades_and_their_squares_need_fp64():
    g = G.health_clean(4100)
    mag = np.abs(g)
    assert mag.min() <= 1e-29 and mag.max() >= 1e29
    with np.errstate(over='ignore', under='ignore'):
        sq32 = g * g                                            # what a sum of squares kept in fp32 would add
    assert np.isinf(sq32).any() and (sq32 == 0).any()
    assert np.isfinite(G.health(g)[1]) and G.health(g)[1] > 1e58


@pytest.mark.parametrize('n,kind', [c for c in G.HEALTH_CASES if c[0] <= 10 ** 5])      # (the large size adds nothing to a numpy-only check)
def test_planted_values_are_counted_and_left_out(n, kind):
    pos = G.plant_positions(n, kind)
    assert all(0 <= i < n for i in pos) and len(set(pos)) == len(pos)
    clean = G.health_clean(n)
    keep = np.ones(n, bool)
    keep[pos] = False
    for value in G.BAD_VALUES:
        bad, sumsq, maxabs = G.health(G.health_planted(n, kind, value))
        want = G.health(clean[keep]) if keep.any() else (0, 0.0, np.float32(0))
        assert bad == len(pos) and sumsq == want[1] and maxabs == want[2]


def test_slab_boundaries_are_planted_on_both_sides():
    n = G.SIZES[-1]
    pos = G.plant_positions(n, 'slab')
    last = (n - 1) // G.HEALTH_SLAB * G.HEALTH_SLAB
    assert pos == [G.HEALTH_SLAB - 1, G.HEALTH_SLAB, last - 1, last]
    assert G.plant_positions(4100, 'slab') == [] and (4100, 'slab') not in G.HEALTH_CASES


def test_guarded_adam_with_a_clean_health_equals_adam_step_and_a_dirty_one_changes_nothing():
    n = 1003
    p, m, v = L.adam_state(n)
    g = L.adam_grad(n, 1)
    alpha = L.adam_alpha(1)
    c = G.new_counters()
    (p1, m1, v1), c = G.guarded_adam(p, g, m, v, alpha, 0, c, gscale=0.125)
    for got, want in zip((p1, m1, v1), L.adam_step(p, g, m, v, alpha, gscale=0.125)):
        assert np.array_equal(got, want)
    assert c == dict(skipped_total=0, skipped_run=0, updates=1)
    for expect in (dict(skipped_total=1, skipped_run=1, updates=2), dict(skipped_total=2, skipped_run=2, updates=3)):
        (p2, m2, v2), c = G.guarded_adam(p, g, m, v, alpha, 7, c)
        assert np.array_equal(p2, p) and np.array_equal(m2, m) and np.array_equal(v2, v) and c == expect
    _, c = G.guarded_adam(p, g, m, v, alpha, 0, c)
    assert c == dict(skipped_total=2, skipped_run=0, updates=4)


def test_restore_restatement():
    dst, src = np.arange(5, dtype=np.float32), -np.arange(5, dtype=np.float32)
    assert np.array_equal(G.restore(dst, src, 3), src) and np.array_equal(G.restore(dst, src, 0), dst)


def test_guard_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                 # an aligned fake address; nothing is launched
    assert lib.kpx_grad_health_workspace_bytes(1) == 16 and lib.kpx_grad_health_workspace_bytes(G.HEALTH_SLAB + 1) == 32
    assert lib.kpx_grad_health_workspace_bytes(1 << 31) == ((1 << 31) // G.HEALTH_SLAB) * 16
    for args in ((None, 8, a, a), (a, 0, a, a), (a, 8, None, a), (a, 8, a, None), (a + 2, 8, a, a), (a, 8, a + 4, a), (a, 8, a, a + 4)):
        assert lib.kpx_grad_health_f32(*args, None) == -1, args

    def adam(p=a, g=a, m=a, v=a, n=8, alpha=a, health=a):
        return lib.kpx_adam_tf_flat_guarded_f32(p, g, m, v, n, alpha, 0.5, 0.999, 1e-8, 1.0, health, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(alpha=None), dict(health=None), dict(n=0),
               dict(p=a + 4), dict(g=a + 8), dict(m=a + 4), dict(v=a + 12), dict(alpha=a + 2), dict(health=a + 4)):
        assert adam(**kw) == -1, kw
    for args in ((None, a, 8, a), (a, None, 8, a), (a, a, 0, a), (a, a, 8, None), (a + 2, a, 8, a), (a, a + 1, 8, a), (a, a, 8, a + 4)):
        assert lib.kpx_guard_restore_f32(*args, None) == -1, args


def test_guard_ops_refuse_cpu_tensors_wrong_dtypes_and_sizes():
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    f = torch.zeros(8)
    health = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(KpxError):
        ops.grad_health(f, health)
    with pytest.raises(KpxError):
        ops.adam_tf_flat_guarded_(f, f, f, f, torch.zeros(1), 0.5, 0.999, 1e-8, health)
    with pytest.raises(KpxError):
        ops.guard_restore_(f, f, health)


@pytest.mark.parametrize('flags', (['--keep', '0'], ['--guard-max-skips', '0'], ['--resume', 'NOWHERE/model.ckpt-7.npz']))
def test_train_py_refuses_bad_flag_values(tmp_path, flags, capsys):
    import train
    flags = [f.replace('NOWHERE', str(tmp_path)) for f in flags]
    with pytest.raises(SystemExit) as e:
        train.main(['--mode', 'action_classifier', '--config', str(tmp_path / 'absent.yaml'), '--synthetic'] + flags)
    assert e.value.code == 2
    assert flags[0] in capsys.readouterr().err
