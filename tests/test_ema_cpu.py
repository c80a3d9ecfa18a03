"""CPU: the averaged generator's host side (kpx_amd/ema.py, the shadow entries of checkpoints, train.py's flags) and the restatements of
tests/ema_ref.py; the two new entries refuse bad arguments before any device call.  No device is involved in any of it."""
import os

import numpy as np
import pytest

import ema_ref as E


def f32_bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


# ----------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize('warmup', (True, False))
@pytest.mark.parametrize('decay', E.DECAYS)
def test_rate_equals_the_restatement_bit_for_bit(decay, warmup):
    from kpx_amd import ema
    for t in E.STEPS:
        got, want = ema.rate(decay, t, warmup), E.rate(decay, t, warmup)
        assert isinstance(got, np.float32) and f32_bits(got)[0] == f32_bits(want)[0], (decay, t, warmup, got, want)
        assert 0.0 < got < 1.0
    assert ema.rate(0.999, 0) == np.float32(1) - np.float32(0.1) and ema.rate(0.9, 10 ** 7) == np.float32(1) - np.float32(0.9)
    assert ema.rate(0.999, 0, warmup=False) == np.float32(1) - np.float32(0.999)
    assert ema.SUFFIX == E.SUFFIX == '/ExponentialMovingAverage'


# ----------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize('n', E.SIZES[:3])
def test_both_float32_forms_stay_inside_the_bound_on_the_chosen_operands(n):
    for r in E.RATES:
        e, p = E.operands(n, r)
        ref, bound = E.update(e, p, r), E.bound(e, p)
        assert np.isfinite(ref).all()
        with np.errstate(under='ignore'):
            for form in (E.update_f32_plain, E.update_f32_fma):
                got = form(e, p, r)
                assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - ref) <= bound).all(), (n, r, form.__name__)
        if n >= 1003:
            i = np.arange(n)
            assert np.array_equal(e[i % 4 == 1], p[i % 4 == 1]) and not np.signbit(e[i % 4 == 1][e[i % 4 == 1] == 0]).any()
            assert np.array_equal(f32_bits(E.update_f32_fma(e, p, r))[i % 4 == 1], f32_bits(e)[i % 4 == 1])       # e == p leaves e's bits
            mags = np.abs(e[i % 4 == 0])
            assert mags.min() < 1e-38 and mags.max() > 1e36                                   # subnormal to 1e38
            if 0 < r < 1:                                                                      # the cancelling quarter ends near zero
                c = i % 4 == 2
                assert (np.abs(ref[c]) <= 1e-6 * (np.abs(e[c]) + np.abs(p[c])) + 1e-30).all()


def test_swap_operands_hold_nan_payloads_infinities_and_negative_zero():
    for n in E.SIZES[:3]:
        a, b = E.swap_operands(n)
        both = np.concatenate([a, b])
        f = both.view(np.float32)
        assert a.dtype == b.dtype == np.uint32 and a.size == b.size == n
        if n >= 5:
            assert np.isnan(f).any() and np.isinf(f).any() and (both == 0x80000000).any()
            assert len({int(w) & 0x3fffff for w in both[np.isnan(f)]}) > 1                    # more than one payload


# ----------------------------------------------------------------------------------------------- select and the module CLI
def test_select_moves_shadows_onto_their_variables_and_drops_slots():
    from kpx_amd import ema
    arrays, want = E.shadow_fixture()
    got = ema.select(arrays)
    assert sorted(got) == sorted(want)
    assert all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)
    assert not [k for k in got if k.endswith(('/Adam', '/Adam_1', ema.SUFFIX))]
    assert np.array_equal(got['translator/conv_8_0/conv2d/kernel'], arrays['translator/conv_8_0/conv2d/kernel' + ema.SUFFIX])
    assert not np.array_equal(got['translator/conv_8_0/conv2d/kernel'], arrays['translator/conv_8_0/conv2d/kernel'])
    assert got['global_step'] == 41 and np.array_equal(got['img_discr/conv_1/conv2d/kernel'], arrays['img_discr/conv_1/conv2d/kernel'])
    plain = {k: v for k, v in arrays.items() if not k.endswith(ema.SUFFIX)}
    with pytest.raises(KeyError) as e:
        ema.select(plain)
    assert 'no averaged weights' in str(e.value) and ema.SUFFIX in str(e.value)
    assert sorted(ema.select(plain, strict=False)) == sorted(k for k in plain if not k.endswith(('/Adam', '/Adam_1')))


@pytest.mark.parametrize('fmt_in', ('npz', 'tf'))
@pytest.mark.parametrize('fmt_out', ('npz', 'tf'))
def test_module_cli_round_trips_through_both_containers(tmp_path, fmt_in, fmt_out, capsys):
    from kpx_amd import ema, tf_bundle
    from kpx_amd.base_model import BaseModel
    arrays, want = E.shadow_fixture()
    src = str(tmp_path / 'in' / 'model.ckpt-40')
    os.makedirs(os.path.dirname(src))
    if fmt_in == 'tf':
        tf_bundle.write_bundle(src, arrays)
    else:
        src += '.npz'
        np.savez(src, **{k.replace('/', '|'): v for k, v in arrays.items()})
    dst = str(tmp_path / 'out' / ('averaged.npz' if fmt_out == 'npz' else 'averaged'))
    os.makedirs(os.path.dirname(dst))
    assert ema.main([src, dst, '--ckpt-format', fmt_out]) == 0
    got = BaseModel.read_checkpoint(dst)
    sel = ema.select(BaseModel.read_checkpoint(src))
    assert sorted(got) == sorted(sel) == sorted(want)
    assert all(np.array_equal(got[k], sel[k]) and got[k].dtype == sel[k].dtype and np.array_equal(got[k], want[k]) for k in want)
    assert not [f for _, _, fs in os.walk(str(tmp_path)) for f in fs if f.endswith('.tmp')]
    # its output holds no averages: a second pass refuses it, and names it
    with pytest.raises(SystemExit) as e:
        ema.main([dst, str(tmp_path / 'out' / 'again.npz')])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert dst in err and 'no averaged weights' in err


# ----------------------------------------------------------------------------------------------- checkpoints of a model with averages
def _toy_classes():
    from kpx_amd import variables
    from kpx_amd.base_model import BaseModel

    class Toy(BaseModel):
        """The CPU toy of tests/test_resume_cpu.py with a fused head, a discriminator variable and, on request, averages."""
        name = 'toy'

        def __init__(self, log_dir, ema=None, seed=1):
            super(Toy, self).__init__(is_training=True)
            self._ema_config(ema)
            self.log_dir, self.global_step = str(log_dir), 0
            self.store = variables.VariableStore(device='cpu', seed=seed)
            self.device = self.store.device
            with self.store.variable_scope('net'):
                self.store.get_variable('kernel', (3, 3, 2, 3), 'kernel')
                self.store.get_variable('bias', (3,), 'zeros')
                self.store.get_variable('moving_mean', (3,), 'moving_zeros')
            with self.store.variable_scope('translator/conv_8_0+1/conv2d'):
                self.store.get_variable('kernel', (3, 3, 2, 4), 'kernel_head31')
            with self.store.variable_scope('img_discr'):
                self.store.get_variable('kernel', (3, 3, 2, 2), 'kernel')
            self.store.materialise(**({'ema': True} if self.ema is not None else {}))

        def build(self, inputs=None):
            pass

        def train_step(self, *a, **k):
            pass

        def test_step(self, *a, **k):
            pass

        def collect_test_results(self, *a, **k):
            pass

        def checkpoint_arrays(self):
            arrays = self.store.export_numpy(include_slots=True)
            arrays['global_step'] = np.int32(self.global_step)
            return arrays

        def _restore_extra(self, arrays):
            self.global_step = int(arrays['global_step'])

    return Toy


G_NAMES = ('net/kernel', 'net/bias', 'translator/conv_8_0/conv2d/kernel', 'translator/conv_8_1/conv2d/kernel')


def _save(model, step, fmt):
    model.global_step = step + 1
    os.makedirs(os.path.join(model.log_dir, model.name), exist_ok=True)
    return model.save_checkpoint(None, step, fmt=fmt)


def _shadow_bits(model):
    from kpx_amd import ema
    return {k: f32_bits(v).copy() for k, v in model.checkpoint_arrays().items() if k.endswith(ema.SUFFIX)}


@pytest.mark.parametrize('fmt', ('npz', 'tf'))
def test_a_save_with_ema_carries_the_shadow_names_and_resume_restores_them(tmp_path, fmt, caplog):
    import logging
    import torch
    from kpx_amd import ema
    from kpx_amd.base_model import BaseModel
    Toy = _toy_classes()
    with pytest.raises(ValueError):
        Toy(tmp_path, ema=1.0)
    with pytest.raises(ValueError):
        Toy(tmp_path, ema=0.0)
    model = Toy(tmp_path, ema=0.9)
    g, d = model.store.buckets['G'], model.store.buckets['D']
    assert d.ema is None and g.ema is not None and g.ema.numel() == g.params.numel() and g.ema.data_ptr() != g.params.data_ptr()
    assert torch.equal(g.ema, g.params.detach())                         # initialised as a copy of the parameters
    with torch.no_grad():
        g.ema.mul_(0.5).add_(0.125)                                      # averages that differ from the parameters
    path = _save(model, 3, fmt)
    arrays = BaseModel.read_checkpoint(path)
    assert sorted(k for k in arrays if k.endswith(ema.SUFFIX)) == sorted(n + ema.SUFFIX for n in G_NAMES)       # fused head split, no 'D' key
    assert arrays['translator/conv_8_0/conv2d/kernel' + ema.SUFFIX].shape == (3, 3, 2, 3)
    assert arrays['translator/conv_8_1/conv2d/kernel' + ema.SUFFIX].shape == (3, 3, 2, 1)
    assert np.array_equal(arrays['net/kernel' + ema.SUFFIX], arrays['net/kernel'] * np.float32(0.5) + np.float32(0.125))
    plain_names = sorted(Toy(tmp_path).checkpoint_arrays())
    assert sorted(k for k in arrays if not k.endswith(ema.SUFFIX)) == plain_names              # every other name is what it is without ema
    # resume with ema: the averages come back bit for bit; the figures count no shadow
    twin = Toy(tmp_path, ema=0.9, seed=2)
    assert twin.resume(None, path) == (4, 6, 10)         # global_step; six variable names (the head counts twice); two slots of five; no shadow
    assert _shadow_bits(twin).keys() == _shadow_bits(model).keys()
    assert all(np.array_equal(_shadow_bits(twin)[k], v) for k, v in _shadow_bits(model).items())
    # resume without ema: ignored, one log line, and the next checkpoint does not carry them
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='kpx'):
        off = Toy(tmp_path, seed=3)
        assert off.resume(None, path) == (4, 6, 10)
    said = [r.getMessage() for r in caplog.records if 'averaged weights' in r.getMessage()]
    assert len(said) == 1 and 'will not carry' in said[0] and path in said[0]
    assert sorted(off.checkpoint_arrays()) == plain_names
    assert all(np.array_equal(off.checkpoint_arrays()[k], arrays[k]) for k in plain_names)


def test_a_resume_from_a_checkpoint_without_shadows_starts_them_at_the_parameters(tmp_path, caplog):
    import logging
    from kpx_amd import ema
    Toy = _toy_classes()
    path = _save(Toy(tmp_path, seed=4), 5, 'npz')                        # written without ema
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='kpx'):
        model = Toy(tmp_path, ema=0.999, seed=5)
        model.resume(None, path)
    said = [r.getMessage() for r in caplog.records if 'averaged weights' in r.getMessage()]
    assert len(said) == 1 and 'start as the restored parameters' in said[0] and path in said[0]
    arrays = model.checkpoint_arrays()
    for n in G_NAMES:
        assert np.array_equal(f32_bits(arrays[n + ema.SUFFIX]), f32_bits(arrays[n])), n
    # and the inference restore refuses such a checkpoint by name under ema=True
    with pytest.raises(Exception) as e:
        Toy(tmp_path).restore(None, path, ema=True)
    assert path in str(e.value) and 'no averaged weights' in str(e.value)


def test_restore_under_ema_reads_the_averages_as_the_variables(tmp_path):
    import torch
    Toy = _toy_classes()
    model = Toy(tmp_path, ema=0.9)
    with torch.no_grad():
        model.store.buckets['G'].ema.add_(1.0)
    path = _save(model, 1, 'tf')
    reader, plain = Toy(tmp_path, seed=7), Toy(tmp_path, seed=7)
    reader.restore(None, path, ema=True)
    plain.restore(None, path)
    for n in ('net/kernel', 'net/bias', 'translator/conv_8_0+1/conv2d/kernel'):
        assert torch.equal(reader.store[n].detach(), plain.store[n].detach() + 1.0), n
    for n in ('net/moving_mean', 'img_discr/kernel'):
        assert torch.equal(reader.store[n].detach(), plain.store[n].detach()), n


# ----------------------------------------------------------------------------------------------- flags and entries
@pytest.mark.parametrize('flags,word', ((['--ema', '1'], 'strictly between 0 and 1'), (['--ema', '0'], 'strictly between 0 and 1'),
                                        (['--ema-test'], 'need --ema DECAY'), (['--ema', '-0.5'], 'strictly between 0 and 1'),
                                        (['--ema-no-warmup'], 'need --ema DECAY')))
def test_train_py_refuses_bad_ema_flags(tmp_path, flags, word, capsys):
    import train
    with pytest.raises(SystemExit) as e:
        train.main(['--mode', 'action_classifier', '--config', str(tmp_path / 'absent.yaml'), '--synthetic'] + flags)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_ema_kw_passes_the_keywords_only_under_the_flags():
    import train
    from argparse import Namespace
    assert train._ema_kw(Namespace(ema=None, ema_no_warmup=False)) == {}
    assert train._ema_kw(Namespace(ema=0.99, ema_no_warmup=False)) == {'ema': 0.99}
    assert train._ema_kw(Namespace(ema=0.99, ema_no_warmup=True)) == {'ema': 0.99, 'ema_warmup': False}


def test_ema_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a, b = 1 << 20, 1 << 21                                     # aligned fake addresses; nothing is launched

    def ema(e=a, p=b, n=8, rate=a, health=None):
        return lib.kpx_ema_flat_f32(e, p, n, rate, health, None)
    for kw in (dict(e=None), dict(p=None), dict(rate=None), dict(n=0), dict(e=a + 4), dict(e=a + 8), dict(p=b + 4), dict(p=b + 12),
               dict(rate=a + 2), dict(rate=a + 1), dict(health=a + 4), dict(health=a + 2)):
        assert ema(**kw) == -1, kw
    for args in ((None, b, 8), (a, None, 8), (a, a, 8), (a, b, 0), (a + 4, b, 8), (a, b + 8, 8), (a + 2, b + 2, 8)):
        assert lib.kpx_swap_flat_f32(*args, None) == -1, args


def test_ema_ops_refuse_cpu_tensors():
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    f, g = torch.zeros(8), torch.zeros(8)
    with pytest.raises(KpxError):
        ops.ema_flat_(f, g, torch.zeros(1))
    with pytest.raises(KpxError):
        ops.swap_flat_(f, g)
