"""CPU: finding, writing and pruning checkpoints (BaseModel.latest_checkpoint / save_checkpoint / prune_checkpoints / resume,
tf_bundle.bundle_complete) on a toy model with a CPU variable store: no device is involved in any of it."""
import os

import numpy as np
import pytest

from kpx_amd import tf_bundle, variables
from kpx_amd.base_model import BaseModel


class Toy(BaseModel):
    name = 'toy'

    def __init__(self, log_dir, width=3):
        super(Toy, self).__init__(is_training=True)
        self.log_dir, self.global_step = str(log_dir), 0
        self.store = variables.VariableStore(device='cpu', seed=1)
        self.device = self.store.device
        with self.store.variable_scope('net'):
            self.store.get_variable('kernel', (3, 3, 2, width), 'kernel')
            self.store.get_variable('bias', (width,), 'zeros')
            self.store.get_variable('moving_mean', (width,), 'moving_zeros')
        self.store.materialise()

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


class Other(Toy):
    name = 'other'


def save(model, step, fmt):
    model.global_step = step + 1
    os.makedirs(os.path.join(model.log_dir, model.name), exist_ok=True)
    return model.save_checkpoint(None, step, fmt=fmt)


def listing(root):
    return sorted(os.path.relpath(os.path.join(d, f), str(root)) for d, _, fs in os.walk(str(root)) for f in fs)


def test_latest_checkpoint_picks_the_newest_complete_one_and_deletes_nothing(tmp_path):
    assert Toy.latest_checkpoint(tmp_path) is None                       # no directory at all
    model = Toy(tmp_path)
    os.makedirs(str(tmp_path / 'toy'))
    assert Toy.latest_checkpoint(tmp_path) is None                       # an empty one
    save(model, 3, 'npz')
    save(model, 5, 'tf')
    save(model, 4, 'npz')
    d = tmp_path / 'toy'
    whole = (d / 'model.ckpt-3.npz').read_bytes()
    (d / 'model.ckpt-9.npz').write_bytes(whole[:len(whole) // 2])        # a truncated archive
    (d / 'model.ckpt-8.npz').write_bytes(b'')                            # an empty one
    np.savez(str(d / 'model.ckpt-10.npz'), weights=np.zeros(3))          # opens as a zip, lists no global_step
    for ext in ('.index', '.data-00000-of-00001'):                       # a bundle whose data file is short
        raw = (d / ('model.ckpt-5' + ext)).read_bytes()
        (d / ('model.ckpt-7' + ext)).write_bytes(raw[:-4] if ext.startswith('.data') else raw)
    (d / 'model.ckpt-11.index').write_bytes(b'not a table')              # an index that does not parse
    (d / 'model.ckpt-12.npz.tmp').write_bytes(whole)                     # a leftover temporary file of a killed write
    (d / 'model.ckpt-13.index.tmp').write_bytes((d / 'model.ckpt-5.index').read_bytes())
    (d / 'notes.txt').write_text('model.ckpt-99.npz')
    (d / 'other.ckpt-20.npz').write_bytes(whole)                         # not this project's file name
    save(Other(tmp_path), 30, 'npz')                                     # a checkpoint of another model name, in its own directory
    before = listing(tmp_path)
    assert Toy.latest_checkpoint(tmp_path) == (str(d / 'model.ckpt-5'), 5)
    assert [(s, os.path.basename(p), c) for s, p, c in Toy.list_checkpoints(tmp_path)] == [
        (3, 'model.ckpt-3.npz', 'npz'), (4, 'model.ckpt-4.npz', 'npz'), (5, 'model.ckpt-5', 'tf')]
    assert Other.latest_checkpoint(tmp_path) == (str(tmp_path / 'other' / 'model.ckpt-30.npz'), 30)
    assert listing(tmp_path) == before
    assert tf_bundle.bundle_complete(str(d / 'model.ckpt-5')) and not tf_bundle.bundle_complete(str(d / 'model.ckpt-7'))
    assert not tf_bundle.bundle_complete(str(d / 'model.ckpt-11')) and not tf_bundle.bundle_complete(str(d / 'model.ckpt-404'))
    os.remove(str(d / 'model.ckpt-5.index'))                             # without its index the bundle is no checkpoint
    assert Toy.latest_checkpoint(tmp_path) == (str(d / 'model.ckpt-4.npz'), 4)


@pytest.mark.parametrize('fmt', ('npz', 'tf'))
def test_an_interrupted_save_leaves_the_previous_newest_and_no_final_name(tmp_path, fmt, monkeypatch):
    model = Toy(tmp_path)
    first = save(model, 1, fmt)
    before = listing(tmp_path)
    state = (tmp_path / 'toy' / 'checkpoint').read_bytes() if fmt == 'tf' else None

    class Killed(Exception):
        pass

    if fmt == 'npz':
        def writer(f, **arrays):
            f.write(b'PK\x03\x04 half an archive')
            raise Killed()
        monkeypatch.setattr(np, 'savez', writer)
    else:
        real = tf_bundle.write_table

        def writer(path, items):
            real(path, items[:2])
            raise Killed()
        monkeypatch.setattr(tf_bundle, 'write_table', writer)
    with pytest.raises(Killed):
        save(model, 2, fmt)
    monkeypatch.undo()
    assert not [f for f in listing(tmp_path) if 'ckpt-2' in f and not f.endswith('.tmp')]          # nothing under a final name
    assert [f for f in listing(tmp_path) if not f.endswith('.tmp')] == before
    assert Toy.latest_checkpoint(tmp_path) == (first, 1)
    if fmt == 'tf':
        assert (tmp_path / 'toy' / 'checkpoint').read_bytes() == state
    fresh = Toy(tmp_path)
    assert fresh.resume(None, first)[0] == 2


@pytest.mark.parametrize('fmt', ('npz', 'tf'))
def test_a_saved_checkpoint_reads_back_bit_for_bit_and_leaves_no_temporary_file(tmp_path, fmt):
    model = Toy(tmp_path)
    path = save(model, 6, fmt)
    got, want = BaseModel.read_checkpoint(path), model.checkpoint_arrays()
    assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in want)
    assert not [f for f in listing(tmp_path) if f.endswith('.tmp')]
    if fmt == 'tf':
        assert (tmp_path / 'toy' / 'checkpoint').read_text() == 'model_checkpoint_path: "model.ckpt-6"\nall_model_checkpoint_paths: "model.ckpt-6"\n'


@pytest.mark.parametrize('fmt', ('npz', 'tf'))
def test_keep_two_over_five_saves_leaves_the_newest_two_with_their_side_files(tmp_path, fmt):
    model = Toy(tmp_path)
    d = tmp_path / 'toy'
    os.makedirs(str(d))
    (d / 'model.ckpt-0.npz').write_bytes(b'truncated')                   # not a checkpoint it can parse: never touched
    (d / 'model.ckpt-77.npz.tmp').write_bytes(b'leftover')
    for step in range(1, 6):
        for rank in (0, 1):
            model.save_rng_state(step, rank)
        model.global_step = step + 1
        model.save_checkpoint(None, step, fmt=fmt, keep=2)
    names = sorted(os.listdir(str(d)))
    kept = ['model.ckpt-%d%s' % (s, e) for s in (4, 5) for e in (('.npz',) if fmt == 'npz' else ('.data-00000-of-00001', '.index'))]
    sides = ['model.ckpt-%d.rng-%d.npz' % (s, r) for s in (4, 5) for r in (0, 1)]
    assert names == sorted(kept + sides + ['model.ckpt-0.npz', 'model.ckpt-77.npz.tmp'] + (['checkpoint'] if fmt == 'tf' else []))
    assert [s for s, _, _ in Toy.list_checkpoints(tmp_path)] == [4, 5]
    if fmt == 'tf':
        assert (d / 'checkpoint').read_text() == ('model_checkpoint_path: "model.ckpt-5"\nall_model_checkpoint_paths: "model.ckpt-4"\n'
                                                  'all_model_checkpoint_paths: "model.ckpt-5"\n')
    with pytest.raises(ValueError):
        model.prune_checkpoints(0)


def test_keep_counts_steps_across_both_containers(tmp_path):
    model = Toy(tmp_path)
    save(model, 1, 'npz'); save(model, 2, 'tf'); save(model, 3, 'npz'); save(model, 4, 'tf')
    removed = model.prune_checkpoints(2)
    assert sorted(os.path.basename(f) for f in removed) == ['model.ckpt-1.npz', 'model.ckpt-2.data-00000-of-00001', 'model.ckpt-2.index']
    assert [s for s, _, _ in Toy.list_checkpoints(tmp_path)] == [3, 4]
    assert (tmp_path / 'toy' / 'checkpoint').read_text() == 'model_checkpoint_path: "model.ckpt-4"\nall_model_checkpoint_paths: "model.ckpt-4"\n'


def test_resume_is_strict_and_names_the_variables(tmp_path):
    model = Toy(tmp_path)
    model.store.assign('net/bias', [1.0, 2.0, 3.0])
    path = save(model, 8, 'npz')
    twin = Toy(tmp_path)
    assert twin.resume(None, path) == (9, 3, 4)                          # global_step, variables (kernel, bias, moving_mean), slots
    assert np.array_equal(twin.store['net/bias'].detach().numpy(), [1.0, 2.0, 3.0])
    wider = Toy(tmp_path, width=4)
    with pytest.raises(Exception) as e:
        wider.resume(None, path)
    assert 'net/kernel: checkpoint (3, 3, 2, 3), model (3, 3, 2, 4)' in str(e.value) and 'net/bias' in str(e.value)
    assert wider.global_step == 0                                        # nothing was restored
    arrays = {k: v for k, v in BaseModel.read_checkpoint(path).items() if k != 'net/bias'}
    np.savez(str(tmp_path / 'toy' / 'model.ckpt-9.npz'), **{k.replace('/', '|'): v for k, v in arrays.items()})
    with pytest.raises(Exception) as e:
        Toy(tmp_path).resume(None, str(tmp_path / 'toy' / 'model.ckpt-9.npz'))
    assert 'net/bias: missing' in str(e.value)
    assert 'net/kernel' in Toy(tmp_path).restore(None, str(tmp_path / 'toy' / 'model.ckpt-9.npz'))     # restore's intersection stays


def test_rng_side_file_round_trip(tmp_path):
    import torch
    model = Toy(tmp_path)
    os.makedirs(str(tmp_path / 'toy'))
    torch.manual_seed(5)
    torch.randn(3)
    path = model.save_rng_state(7, 2)
    assert os.path.basename(path) == 'model.ckpt-7.rng-2.npz'
    want = torch.randn(4)
    torch.manual_seed(99)
    assert model.load_rng_state(7, 2) and torch.equal(torch.randn(4), want)
    assert not model.load_rng_state(7, 3)


def test_scalars_reads_every_event_file_of_a_directory_in_order(tmp_path):
    from kpx_amd import summary
    d = str(tmp_path / 'train')
    for name, steps in (('events.out.tfevents.0000000100.host', (0, 1)), ('events.out.tfevents.0000000200.host', (2, 3))):
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), 'wb') as f:
            for s in steps:
                f.write(summary.frame_record(summary.encode_event(float(s), step=s, values=[summary.scalar_value('lr', 0.5 * s)])))
    assert summary.scalars(d) == {'lr': [(0, 0.0), (1, 0.5), (2, 1.0), (3, 1.5)]}
    assert summary.scalars(summary.event_files(d)[1]) == {'lr': [(2, 1.0), (3, 1.5)]}
