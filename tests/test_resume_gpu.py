"""GPU: train.py --resume.  A run of six steps (A) and a run of three steps continued to six with --resume (B), each from
torch.manual_seed(0) with the synthetic feeds, must write the same model.ckpt-5 bit for bit, name for name: variables, Adam slots, beta
powers and global_step.  For stage 2 that holds only if the device generator's state travelled in the side file of the checkpoint."""
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
MODES = ('detector_translator', 'motion_generator', 'action_classifier')


def _argv(tmp_path, mode, log_dir):
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(log_dir)},
           'training': {'n_steps': 6, 'test_interval': 10 ** 6, 'checkpoint_interval': 1, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': 5, 'n_action': 9, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / ('cfg_%s.yaml' % os.path.basename(str(log_dir)))
    cfg_path.write_text(yaml.safe_dump(cfg))
    return ['--mode', mode, '--config', str(cfg_path), '--synthetic'] + (['--synthetic-vgg'] if mode == 'detector_translator' else [])


def _run(argv, *extra):
    import train
    torch.manual_seed(0)
    train.main(list(argv) + list(extra))


def _last(log_dir, mode, fmt='npz'):
    from kpx_amd.base_model import BaseModel
    return BaseModel.read_checkpoint(os.path.join(str(log_dir), mode, 'model.ckpt-5' + ('.npz' if fmt == 'npz' else '')))


def _assert_same(a, b):
    assert sorted(a) == sorted(b) and 'global_step' in a and int(a['global_step']) == 6
    assert any(k.endswith('/Adam_1') for k in a) and 'beta1_power' in a
    diff = [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
            or not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))]
    assert diff == [], diff


_plain = {}


def plain_run(tmp_path_factory, mode, *extra):
    """Run A, once per (mode, flags) for every case that compares against it."""
    key = (mode,) + extra
    if key not in _plain:
        root = tmp_path_factory.mktemp('plain_%s' % mode)
        _run(_argv(root, mode, root / 'a'), '--steps', '6', *extra)
        _plain[key] = _last(root / 'a', mode)
    return _plain[key]


@pytest.mark.parametrize('mode', MODES)
def test_three_steps_resumed_to_six_equal_six_steps(tmp_path, tmp_path_factory, mode, caplog):
    want = plain_run(tmp_path_factory, mode)
    argv = _argv(tmp_path, mode, tmp_path / 'b')
    _run(argv, '--steps', '3')
    d = tmp_path / 'b' / mode
    assert (d / 'model.ckpt-2.npz').exists() and not (d / 'model.ckpt-3.npz').exists()
    assert (d / 'model.ckpt-2.rng-0.npz').exists() == (mode == 'motion_generator')
    with caplog.at_level('INFO', logger='kpx'):
        _run(argv, '--resume', 'latest', '--steps', '6')
    assert 'global_step 3' in caplog.text and 'model.ckpt-2.npz' in caplog.text and 'Adam slots restored' in caplog.text
    _assert_same(want, _last(tmp_path / 'b', mode))
    assert len([f for f in os.listdir(str(d / 'train')) if f.startswith('events.out.tfevents.')]) >= 1


def test_resume_from_a_bundle(tmp_path, tmp_path_factory):
    mode = 'action_classifier'
    argv = _argv(tmp_path, mode, tmp_path / 'b')
    _run(argv, '--steps', '3', '--ckpt-format', 'tf')
    _run(argv, '--resume', 'latest', '--steps', '6', '--ckpt-format', 'tf')
    assert (tmp_path / 'b' / mode / 'checkpoint').read_text().startswith('model_checkpoint_path: "model.ckpt-5"')
    _assert_same(plain_run(tmp_path_factory, mode), _last(tmp_path / 'b', mode, 'tf'))


def test_resume_from_an_explicit_path_and_without_the_side_file(tmp_path, tmp_path_factory, caplog):
    mode = 'motion_generator'
    argv = _argv(tmp_path, mode, tmp_path / 'b')
    _run(argv, '--steps', '3')
    _run(argv, '--resume', str(tmp_path / 'b' / mode / 'model.ckpt-2.npz'), '--steps', '6')
    want = plain_run(tmp_path_factory, mode)
    _assert_same(want, _last(tmp_path / 'b', mode))
    # the same resume without the generator state: the noise is reseeded (and said so), the run goes on, the result differs
    os.remove(str(tmp_path / 'b' / mode / 'model.ckpt-2.rng-0.npz'))
    with caplog.at_level('WARNING', logger='kpx'):
        _run(argv, '--resume', str(tmp_path / 'b' / mode / 'model.ckpt-2.npz'), '--steps', '6')
    assert 'reseeds its noise' in caplog.text
    got = _last(tmp_path / 'b', mode)
    assert int(got['global_step']) == 6 and any(not np.array_equal(got[k], want[k]) for k in want)


def test_resume_latest_on_an_empty_directory_is_a_plain_run(tmp_path, tmp_path_factory, caplog):
    mode = 'action_classifier'
    with caplog.at_level('INFO', logger='kpx'):
        _run(_argv(tmp_path, mode, tmp_path / 'b'), '--resume', 'latest', '--steps', '6')
    assert 'starting from scratch' in caplog.text
    _assert_same(plain_run(tmp_path_factory, mode), _last(tmp_path / 'b', mode))


def test_resume_under_guard_and_keep(tmp_path, tmp_path_factory):
    mode = 'motion_generator'            # (stage 1 under the guard, both launch forms: tests/test_guard_gpu.py)
    want = plain_run(tmp_path_factory, mode, '--guard')
    _assert_same(want, plain_run(tmp_path_factory, mode))                # a clean guarded run is the plain run
    argv = _argv(tmp_path, mode, tmp_path / 'b')
    _run(argv, '--steps', '3', '--guard', '--keep', '2')
    _run(argv, '--resume', 'latest', '--steps', '6', '--guard', '--keep', '2')
    _assert_same(want, _last(tmp_path / 'b', mode))
    assert sorted(f for f in os.listdir(str(tmp_path / 'b' / mode)) if f.startswith('model.ckpt')) == [
        'model.ckpt-4.npz', 'model.ckpt-4.rng-0.npz', 'model.ckpt-5.npz', 'model.ckpt-5.rng-0.npz']
