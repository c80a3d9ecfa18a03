"""CPU: the host half of evaluate.py --prdc -- the constants against the header, the argument errors of the wrapper, of the C entry and of
evaluate.py, the restatement's own tie rules, the numpy scorer and the ``prdc`` block on hand-made arrays against the restatement of
tests/prdc_ref.py, and ``python -m kpx_amd.prdc`` on a small prdc.npz.  None of it needs a GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import prdc_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SHAPES = ((37, 53, 70, 3), (65, 130, 30, 5), (96, 160, 129, 5))


def test_constants_mirror_the_header():
    from kpx_amd import ops, prdc, tool_ops
    src = open(os.path.join(REPO, 'include', 'kpx.h')).read()
    val = lambda name: eval(re.search(r'#define\s+%s\s+(.+)' % name, src).group(1))
    assert prdc.SET_MAX_K == val('KPX_SET_MAX_K') == 8 and prdc.SET_MAX_DIM == val('KPX_SET_MAX_DIM') == 16384
    assert prdc.SET_MAX_QUERIES == val('KPX_SET_MAX_QUERIES') == 4096 and prdc.SET_MAX_REFS == val('KPX_SET_MAX_REFS') == 1 << 20
    assert prdc.SET_BLOCK == val('KPX_SET_BLOCK')
    assert val('KPX_ABI_VERSION') == 25                                 # new entries, no signature changed
    assert ops.set_neighbours is tool_ops.set_neighbours is prdc.set_neighbours and ops.prdc is tool_ops.prdc is prdc.prdc
    assert ops.SET_MAX_K == 8 and ops.SET_MAX_QUERIES == 4096


def test_the_wrapper_and_the_entry_refuse_bad_arguments_without_a_gpu():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib, ops
    from kpx_amd._lib import KpxError, lib
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt)
    launched = _lib.abi_calls[0]
    q, r = z(torch.float64, 3, 4), z(torch.float64, 5, 4)
    for k in (0, 9, True, 2.0):
        with pytest.raises(KpxError, match='set_neighbours: k must be an integer in \\[1, 8\\]'):
            ops.set_neighbours(q, r, k)
    for groups in (dict(q_group=z(torch.int32, 3)), dict(r_group=z(torch.int32, 5))):
        with pytest.raises(KpxError, match='both or neither'):
            ops.set_neighbours(q, r, 2, **groups)
    with pytest.raises(KpxError, match='set_neighbours: .*no CPU fallback'):
        ops.set_neighbours(q, r, 2)
    with pytest.raises(KpxError, match='both or neither'):
        ops.prdc(q, r, 2, real_group=z(torch.int32, 3))
    assert _lib.abi_calls[0] == launched
    a = 1 << 20                                                       # an aligned fake address
    call = lambda q=a, m=3, r=a, n=5, d=4, qg=None, rg=None, skip=None, rad=None, k=2, work=a, nbytes=1 << 20, d2=a, idx=a, inside=None: \
        lib.kpx_set_neighbours_f64(q, m, r, n, d, qg, rg, skip, rad, k, work, nbytes, d2, idx, inside, None)
    need = 1 * 3 * (2 * 12 + 4)                                       # one block of refs x 3 queries x (k (d2, index) + one count)
    for bad in (dict(k=0), dict(k=9), dict(d=0), dict(d=16385), dict(m=0), dict(m=4097), dict(n=0), dict(n=(1 << 20) + 1),
                dict(qg=a), dict(rg=a), dict(inside=a), dict(rad=a), dict(q=None), dict(r=None), dict(work=None), dict(d2=None), dict(idx=None),
                dict(q=a + 4), dict(r=a + 4), dict(work=a + 4), dict(d2=a + 4), dict(rad=a + 4, inside=a), dict(idx=a + 2), dict(rad=a, inside=a + 2),
                dict(qg=a + 2, rg=a), dict(qg=a, rg=a + 1), dict(skip=a + 2), dict(nbytes=need - 1)):
        assert call(**bad) == -1, bad
    assert lib.kpx_set_neighbours_workspace_bytes(3, 5, 2) == need
    assert lib.kpx_set_neighbours_workspace_bytes(4096, 65, 8) == 2 * 4096 * (8 * 12 + 4)
    assert lib.kpx_set_neighbours_workspace_bytes(4096, 1 << 20, 8) == (1 << 14) * 4096 * 100        # beyond 2^32: a size_t
    for m, n, k in ((0, 5, 2), (4097, 5, 2), (3, 0, 2), (3, (1 << 20) + 1, 2), (3, 5, 0), (3, 5, 9)):
        assert lib.kpx_set_neighbours_workspace_bytes(m, n, k) == 0


def test_the_restatement_knows_its_own_tie_rules():
    """prdc_ref.neighbours on hand-made rows: the lowest index of equal distances, the skipped reference, the groups, non-finite rows and
    radii, fewer than k candidates.  The shipped CPU re-scorer, kpx_amd.prdc.neighbours_numpy, is held to the same answers."""
    from kpx_amd import prdc
    r = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [np.nan, 0.0], [3.0, 0.0], [-1.0, 0.0]])     # 0 = 1; 0, 1, 2, 5 at distance 1 of the origin
    q = np.array([[0.0, 0.0], [1.0, 0.0]])
    for search in (lambda *a, **kw: P.neighbours(*a, **kw)[:3], prdc.neighbours_numpy):
        d2, idx, inside = search(q, r, 3, r_radius2=np.array([1.0, 0.5, np.inf, 9.0, np.nan, 1.0]))
        assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and d2.tolist() == [[1.0, 1.0, 1.0], [0.0, 0.0, 2.0]] and idx.dtype == np.int32
        assert inside.tolist() == [2, 2]                              # refs 0 and 5 hold the origin (d2 = radius counts); 0 and 1 hold q[1]
        d2, idx, inside = search(q, r, 8)
        assert idx.tolist() == [[0, 1, 2, 5, 4, -1, -1, -1], [0, 1, 2, 4, 5, -1, -1, -1]] and np.isinf(d2[:, 5:]).all() and 3 not in idx
        assert inside is None
        d2, idx, _ = search(q, r, 2, q_skip=np.array([0, -1]), q_group=np.array([7, 8]), r_group=np.array([7, 7, 8, 8, 8, 7]))
        assert idx.tolist() == [[1, 5], [2, 4]] and d2.tolist() == [[1.0, 1.0], [2.0, 4.0]]
        d2, idx, inside = search(np.array([[np.inf, 0.0]]), r, 1, r_radius2=np.full(6, 1e300))
        assert idx.tolist() == [[-1]] and np.isinf(d2).all() and inside.tolist() == [0]


def test_the_numpy_scorer_equals_the_restatement_on_planted_sets():
    from kpx_amd import prdc
    for n, m, d, k in SHAPES:
        for seed in range(4):
            real, fake, _, _ = P.planted(seed, n, m, d)
            want = P.prdc(real, fake, k)
            assert all(0.1 < want[s] < 0.9 for s in P.SCORES) and want['margin'] >= 1e-9, (n, m, d, k, seed, want['margin'])
            got = prdc.prdc_numpy(real, fake, k)
            for s in P.SCORES:
                assert float(got[s]) == want[s], (s, seed)
            for key in ('real_inside', 'fake_inside', 'real_nn_idx'):
                assert np.array_equal(got[key], want[key]), key
            for key in ('real_radius2', 'fake_radius2', 'real_nn_d2'):
                assert np.all(np.abs(got[key] - want[key]) <= (d + 10) * 2.0 ** -53 * want[key]), key
    real, fake, _, _ = P.planted(5, 40, 60, 33)
    rg, fg = (np.arange(40) % 3).astype(np.int32), (np.arange(60) % 4).astype(np.int32)             # group 3 has no real row
    want, got = P.prdc(real, fake, 2, rg, fg), prdc.prdc_numpy(real, fake, 2, rg, fg)
    assert want['margin'] >= 1e-9 and got['groups'].tolist() == [0, 1, 2, 3] and np.isnan(want['precision'][3])
    assert all(0.0 < v < 1.0 for v in want['recall'][:3])
    for s in P.SCORES:
        assert P.equal_or_nan(got[s], want[s]), s
    assert got['group_n_real'].tolist() == [14, 13, 13, 0] and got['group_n_fake'].tolist() == [15, 15, 15, 15]


def _store(seed=2, s=24, draws=2, d=10, commanded=True):
    rs = np.random.RandomState(seed)
    real, fake, _, _ = P.planted(seed, s, s * draws, d)
    store = {'kp_real': real, 'kp_fake': fake.reshape(draws, s, d), 'own': (np.arange(s) % 2).astype(np.int32),
             'parity': (np.arange(s) % 2).astype(np.int32)}
    store['own'] = rs.randint(0, 2, size=s).astype(np.int32)
    if commanded:
        store['actions'] = np.array([1, 0], np.int32)
        store['kp_commanded'] = np.stack([P.planted(seed + 1 + c, 1, s, d)[1] for c in range(2)])
    return store


def test_the_prdc_block_on_hand_made_arrays():
    from kpx_amd import prdc
    store = _store()
    k = 2
    arrays = prdc.score_store(store, k)
    blk = prdc.summarise(arrays)
    assert blk['definition'] == prdc.DEFINITION and blk['k'] == k and blk['spaces'] == ['kp']
    for text in ('not comparable with published', 'unstable for unequal set sizes', 'own key-point-space and recogniser-space', 'no published figure'):
        assert text in blk['definition'], text
    real, fake, own = store['kp_real'], store['kp_fake'], store['own']
    even, odd = store['parity'] == 0, store['parity'] == 1
    flat = fake.reshape(-1, fake.shape[-1])
    cases = {'draw0': (real, fake[0], None, None), 'all_draws': (real, flat, None, None), 'ceiling': (real[odd], real[even], None, None),
             'draw0_per_class': (real, fake[0], own, own), 'all_draws_per_class': (real, flat, own, np.tile(own, 2)),
             'ceiling_per_class': (real[odd], real[even], own[odd], own[even]),
             'commanded_1': (real[own == 1], store['kp_commanded'][0], None, None), 'commanded_0': (real[own == 0], store['kp_commanded'][1], None, None)}
    assert sorted(blk['kp']) == sorted(cases)
    num = lambda v: None if np.isnan(v) else float(v)
    for name, (x, y, xg, yg) in cases.items():
        want = P.prdc(x, y, k, xg, yg)
        assert want['margin'] >= 1e-9, name
        got = blk['kp'][name]
        assert got['n_real'] == len(x) and got['n_fake'] == len(y)
        for s in P.SCORES:
            if xg is None:
                assert got[s] == num(want[s]), (name, s)
            else:
                assert got[s] == [num(v) for v in want[s]] and got['classes'] == [0, 1], (name, s)
        for key in ('real_inside', 'fake_inside', 'real_nn_idx'):
            assert np.array_equal(arrays['prdc_kp_%s_%s' % (name, key)], want[key])
    assert blk['kp']['all_draws']['n_fake'] == 48 and blk['kp']['ceiling']['n_real'] == 12
    assert json.loads(json.dumps(blk, allow_nan=False)) == blk

    # Y = X: every row lies in its own ball and is its own nearest generated row
    same = prdc.prdc_numpy(real, real, 3)
    assert float(same['precision']) == 1.0 and float(same['recall']) == 1.0 and float(same['coverage']) == 1.0 and float(same['density']) >= 1.0 / 3
    assert same['real_nn_idx'].tolist() == list(range(len(real))) and (same['real_nn_d2'] == 0).all()
    # fewer than k + 1 rows on either side: null, in the dict and in the block
    few = prdc.prdc_numpy(real[:3], fake[0], 3)
    assert all(np.isnan(few[s]) for s in P.SCORES) and np.isinf(few['real_radius2']).all() and (few['fake_inside'] == 0).all()
    assert all(np.isnan(prdc.prdc_numpy(real, fake[0][:3], 3)[s]) for s in P.SCORES)
    assert np.isfinite(prdc.prdc_numpy(real[:4], fake[0][:4], 3)['precision'])
    empty = prdc.prdc_numpy(real[:0], fake[0], 3)
    assert all(np.isnan(empty[s]) for s in P.SCORES) and empty['real_nn_idx'].shape == (0,) and (empty['fake_inside'] == 0).all()
    one = dict(_store(commanded=False), kp_real=real[:1], kp_fake=fake[:, :1], own=own[:1], parity=store['parity'][:1])
    blk = prdc.summarise(prdc.score_store(one, 1))
    assert blk['kp']['draw0']['precision'] is None and blk['kp']['ceiling']['n_real'] == 0 and blk['kp']['ceiling']['n_fake'] == 1
    assert blk['kp']['draw0_per_class']['coverage'] == [None]
    assert json.loads(json.dumps(blk, allow_nan=False)) == blk


def test_a_row_with_a_nan_lies_in_no_ball_and_is_nobodys_neighbour():
    from kpx_amd import prdc
    real, fake, _, _ = P.planted(3, 30, 30, 12)
    real[4, 2], fake[7, 0] = np.nan, np.inf
    want, got = P.prdc(real, fake, 2), prdc.prdc_numpy(real, fake, 2)
    assert np.isinf(got['real_radius2'][4]) and np.isinf(got['fake_radius2'][7]) and got['real_inside'][4] == 0 and got['fake_inside'][7] == 0
    assert got['real_nn_idx'][4] == -1 and 7 not in got['real_nn_idx']
    for s in P.SCORES:
        assert float(got[s]) == want[s]


def test_evaluate_prdc_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval')]
    for extra, text in ((['--prdc'], '--prdc adds to the scores of --metrics and needs it'),
                        (['--prdc', '--samples', '2'], 'needs it'),
                        (['--metrics', '--prdc', '--synthetic', '2'], '--synthetic inputs have neither'),
                        (['--prdc', '--synthetic', '2'], '--synthetic inputs have neither'),
                        (['--metrics', '--prdc-k', '3'], '--prdc-k sets the neighbour count of --prdc and needs it'),
                        (['--metrics', '--prdc', '--prdc-k', '0'], '--prdc-k takes 1..8'),
                        (['--metrics', '--prdc', '--prdc-k', '9'], '--prdc-k takes 1..8'),
                        (['--metrics', '--prdc', '--drive', 'hold', '--drive-only'], "--drive-only skips the model's own rollout, which --prdc is about")):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_the_module_rescores_a_stored_prdc_npz(tmp_path, capsys):
    from kpx_amd import prdc
    store = _store(seed=6, s=20, d=7)
    path = str(tmp_path / 'prdc.npz')
    np.savez(path, k=np.int32(3), **{key: v.astype(np.float32) if v.dtype == np.float64 else v for key, v in store.items()})
    assert prdc.main([path]) == 0
    got = json.loads(capsys.readouterr().out)
    assert got['k'] == 3 and got == json.loads(json.dumps(prdc.summarise(prdc.score_store(store, 3))))
    want = P.prdc(store['kp_real'], store['kp_fake'][0], 3)
    assert want['margin'] >= 1e-9 and all(got['kp']['draw0'][s] == want[s] for s in P.SCORES)
    assert prdc.main([path, '--k', '1']) == 0
    got = json.loads(capsys.readouterr().out)
    want = P.prdc(store['kp_real'], store['kp_fake'][0], 1)
    assert got['k'] == 1 and want['margin'] >= 1e-9 and all(got['kp']['draw0'][s] == want[s] for s in P.SCORES)
    for bad in ([], [path, '--k', '9'], [path, '--k'], [path, path]):
        assert prdc.main(bad) == 2
    assert 'usage: python -m kpx_amd.prdc' in capsys.readouterr().err
