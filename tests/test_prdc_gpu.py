"""GPU: the k-nearest-row search of csrc/prdc.hip (kpx_amd.ops.set_neighbours) against the longdouble restatement of tests/prdc_ref.py -- the
indices and the inside counts bit for bit, the distances within the bound of the kernel's summation order, exact ties, position independence,
the skipped reference, the groups, non-finite values, the query chunks -- then ops.prdc against the restated scores and evaluate.py --prdc
end to end on the fixture videos."""
import json
import os

import numpy as np
import pytest
import torch

import prdc_ref as P
import resident_seq_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
SIZES = ((1, 1), (2, 9), (7, 33), (9, 65), (33, 31), (65, 130))
KS = (1, 3, 8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return None if t is None else t.cpu().numpy()


def _search(q, r, k, q_group=None, r_group=None, q_skip=None, r_radius2=None):
    from kpx_amd import ops
    opt = lambda a, dt: None if a is None else _dev(np.asarray(a, dt))
    out = ops.set_neighbours(_dev(q), _dev(r), k, opt(q_group, np.int32), opt(r_group, np.int32), opt(q_skip, np.int32), opt(r_radius2, np.float64))
    assert out[0].dtype == torch.float64 and out[1].dtype == torch.int32 and out[0].shape == out[1].shape == (len(q), k)
    return tuple(_host(t) for t in out)


def _clear(d2, ok, k):
    """the precondition of a bit-equal index: among each query's eligible distances the k + 1 lowest are 1e-9 relative apart"""
    for j in range(d2.shape[0]):
        low = np.sort(d2[j][ok[j]])[:k + 1]
        if len(low) > 1 and not np.all(np.diff(low) >= 1e-9 * low[1:]):
            return False
    return True


def _assert_matches(got, want, d, exact=False):
    (g_d2, g_idx, g_in), (w_d2, w_idx, w_in) = got, want[:3]
    assert np.array_equal(g_idx, w_idx)
    empty = w_idx < 0
    assert np.isinf(g_d2[empty]).all() and (g_d2[empty] > 0).all()
    if exact:
        assert np.array_equal(g_d2[~empty], w_d2[~empty].astype(np.float64))
    else:
        err = np.abs(g_d2[~empty].astype(P.LD) - w_d2[~empty])
        assert np.all(err <= P.d2_bound(d) * w_d2[~empty]), float((err / np.maximum(w_d2[~empty], 1e-300)).max())
    if w_in is None:
        assert g_in is None
    else:
        assert g_in.dtype == np.int32 and np.array_equal(g_in, w_in)


# ------------------------------------------------------------------------------------------------ 1. planted sets against the restatement
@pytest.mark.parametrize('d', [1, 63, 64, 65, 129, 960])
def test_neighbours_and_counts_on_planted_sets(d):
    for m, n in SIZES:
        refs, queries, _, _ = P.planted(1000 * d + n, n, m, d)
        d2 = P.d2_matrix(queries, refs)
        radius2 = (d2.mean(axis=0) * P.LD(0.37)).astype(np.float64)          # a generic value per reference: no distance equals it
        with np.errstate(invalid='ignore'):
            assert np.all(np.abs(d2 - radius2[None, :]) >= 1e-9 * radius2[None, :])
        assert _clear(d2, np.isfinite(d2), max(KS))
        for k in KS:                                                           # N < k included: (1,1), (2,9) ... leave places empty
            want = P.neighbours(queries, refs, k, r_radius2=radius2, d2=d2)
            _assert_matches(_search(queries, refs, k, r_radius2=radius2), want, d)
            assert (want[1][:, min(n, k):] == -1).all() and (want[1][:, :min(n, k)] >= 0).all()
        if n > 1:
            assert 0 < want[2].sum() < m * n                                   # the counts test something: some balls hold a query, some do not
    got = _search(queries, refs, 3)
    assert got[2] is None                                                      # no radii, no counts


# ------------------------------------------------------------------------------------------------ 2. exact ties
def test_planted_exact_ties_go_to_the_lowest_index():
    rs = np.random.RandomState(5)
    d, m = 70, 9
    refs = rs.randint(-8, 9, size=(100, d)).astype(np.float64)
    refs[50:] = refs[:50]                                                     # every reference twice, 50 apart: two blocks of the kernel
    refs[20], refs[21], refs[85] = refs[3], refs[3], refs[3]                  # and one five times: 3, 20, 21, 53, 85
    queries = rs.randint(-8, 9, size=(m, d)).astype(np.float64)
    queries[0] = refs[3]                                                      # distance 0 to five references
    e = np.zeros(d)
    e[7] = 2.0
    refs[10], refs[35], refs[60] = queries[1] + e, queries[1] - e, queries[1] + np.roll(e, 3)      # a query equidistant from three others
    d2 = P.d2_matrix(queries, refs)
    radius2 = d2[rs.randint(0, m, size=100), np.arange(100)].astype(np.float64)                    # every radius equals one query's distance: <= counts it
    for k in KS:
        want = P.neighbours(queries, refs, k, r_radius2=radius2, d2=d2)
        got = _search(queries, refs, k, r_radius2=radius2)
        _assert_matches(got, want, d, exact=True)                             # integers: every sum is exact, nn_d2 included
        assert got[1][0, 0] == 3 and got[0][0, 0] == 0.0 and got[1][1, 0] == 10 and got[0][1, 0] == 4.0
    assert got[1][0, :5].tolist() == [3, 20, 21, 53, 85] and got[1][1, :3].tolist() == [10, 35, 60]
    pairs = got[1][2:7]                                                       # queries 2..6 meet untouched references only:
    assert (pairs[:, 0::2] < 50).all() and np.array_equal(pairs[:, 1::2], pairs[:, 0::2] + 50)     # a duplicate follows its original
    assert np.array_equal(got[0][2:7, 0::2], got[0][2:7, 1::2]) and (got[2] >= 1).all()


# ------------------------------------------------------------------------------------------------ 3. position independence
def test_a_distance_depends_on_neither_rows_position_nor_the_problems_size():
    d = 129
    refs, queries, _, _ = P.planted(9, 150, 70, d)
    pair_q = queries[0].copy()
    pair_r = (pair_q + 1e-3 * np.random.RandomState(1).randn(d)).astype(np.float32).astype(np.float64)     # the nearest reference wherever it stands
    bits = []
    for m, n, at_q, at_r in ((1, 1, 0, 0), (13, 150, 11, 133), (70, 67, 64, 66), (8, 64, 7, 0), (9, 65, 8, 64)):
        q, r = queries[:m].copy(), refs[:n].copy()
        q[at_q], r[at_r] = pair_q, pair_r
        d2, idx, _ = _search(q, r, 1)
        assert idx[at_q, 0] == at_r
        bits.append(d2[at_q, 0].view(np.int64))
    assert len(set(int(b) for b in bits)) == 1
    want = P.d2_matrix(pair_q[None], pair_r[None])[0, 0]
    assert abs(P.LD(bits[0].view(np.float64)) - want) <= P.d2_bound(d) * want


# ------------------------------------------------------------------------------------------------ 4. the skipped reference and the groups
def test_self_exclusion_and_groups_equal_the_restatement_on_the_reduced_sets():
    d, n, k = 65, 40, 3
    rows, other, _, _ = P.planted(12, n, 33, d)
    d2_all = P.d2_matrix(rows, rows)
    assert _clear(d2_all, ~np.eye(n, dtype=bool), k)
    got = _search(rows, rows, k, q_skip=np.arange(n))
    assert (got[1] != np.arange(n)[:, None]).all()
    for j in range(n):
        keep = np.flatnonzero(np.arange(n) != j)
        w_d2, w_idx, _, _, _ = P.neighbours(rows[j:j + 1], rows[keep], k)
        _assert_matches((got[0][j:j + 1], got[1][j:j + 1], None), (w_d2, keep[w_idx].astype(np.int32), None), d)
    full = _search(rows, rows, k)
    assert (full[1][:, 0] == np.arange(n)).all() and (full[0][:, 0] == 0).all()                    # without it every row finds itself
    some = np.where(np.arange(n) % 3 == 0, -1, (np.arange(n) + 1) % n)                            # -1 skips nothing; any index may be skipped
    _assert_matches(_search(rows, rows, k, q_skip=some), P.neighbours(rows, rows, k, q_skip=some, d2=d2_all), d)

    qg, rg = np.arange(33) % 4, np.array([0, 1, 2, 7])[np.arange(n) % 4]                            # group 3 has no reference, group 7 no query
    d2 = P.d2_matrix(other, rows)
    radius2 = (d2.mean(axis=0) * P.LD(0.41)).astype(np.float64)
    got = _search(other, rows, k, q_group=qg, r_group=rg, r_radius2=radius2)
    _assert_matches(got, P.neighbours(other, rows, k, qg, rg, None, radius2, d2=d2), d)
    for g in range(4):
        qi, ri = np.flatnonzero(qg == g), np.flatnonzero(rg == g)
        if not len(ri):
            assert (got[1][qi] == -1).all() and (got[2][qi] == 0).all()
            continue
        w_d2, w_idx, w_in, _, _ = P.neighbours(other[qi], rows[ri], k, r_radius2=radius2[ri])      # the restatement on the group alone
        _assert_matches((got[0][qi], got[1][qi], got[2][qi]), (w_d2, ri[w_idx].astype(np.int32), w_in), d)
    both = _search(rows, rows, k, q_group=rg, r_group=rg, q_skip=np.arange(n))                      # what ops.prdc asks for its radii
    _assert_matches(both, P.neighbours(rows, rows, k, rg, rg, np.arange(n), d2=d2_all), d)
    assert (both[1][:, 2] >= 0).all() and (rg[both[1]] == rg[:, None]).all()


# ------------------------------------------------------------------------------------------------ 5. non-finite values
def test_non_finite_rows_and_radii_are_never_chosen_and_never_counted():
    d, k = 64, 3
    refs, queries, _, _ = P.planted(13, 70, 12, d)
    d2 = P.d2_matrix(queries, refs)
    radius2 = (d2.mean(axis=0) * P.LD(0.9)).astype(np.float64)
    clean = _search(queries, refs, k, r_radius2=radius2)
    assert (clean[2] > 0).all()
    bad_r, bad_q, bad_rad = refs.copy(), queries.copy(), radius2.copy()
    near = clean[1][:, 0]
    bad_r[near[0], 5], bad_r[near[1], 63], bad_r[69, 0] = np.nan, np.inf, -np.inf          # the nearest reference of queries 0 and 1, and the last one
    bad_q[4, 17], bad_q[5, 0] = np.nan, np.inf
    gone = {int(near[0]), int(near[1]), 69}
    held = lambda j, taken: next(int(i) for i in np.argsort(d2[j]) if d2[j, i] <= radius2[i] and int(i) not in taken)
    ball2 = held(2, gone)                                                     # a ball that held query 2, another that held query 3
    ball3 = held(3, gone | {ball2})
    bad_rad[ball2], bad_rad[ball3], bad_rad[2] = np.nan, np.inf, -np.inf
    got = _search(bad_q, bad_r, k, r_radius2=bad_rad)
    want = P.neighbours(bad_q, bad_r, k, r_radius2=bad_rad)
    _assert_matches(got, want, d)
    assert not gone & set(got[1].ravel().tolist())
    assert (got[1][[4, 5]] == -1).all() and np.isinf(got[0][[4, 5]]).all() and (got[2][[4, 5]] == 0).all()
    ok = np.ones(70, bool)
    ok[list(gone | {ball2, ball3, 2})] = False
    with np.errstate(invalid='ignore'):
        assert got[2][2] == (d2[2, ok] <= radius2[ok]).sum() < clean[2][2] and got[2][3] < clean[2][3]     # a NaN / inf radius holds nothing
    all_bad = _search(queries, np.full_like(refs, np.nan), k, r_radius2=radius2)
    assert (all_bad[1] == -1).all() and (all_bad[2] == 0).all()


# ------------------------------------------------------------------------------------------------ 6. the four scores
@pytest.mark.parametrize('n,m,d,k', [(37, 53, 70, 3), (96, 160, 129, 5)])
def test_prdc_equals_the_restated_scores(n, m, d, k):
    from kpx_amd import ops
    for seed in (0, 1):
        real, fake, _, _ = P.planted(seed, n, m, d)
        want = P.prdc(real, fake, k)
        assert all(0.1 < want[s] < 0.9 for s in P.SCORES) and want['margin'] >= 1e-9       # the precondition: the sets test something, no near tie
        got = ops.prdc(_dev(real), _dev(fake), k)
        assert got['k'] == k and got['n_real'] == n and got['n_fake'] == m
        for s in P.SCORES:
            assert got[s].dtype == torch.float64 and got[s].dim() == 0
            assert float(got[s]) == want[s], (s, float(got[s]), want[s])                     # ratios of equal integers
        for key in ('real_inside', 'fake_inside', 'real_nn_idx'):
            assert np.array_equal(_host(got[key]), want[key]), key
        for key in ('real_radius2', 'fake_radius2', 'real_nn_d2'):
            assert np.all(np.abs(_host(got[key]).astype(P.LD) - want[key]) <= P.d2_bound(d) * want[key]), key
        rg, fg = (np.arange(n) % 3).astype(np.int32), (np.arange(m) % 4).astype(np.int32)   # group 3 has no real row: null
        want = P.prdc(real, fake, k, rg, fg)
        assert want['margin'] >= 1e-9 and all(0.0 < v < 1.0 for v in want['coverage'][:3])
        got = ops.prdc(_dev(real), _dev(fake), k, _dev(rg), _dev(fg))
        assert _host(got['groups']).tolist() == [0, 1, 2, 3]
        assert np.array_equal(_host(got['group_n_real']), want['group_n_real']) and np.array_equal(_host(got['group_n_fake']), want['group_n_fake'])
        for s in P.SCORES:
            assert P.equal_or_nan(_host(got[s]), want[s]), s
            assert np.isnan(_host(got[s])[3])
    few = ops.prdc(_dev(real[:k]), _dev(fake), k)                                            # fewer than k + 1 rows: null
    assert all(np.isnan(float(few[s])) for s in P.SCORES) and np.isinf(_host(few['real_radius2'])).all()
    none = ops.prdc(_dev(real[:0]), _dev(fake), k)
    assert all(np.isnan(float(none[s])) for s in P.SCORES) and none['real_inside'].shape == (0,) and (_host(none['fake_inside']) == 0).all()


# ------------------------------------------------------------------------------------------------ 7. chunks
def test_more_than_4096_queries_go_in_two_calls():
    from kpx_amd import _lib, ops
    rs = np.random.RandomState(3)
    q, r = _dev(rs.randn(4097, 4)), _dev(rs.randn(50, 4))
    radius2 = _dev(np.full(50, 2.0))
    skip = _dev((np.arange(4097) % 50).astype(np.int32))
    calls = _lib.abi_calls[0]
    whole = ops.set_neighbours(q, r, 3, q_skip=skip, r_radius2=radius2)
    assert _lib.abi_calls[0] == calls + 2
    head = ops.set_neighbours(q[:4096], r, 3, q_skip=skip[:4096], r_radius2=radius2)
    tail = ops.set_neighbours(q[4096:], r, 3, q_skip=skip[4096:], r_radius2=radius2)
    for w, h, t in zip(whole, head, tail):
        assert torch.equal(w.view(torch.int64) if w.dtype == torch.float64 else w, torch.cat([h, t]).view(torch.int64) if w.dtype == torch.float64 else torch.cat([h, t]))
    assert (_host(whole[1]) != _host(skip)[:, None]).all() and 0 < _host(whole[2]).sum() < 4097 * 50
    with pytest.raises(_lib.KpxError):
        ops.set_neighbours(q, r[:, :3].contiguous(), 3)


# ------------------------------------------------------------------------------------------------ 8. evaluate.py --prdc end to end
def _expected_arrays(store, k):
    """the restatement on every comparison of the stored rows: {name: P.prdc(...)}"""
    real_own, parity = store['own'], store['parity']
    out = {}
    for sp in sorted(key[:-5] for key in store if key.endswith('_real')):
        real, fake = store[sp + '_real'].astype(np.float64), store[sp + '_fake'].astype(np.float64)
        draws = fake.shape[0]
        flat = fake.reshape(-1, fake.shape[-1])
        even, odd = parity == 0, parity == 1
        cases = {'draw0': (real, fake[0], None, None), 'all_draws': (real, flat, None, None), 'ceiling': (real[odd], real[even], None, None),
                 'draw0_per_class': (real, fake[0], real_own, real_own), 'all_draws_per_class': (real, flat, real_own, np.tile(real_own, draws)),
                 'ceiling_per_class': (real[odd], real[even], real_own[odd], real_own[even])}
        if sp + '_commanded' in store:
            for c, a in enumerate(store['actions'].tolist()):
                cases['commanded_%d' % a] = (real[real_own == a], store[sp + '_commanded'][c].astype(np.float64), None, None)
        for name, (x, y, xg, yg) in cases.items():
            out['%s_%s' % (sp, name)] = P.prdc(x, y, k, xg, yg)
    return out


def test_evaluate_prdc_end_to_end(tmp_path, capsys):
    import yaml
    import kpx_amd
    import evaluate
    from kpx_amd import prdc
    data = tmp_path / 'penn'
    S.write_dataset(data)                                                    # the fixture videos of test_novelty_gpu.py: 7 test samples, K = 5, A = 9
    cfg = {'paths': {'data_dir': str(data), 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': S.K, 'n_action': S.N_ACTION, 'cell_info': [32, 32], 'vae_dim': 8, 'classifier_cells': [32, 16]}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    cls = kpx_amd.ActionClassifierModel(cfg, device=DEV)                       # a freshly initialised recogniser
    cls.build()
    cls.initialize_loggers(str(tmp_path / 'cls'))
    cls_ckpt = cls.save_checkpoint(None, 0)
    cls.close_loggers()

    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics', '--samples', '2']
    flags = ['--prdc', '--prdc-k', '1']
    quiet = ['--no-save']                                                      # the PNGs are compared once, on the first pair of runs
    runs = (('prdc', flags), ('act', flags + quiet + ['--actions', 'all']), ('acc', flags + quiet + ['--action-accuracy', cls_ckpt]), ('plain', []),
            ('acc_plain', quiet + ['--action-accuracy', cls_ckpt]))
    for name, extra in runs:
        torch.manual_seed(11)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
    capsys.readouterr()

    own = np.array([int(line.split()[1]) for line in open(str(data / 'test_set.txt')).read().splitlines()], np.int32)
    n = len(own)
    assert n == 7
    for name, spaces, commanded in (('prdc', ['kp'], False), ('act', ['kp'], True), ('acc', ['cls', 'kp'], False)):
        ev = tmp_path / name
        with np.load(str(ev / 'prdc.npz')) as f:
            store = {key: f[key] for key in f.files}
        assert int(store.pop('k')) == 1 and np.array_equal(store['own'], own) and store['parity'].tolist() == [0, 1, 0, 1, 0, 1, 0]
        assert store['kp_real'].dtype == np.float32 and store['kp_real'].shape == (n, 32 * S.K * 2) and store['kp_fake'].shape == (2, n, 32 * S.K * 2)
        if 'cls' in spaces:
            assert store['cls_real'].shape == (n, 16) and store['cls_fake'].shape == (2, n, 16) and store['cls_fake'].dtype == np.float32
        if commanded:
            assert store['actions'].tolist() == list(range(S.N_ACTION)) and store['kp_commanded'].shape == (S.N_ACTION, n, 32 * S.K * 2)
        npz = np.load(str(ev / 'metrics.npz'))
        blk = json.load(open(str(ev / 'metrics.json')))['prdc']
        assert blk['k'] == 1 and blk['spaces'] == spaces and blk['definition'] == prdc.DEFINITION and int(npz['prdc_k']) == 1
        want = _expected_arrays(store, 1)
        assert sorted(want) == sorted('%s_%s' % (sp, c) for sp in spaces for c in blk[sp])
        num = lambda v: None if np.isnan(v) else float(v)
        for comparison, w in want.items():
            sp, short = comparison.split('_', 1)
            d = store[sp + '_real'].shape[1]
            get = lambda key: npz['prdc_%s_%s' % (comparison, key)]
            print('%s %s: margin %.3e' % (name, comparison, w['margin']))
            assert w['margin'] >= 1e-9, (comparison, w['margin'])                 # the precondition: no distance within 1e-9 of its radius
            assert int(get('n_real')) == w['n_real'] == blk[sp][short]['n_real'] and int(get('n_fake')) == w['n_fake'] == blk[sp][short]['n_fake']
            for key in ('real_inside', 'fake_inside', 'real_nn_idx'):
                assert np.array_equal(get(key), w[key]), (comparison, key)
            for key in ('real_radius2', 'fake_radius2', 'real_nn_d2'):
                fin = np.isfinite(w[key])
                assert np.array_equal(get(key)[~fin], w[key][~fin].astype(np.float64)), (comparison, key)
                assert np.all(np.abs(get(key)[fin].astype(P.LD) - w[key][fin]) <= P.d2_bound(d) * w[key][fin]), (comparison, key)
            for s in P.SCORES:
                assert P.equal_or_nan(get(s), w[s]), (comparison, s)
                assert blk[sp][short][s] == (num(w[s]) if 'groups' not in w else [num(v) for v in w[s]]), (comparison, s)
            if 'groups' in w:
                assert blk[sp][short]['classes'] == w['groups'].tolist() and np.array_equal(get('groups'), w['groups'])
        assert blk['kp']['draw0']['n_real'] == blk['kp']['draw0']['n_fake'] == n and blk['kp']['all_draws']['n_fake'] == 2 * n
        assert blk['kp']['ceiling']['n_real'] == 3 and blk['kp']['ceiling']['n_fake'] == 4
        assert all(blk['kp']['draw0'][s] is not None for s in P.SCORES)
        assert blk == json.loads(json.dumps(prdc.summarise({key: npz[key] for key in npz.files})))
        capsys.readouterr()                                                   # the margins printed above
        assert prdc.main([str(ev / 'prdc.npz')]) == 0                         # the CPU re-scorer reproduces the block
        assert json.loads(capsys.readouterr().out) == blk

    # without --prdc every output keeps its bytes: the plain runs against the entries the flag leaves alone
    for with_flag, without in (('prdc', 'plain'), ('acc', 'acc_plain')):
        a, b = np.load(str(tmp_path / without / 'metrics.npz')), np.load(str(tmp_path / with_flag / 'metrics.npz'))
        assert not [key for key in a.files if key.startswith('prdc')] and set(a.files) == {key for key in b.files if not key.startswith('prdc')}
        for key in a.files:
            assert a[key].tobytes() == b[key].tobytes() and a[key].dtype == b[key].dtype, key
        ja, jb = (json.load(open(str(tmp_path / d / 'metrics.json'))) for d in (without, with_flag))
        assert 'prdc' not in ja and ja == {key: v for key, v in jb.items() if key != 'prdc'}
        assert not (tmp_path / without / 'prdc.npz').exists()
        pngs = 0
        for root, _, files in os.walk(str(tmp_path / without)):
            for name in files:
                if name.endswith('.png'):
                    other = os.path.join(str(tmp_path / with_flag), os.path.relpath(os.path.join(root, name), str(tmp_path / without)))
                    assert open(os.path.join(root, name), 'rb').read() == open(other, 'rb').read(), other
                    pngs += 1
        assert pngs > 7 * 32 if without == 'plain' else pngs == 0
    assert sorted(np.load(str(tmp_path / 'plain' / 'metrics.npz')).files) == ['mse', 'psnr', 'ssim']
