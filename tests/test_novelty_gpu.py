"""GPU: the nearest-motion search of csrc/novelty.hip (kpx_amd.novelty.MotionStore, ops.seq_nearest) against the float64 restatement of
tests/novelty_ref.py -- the window values against the existing gather, the distances within 1e-12, the argmin and its tie rules, position
independence bit for bit, the exclusion, non-finite values -- and evaluate.py --novelty end to end."""
import json
import os

import numpy as np
import pytest
import torch

import novelty_ref as N
import resident_seq_ref as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ABSENT = [0, 2, 3, 5, 6]                     # the classes write_dataset lists no video under


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.cpu().numpy()


def _store_from_arrays(names, counts, arrays, listing, k, n_action=S.N_ACTION):
    """-> (MotionStore, table, frames): a store without files, and the restatement's own table and window frames for it"""
    from kpx_amd import novelty, resident
    idx = resident.LabelIndex(names, counts, arrays, [line.split()[1] for line in listing], k)
    store = novelty.MotionStore(None, listing, k, n_action, DEV, index=idx)
    table, _ = N.enumerate_windows(listing, dict(zip(names, counts)), {name: v for v, name in enumerate(names)})
    assert (store.windows.table == table).all()
    return store, table, N.window_frames(arrays, table)


@pytest.fixture(scope='module')
def small(tmp_path_factory):
    """The 35-window store of resident_seq_ref.write_dataset (K = 5, A = 9), read from its files."""
    from kpx_amd import novelty
    root = tmp_path_factory.mktemp('novelty_gpu') / 'penn'
    labels = S.write_dataset(root)
    with open(os.path.join(str(root), 'train_set.txt')) as f:
        listing = f.read().splitlines()
    store = novelty.MotionStore(str(root), listing, S.K, S.N_ACTION, DEV)
    names = [S.video_name(v) for v in range(len(S.FRAMES))]
    table, _ = N.enumerate_windows(listing, dict(zip(names, S.FRAMES)), {name: v for v, name in enumerate(names)})
    assert (store.windows.table == table).all() and table.shape == (35, 4)
    arrays = [labels[name] for name in names]
    return {'root': str(root), 'store': store, 'table': table, 'frames': N.window_frames(arrays, table), 'arrays': arrays, 'names': names,
            'listing': listing}


def _queries(seed, q, k):
    return (np.random.RandomState(seed).rand(q, 32, k, 2) * 2.0 - 1.0).astype(np.float32)


def test_the_search_reads_the_windows_the_gather_delivers(small):
    store, table, frames = small['store'], small['table'], small['frames']
    codes = np.arange(2 * 35)
    got = store.gather(codes)
    assert got.shape == (70, 32, S.K, 2) and got.dtype == torch.float32
    want = np.repeat(frames, 2, axis=0)
    want[1::2, ..., 0] *= np.float32(-1)
    assert np.array_equal(S.bits(got), S.bits(want))                 # the gather with no flag / SEQ_FLIP = the restatement's frames, bit for bit
    d2, code = store.nearest(got)
    d2, code = _host(d2), _host(code)
    same = {0: 33, 1: 34, 33: 0, 34: 1}                              # the doubled line: the same data under a second id and class
    for i, c in enumerate(codes):
        w, m = c >> 1, c & 1
        for ww in (w, same.get(w)):
            if ww is not None:
                a = table[ww, 3]
                assert d2[i, a] == 0.0 and code[i, a] == 2 * ww + m, (i, ww)
    assert np.isinf(d2[:, ABSENT]).all() and (code[:, ABSENT] == -1).all()


@pytest.mark.parametrize('mirror', [True, False])
@pytest.mark.parametrize('q', [1, 3, 65])
def test_distances_and_argmin_on_the_small_store(small, q, mirror):
    store, table, frames = small['store'], small['table'], small['frames']
    queries = _queries(100 + q, q, S.K)
    want = N.nearest(queries, frames, table, S.N_ACTION, mirror)
    d2, code = store.nearest(_dev(queries), mirror=mirror)
    assert d2.dtype == torch.float64 and code.dtype == torch.int32 and d2.shape == (q, S.N_ACTION)
    N.assert_matches(_host(d2), _host(code), *want)
    assert np.isinf(_host(d2)[:, ABSENT]).all() and (_host(code)[:, ABSENT] == -1).all()
    assert np.isfinite(_host(d2)[:, [1, 4, 7, 8]]).all()
    if not mirror:
        assert (_host(code)[:, [1, 4, 7, 8]] % 2 == 0).all()


def test_distances_and_argmin_on_a_larger_store_from_arrays():
    names, counts, arrays, listing = N.array_store(seed=7)
    assert set((17, 32, 33, 65, 66, 200)) <= set(counts) and len(counts) == 70
    store, table, frames = _store_from_arrays(names, counts, arrays, listing, 40)
    w = table.shape[0]
    assert w % 4 and w % 16 and w % 64 and (table[:, 2] == 0).any() and (table[:, 2] == 1).any() and (table[:, 2] >= 2).any()
    queries = _queries(8, 7, 40)
    queries[3] = frames[w // 2] + np.float32(0.01) * queries[3]      # one query close to a window, the others far from all
    want = N.nearest(queries, frames, table, S.N_ACTION, True)
    d2, code = store.nearest(_dev(queries))
    N.assert_matches(_host(d2), _host(code), *want)
    assert _host(code)[3, table[w // 2, 3]] == 2 * (w // 2)


def test_planted_exact_ties_go_to_the_lowest_code():
    rs = np.random.RandomState(21)
    k = 5
    a = (rs.rand(40, k, 2) * 2.0 - 1.0).astype(np.float32)
    b = (rs.rand(35, k, 2) * 2.0 - 1.0).astype(np.float32)
    b[..., 0] = np.where(rs.rand(35, k) < 0.5, np.float32(0.0), np.float32(-0.0))          # x = +-0.0: every window ties with its mirror
    names, counts, arrays = ['frames/0001', 'frames/0002'], [40, 35], [a, b]
    listing = ['frames/0001 2', 'frames/0001 2', 'frames/0002 3', 'frames/0001 5']           # windows 0-7, 8-15 (the same, same class), 16-18, 19-26
    store, table, frames = _store_from_arrays(names, counts, arrays, listing, k)
    assert table.shape[0] == 27 and np.array_equal(S.bits(frames[:8]), S.bits(frames[8:16]))
    noise = np.float32(1e-3) * _queries(22, 4, k)
    queries = np.stack([frames[3], frames[13], frames[17], frames[22]]) + noise
    want_d2, want_code, runner = N.nearest(queries, frames, table, S.N_ACTION, True)
    planted = np.zeros(want_d2.shape, bool)
    planted[:, [2, 3]] = True                                        # class 2: every window twice; class 3: every window equals its mirror
    assert not N.clear_margin(want_d2, runner)[:, [2, 3]].any()      # ... exact ties in the restatement, for every query
    d2, code = store.nearest(_dev(queries))
    d2, code = _host(d2), _host(code)
    N.assert_matches(d2, code, want_d2, want_code, runner, planted)
    assert code[0, 2] == 2 * 3 and code[1, 2] == 2 * 5 and code[3, 2] == 2 * 3           # the lower of the two ids, never 11 / 13
    assert code[2, 3] == 2 * 17 and (code[:, 3] % 2 == 0).all()                          # m = 0 wins against its equal mirror
    assert code[0, 5] == 2 * 22 and code[3, 5] == 2 * 22                                 # a class present through the duplicate line alone
    assert np.array_equal(d2[:, 5].view(np.int64), d2[:, 2].view(np.int64))              # ... at the same distance, bit for bit


def test_a_distance_depends_on_neither_the_querys_nor_the_windows_position(small):
    from kpx_amd import ops
    store, table = small['store'], small['table']
    queries = _queries(31, 65, S.K)
    queries[64] = queries[0]
    d2, code = store.nearest(_dev(queries))
    d2, code = _host(d2), _host(code)
    assert np.array_equal(d2[0].view(np.int64), d2[64].view(np.int64)) and np.array_equal(code[0], code[64])
    one, _ = store.nearest(_dev(queries[:1]))                        # the same query alone: another Q, another grid
    assert np.array_equal(_host(one)[0].view(np.int64), d2[0].view(np.int64))
    # the same store with a line in front (a new video under class 0, which had none): every id moves, no distance does
    extra = (np.random.RandomState(32).rand(50, S.K, 2) * 2.0 - 1.0).astype(np.float32)
    names = ['frames/0099'] + small['names']
    moved, table2, _ = _store_from_arrays(names, [50] + list(S.FRAMES), [extra] + small['arrays'], ['frames/0099 0'] + small['listing'], S.K)
    shift = 50 - 33 + 1
    assert table2.shape[0] == 35 + shift and (table2[shift:, 1:] == table[:, 1:]).all() and (table2[shift:, 0] == table[:, 0] + 1).all()
    d2m, codem = moved.nearest(_dev(queries))
    d2m, codem = _host(d2m), _host(codem)
    present = [1, 4, 7, 8]
    assert np.array_equal(d2m[:, present].view(np.int64), d2[:, present].view(np.int64))
    assert np.array_equal(codem[:, present], code[:, present] + 2 * shift)
    assert np.isfinite(d2m[:, 0]).all() and (codem[:, 0] < 2 * shift).all()
    # the wrapper on the store's own tensors writes into the caller's outputs
    out = (torch.empty((65, S.N_ACTION), dtype=torch.float64, device=DEV), torch.empty((65, S.N_ACTION), dtype=torch.int32, device=DEV))
    got = ops.seq_nearest(store.labels.labels, store.labels.label_off, store.table, store.order, store.group_first, _dev(queries), out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert np.array_equal(_host(out[0]).view(np.int64), d2.view(np.int64)) and np.array_equal(_host(out[1]), code)


def test_exclude_video_equals_the_store_without_that_videos_lines(small):
    store, table, frames = small['store'], small['table'], small['frames']
    src = [0, 20, 34, 8, 15]                                         # windows of videos 0, 4, 0 (the doubled line), 2, 3
    queries = frames[src] + np.float32(0.05) * _queries(41, len(src), S.K)
    exclude = table[src, 0].astype(np.int32)
    exclude[3] = -1                                                  # one query excludes nothing
    d2, code = store.nearest(_dev(queries), exclude_video=_dev(exclude))
    d2, code = _host(d2), _host(code)
    for i in range(len(src)):
        keep = np.flatnonzero(table[:, 0] != exclude[i])
        w_d2, w_code, runner = N.nearest(queries[i:i + 1], frames[keep], table[keep], S.N_ACTION, True)
        w_code = np.where(w_code >= 0, 2 * keep[np.maximum(w_code, 0) >> 1] + (w_code & 1), -1).astype(np.int32)       # back to the full table's ids
        N.assert_matches(d2[i:i + 1], code[i:i + 1], w_d2, w_code, runner)
        if exclude[i] >= 0:
            assert (table[code[i][code[i] >= 0] >> 1, 0] != exclude[i]).all()
    assert code[3, table[8, 3]] == 2 * 8                             # without exclusion the query finds the window it was made from
    assert np.isinf(d2[0, 8]) and code[0, 8] == -1 and np.isinf(d2[2, 8]) and code[2, 8] == -1      # class 8 holds video 0 alone: emptied
    full, _ = store.nearest(_dev(queries))
    assert np.isfinite(_host(full)[:, 8]).all()


def test_non_finite_values_are_never_chosen(small):
    store = small['store']
    queries = _queries(51, 3, S.K)
    clean, clean_code = store.nearest(_dev(queries))
    bad = queries.copy()
    bad[1, 5, 2, 0] = np.nan
    d2, code = store.nearest(_dev(bad))
    d2, code = _host(d2), _host(code)
    assert np.isinf(d2[1]).all() and (d2[1] > 0).all() and (code[1] == -1).all()
    assert np.array_equal(d2[[0, 2]].view(np.int64), _host(clean)[[0, 2]].view(np.int64)) and np.array_equal(code[[0, 2]], _host(clean_code)[[0, 2]])
    # a store row holding an Inf: the windows that read it are never chosen
    arrays = [a.copy() for a in small['arrays']]
    arrays[2][20, 3, 1] = np.inf                                     # video 2 (40 rows, gap 1): every one of its 8 windows reads row 20
    arrays[4][31, 0, 0] = -np.inf                                    # video 4 (short form): only the last window, rows 15..31, reads row 31
    holed, table, frames = _store_from_arrays(small['names'], list(S.FRAMES), arrays, small['listing'], S.K)
    want = N.nearest(queries, frames, table, S.N_ACTION, True)
    d2, code = holed.nearest(_dev(queries))
    d2, code = _host(d2), _host(code)
    N.assert_matches(d2, code, *want)
    chosen = code[code >= 0] >> 1
    assert np.isfinite(frames[chosen]).all() and not (table[chosen, 0] == 2).any() and 31 not in chosen.tolist()
    assert np.isfinite(d2[:, 4]).all()                               # class 4 still has video 1 and the other windows of video 4


def test_evaluate_novelty_end_to_end(tmp_path, monkeypatch, small):
    import yaml
    from PIL import Image
    import kpx_amd
    import evaluate
    data, table, frames = small['root'], small['table'], small['frames']
    cfg = {'paths': {'data_dir': data, 'vggnet': str(tmp_path / 'none.npy'), 'log_dir': str(tmp_path / 'results')},
           'training': {'n_steps': 1, 'summary_interval': 500, 'test_interval': 500, 'checkpoint_interval': 1000, 'log_interval': 1,
                        'batch_size': 2, 'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}},
           'model': {'n_pts': S.K, 'n_action': S.N_ACTION, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)

    calls = []
    run = kpx_amd.FinalModel.run

    def recording_run(self, sess, feed_dict, z=None):
        out = run(self, sess, feed_dict, z=z)
        calls.append(out['fut_pt_raw'].cpu().numpy().copy())
        return out

    monkeypatch.setattr(kpx_amd.FinalModel, 'run', recording_run)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--batch', '2', '--metrics', '--samples', '2']
    recorded = {}
    for name, extra in (('nov', ['--novelty', '--novelty-sheets']), ('act', ['--novelty', '--novelty-sheets', '--actions', '1,4']), ('plain', [])):
        del calls[:]
        torch.manual_seed(11)
        evaluate.main(base + extra + ['--save_dir', str(tmp_path / name)])
        recorded[name] = list(calls)

    n_samples, d = 7, 2
    videos = [int(small['names'].index(line.split()[0])) for line in small['listing']]       # train = test: sample s is listing line s
    real = np.stack([frames[np.flatnonzero((table[:, 0] == v) & (table[:, 1] == 0))[0]] for v in videos])     # the loader's un-augmented start-0 futures

    def over_classes(d2, code):
        """the minimum over the classes of one query, ties to the lowest code"""
        best, at = np.inf, -1
        for a in range(S.N_ACTION):
            if code[a] >= 0 and (d2[a] < best or (d2[a] == best and code[a] < at)):
                best, at = d2[a], code[a]
        return best, at

    def expected(query, s):
        d2, code, runner = N.nearest(query[None], frames, table, S.N_ACTION, True, exclude=np.array([videos[s]]))
        assert N.clear_margin(d2, runner).all()
        low, at = over_classes(d2[0], code[0])          # classes 1 and 8 share video 0's windows: such a tie goes to the lowest code
        return np.sqrt(low), at, np.sqrt(d2[0])

    def close(got, want):
        got, want = np.atleast_1d(got), np.atleast_1d(want)
        fin = np.isfinite(want)                                        # an absent or emptied class: +inf on both sides
        return np.array_equal(got[~fin], want[~fin]) and np.all(np.abs(got[fin] - want[fin]) <= 1e-12 * np.abs(want[fin]))

    for name, per_draw in (('nov', 1), ('act', 3)):
        ev = tmp_path / name
        npz = np.load(str(ev / 'metrics.npz'))
        rec = recorded[name]
        assert len(rec) == 4 * d * per_draw                            # batches of 2, 2, 2 and 1
        assert npz['nov_d'].shape == (n_samples, d) and npz['nov_code'].shape == (n_samples, d) and npz['nov_code'].dtype == np.int32
        assert npz['nov_class_d'].shape == (n_samples, d, S.N_ACTION) and npz['nov_window'].shape == (n_samples, d, 4)
        assert npz['nov_real_d'].shape == (n_samples,) and npz['nov_real_window'].shape == (n_samples, 4) and npz['nov_d'].dtype == np.float64
        assert np.array_equal(npz['nov_own'], [int(line.split()[1]) for line in small['listing']])
        assert np.array_equal(npz['nov_window_action'], table[:, 3])
        for s in range(n_samples):
            b, i = divmod(s, 2)
            w_d, w_code, w_class = expected(real[s], s)
            assert close(npz['nov_real_d'][s], w_d) and npz['nov_real_code'][s] == w_code
            assert table[w_code >> 1, 0] != videos[s]                  # the real future does not find its own video
            for draw in range(d):
                kp = rec[(b * d + draw) * per_draw][i]
                w_d, w_code, w_class = expected(kp, s)
                assert close(npz['nov_d'][s, draw], w_d) and npz['nov_code'][s, draw] == w_code, (s, draw)
                assert close(npz['nov_class_d'][s, draw], w_class)
                line = np.flatnonzero(np.cumsum([0, 2, 5, 8, 1, 16, 1, 2]) <= (w_code >> 1))[-1]
                assert npz['nov_window'][s, draw].tolist() == [line, table[w_code >> 1, 1], table[w_code >> 1, 2], w_code & 1]
                if per_draw > 1:
                    for c in range(2):
                        w_d, w_code, _ = expected(rec[(b * d + draw) * per_draw + 1 + c][i], s)
                        assert close(npz['act_nov_d'][s, c, draw], w_d) and npz['act_nov_code'][s, c, draw] == w_code
        blk = json.load(open(str(ev / 'metrics.json')))['novelty']
        assert blk['definition'] == evaluate.NOVELTY_DEFINITION and blk['n_windows'] == 35 and blk['n_pred'] == 14 and blk['n_real'] == 7
        assert blk['copy_threshold'] is None and blk['copied'] is None and blk['n_nonfinite'] == 0 and blk['mirror'] is True
        assert blk['ratio'] == float(np.median(npz['nov_d']) / np.median(npz['nov_real_d'])) and blk['nn_top1']['chance'] == 0.25
        assert ('commanded' in blk['nn_top1']) == (per_draw > 1)
        assert blk == json.loads(json.dumps(evaluate.summarise_novelty({key: npz[key] for key in npz.files})))
        for s in range(n_samples):
            im = Image.open(str(ev / ('%04d' % s) / 'nearest.png'))
            assert im.size == (8 * 128, (1 + 2 * d) * 128) and im.mode == 'RGB'
            rows = np.asarray(im).reshape(1 + 2 * d, 128, 8 * 128, 3)
            assert all(r.any() for r in rows)                          # every row drew its key points
    plain, nov = np.load(str(tmp_path / 'plain' / 'metrics.npz')), np.load(str(tmp_path / 'nov' / 'metrics.npz'))
    assert sorted(plain.files) == ['mse', 'psnr', 'ssim'] and set(plain.files) < set(nov.files)
    for key in plain.files:                                            # without the flags every pre-existing entry keeps its bytes
        assert plain[key].tobytes() == nov[key].tobytes() and plain[key].dtype == nov[key].dtype
    assert 'novelty' not in json.load(open(str(tmp_path / 'plain' / 'metrics.json')))
    assert not (tmp_path / 'plain' / '0000' / 'nearest.png').exists()
