"""CPU: the host half of evaluate.py --novelty -- the candidate windows (kpx_amd.novelty.WindowIndex) against what SequenceDataLoader.plan()
draws, the table's validation, the class-grouped order, the ``novelty`` block of metrics.json on hand-made arrays, the argument errors of
evaluate.py and of the wrapper and the C entry, none of which needs a GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import novelty_ref as N
import resident_seq_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp('novelty_cpu') / 'penn'
    labels = S.write_dataset(root)
    with open(os.path.join(str(root), 'train_set.txt')) as f:
        listing = f.read().splitlines()
    return str(root), labels, listing


def _index(dataset):
    from kpx_amd import novelty, resident
    root, _, listing = dataset
    idx = resident.LabelIndex.scan(root, listing, S.K)
    return idx, novelty.WindowIndex(idx, listing)


def test_constants_mirror_the_header():
    from kpx_amd import novelty, ops, tool_ops
    src = open(os.path.join(REPO, 'include', 'kpx.h')).read()
    val = lambda name: eval(re.search(r'#define\s+%s\s+(.+)' % name, src).group(1))
    assert novelty.NEAREST_ROW_INTS == val('KPX_NEAREST_ROW_INTS') and novelty.NEAREST_GROUP == val('KPX_NEAREST_GROUP')
    assert novelty.NEAREST_MAX_QUERIES == val('KPX_NEAREST_MAX_QUERIES') == 4096
    assert novelty.NEAREST_MAX_WINDOWS == val('KPX_NEAREST_MAX_WINDOWS') == 2 ** 30 - 1
    assert val('KPX_ABI_VERSION') == 25
    assert ops.seq_nearest is tool_ops.seq_nearest is novelty.seq_nearest and ops.NEAREST_MAX_QUERIES == 4096


def test_the_windows_are_the_sequences_plan_can_draw(dataset):
    root, labels, listing = dataset
    idx, win = _index(dataset)
    assert len(win) == 2 + 5 + 8 + 1 + 16 + 1 + 2 == 35 and win.table.dtype == np.int32 and win.table.shape == (35, 4)
    counts = {S.video_name(v): n for v, n in enumerate(S.FRAMES)}
    numbers = {S.video_name(v): v for v in range(len(S.FRAMES))}
    table, line = N.enumerate_windows(listing, counts, numbers)
    assert (win.table == table).all() and (win.line == line).all()
    assert (np.diff(win.line) >= 0).all()                                       # listing order ...
    for li in range(len(listing)):                                              # ... every line's starts ascending from 0 to the last legal one
        rows = win.table[win.line == li]
        n = counts[listing[li].split()[0]]
        assert rows[:, 1].tolist() == list(range(S.last_im_idx(n) + 1))
        assert (rows[:, 2] == int(n / 33)).all() and (rows[:, 3] == int(listing[li].split()[1])).all()
    assert (win.table[win.line == 0][:, :3] == win.table[win.line == 6][:, :3]).all()          # the doubled line: the same data, its own action
    assert win.table[win.line == 0][0, 3] != win.table[win.line == 6][0, 3]
    have = {(int(r[0]), int(r[1]), int(r[3])) for r in win.table}
    ld = S.loader(root, random_order=True, randomness=True, seed=5)
    drawn = set()
    for _ in range(400):
        for p in ld.plans():
            key = (numbers[p.video], p.im_idx, int(listing[p.index].split()[1]))
            assert key in have, p
            drawn.add(key)
    assert len(drawn) == 35                                                     # and the loader reaches every window of the table
    win.check(S.N_ACTION)


def test_check_refuses_a_window_that_leaves_its_video(dataset):
    from kpx_amd._lib import KpxError
    idx, win = _index(dataset)
    for edit, text in (((0, 1, 4), 'leaves'), ((34, 1, 4), 'leaves'), ((20, 1, 16), 'leaves'), ((3, 1, -1), 'leaves'), ((3, 2, -1), 'leaves'),
                       ((5, 0, 6), 'video number'), ((5, 0, -1), 'video number'), ((7, 3, 9), 'action'), ((7, 3, -1), 'action')):
        t = win.table.copy()
        t[edit[0], edit[1]] = edit[2]
        with pytest.raises(KpxError, match=text):
            win.check(S.N_ACTION, t)
    t = win.table.copy()
    t[0, 2] = 4                                                                 # video 0 has 100 rows: gap 4 from start 0 needs row 128
    with pytest.raises(KpxError, match='leaves'):
        win.check(S.N_ACTION, t)
    for bad in (win.table.astype(np.int64), win.table[:, :3], win.table[:0]):
        with pytest.raises(KpxError, match='windows: int32'):
            win.check(S.N_ACTION, bad)


def test_plan_groups_the_windows_by_class_in_padded_blocks(dataset):
    from kpx_amd import novelty
    idx, win = _index(dataset)
    order, first = win.plan(S.N_ACTION)
    g = novelty.NEAREST_GROUP
    assert order.dtype == first.dtype == np.int32 and first.shape == (S.N_ACTION + 1,) and order.shape == (first[-1] * g,)
    assert sorted(order[order >= 0].tolist()) == list(range(35))
    for a in range(S.N_ACTION):
        block = order[first[a] * g:first[a + 1] * g]
        ids = block[block >= 0]
        assert ids.tolist() == np.flatnonzero(win.table[:, 3] == a).tolist()    # ascending inside the class
        assert (block[len(ids):] == -1).all()                                   # the pads close the class's last block
        assert first[a + 1] - first[a] == (len(ids) + g - 1) // g
    assert [int(first[a + 1] - first[a]) for a in range(S.N_ACTION)] == [0, 1, 0, 0, 1, 0, 0, 1, 1]      # classes 1, 4, 7, 8 have windows
    desc = win.describe(np.array([[0, 1], [69, -1]]))
    assert desc.tolist() == [[[0, 0, 3, 0], [0, 0, 3, 1]], [[6, 1, 3, 1], [-1, -1, -1, -1]]]


def test_nearest_over_classes_takes_the_lowest_code_of_the_minimum():
    import evaluate
    d2 = np.array([[3.0, 1.0, 1.0, np.inf], [np.inf] * 4, [2.0, np.inf, np.inf, np.inf]])
    code = np.array([[4, 9, 6, -1], [-1] * 4, [11, -1, -1, -1]])
    low, best = evaluate.nearest_over_classes(d2, code)
    assert low.tolist() == [1.0, np.inf, 2.0] and best.tolist() == [6, -1, 11] and best.dtype == np.int32


def _arrays(n_real=24):
    """24 samples x 2 draws over a store of 6 windows in classes (0, 0, 1, 1, 2, 2); sample s has class s % 3."""
    rs = np.random.RandomState(3)
    s, d = n_real, 2
    own = (np.arange(s) % 3).astype(np.int32)
    real_d = 0.5 + rs.rand(s)
    real_code = (2 * (2 * own) + (np.arange(s) % 2)).astype(np.int32)           # window 2 * class: always the own class
    nov_d = 0.25 + rs.rand(s, d)
    nov_code = np.stack([2 * (2 * own + 1), 2 * ((2 * own + 2) % 6) + 1], 1).astype(np.int32)     # draw 0 own class, draw 1 the next class, mirrored
    return {'nov_window_action': np.array([0, 0, 1, 1, 2, 2], np.int32), 'nov_own': own, 'nov_real_d': real_d, 'nov_real_code': real_code,
            'nov_d': nov_d, 'nov_code': nov_code}


def test_the_novelty_block_on_hand_made_arrays():
    import evaluate
    a = _arrays()
    r = evaluate.summarise_novelty(a)
    assert r['definition'] == evaluate.NOVELTY_DEFINITION and 'not comparable with published figures' in r['definition']
    assert r['n_windows'] == 6 and r['n_pred'] == 48 and r['n_real'] == 24 and r['n_nonfinite'] == 0 and r['mirror'] is True
    for name, x in (('pred', a['nov_d'].ravel()), ('real', a['nov_real_d'])):
        assert r[name] == {'mean': float(x.mean()), 'median': float(np.median(x)), 'p05': float(np.percentile(x, 5))}
    assert r['ratio'] == float(np.median(a['nov_d']) / np.median(a['nov_real_d']))
    assert r['copy_threshold'] == r['real']['p05']
    assert r['copied'] == float((a['nov_d'] < r['copy_threshold']).mean())
    assert r['nn_top1'] == {'chance': 1.0 / 3, 'real': 1.0, 'pred': 0.5} and r['mirrored'] == 0.5
    assert json.loads(json.dumps(r, allow_nan=False)) == r

    few = evaluate.summarise_novelty(_arrays(19))                               # below 20 real samples: no threshold, no share
    assert few['copy_threshold'] is None and few['copied'] is None and few['ratio'] is not None

    # a rollout that found nothing (code -1, d +inf), one with a NaN distance and a real future without a window: counted, and in no figure
    b = _arrays()
    b['nov_d'][0, 0], b['nov_code'][0, 0] = np.inf, -1
    b['nov_d'][1, 1] = np.nan
    b['nov_real_d'][2], b['nov_real_code'][2] = np.inf, -1
    r = evaluate.summarise_novelty(b, mirror=False)
    keep = np.ones((24, 2), bool)
    keep[0, 0] = keep[1, 1] = False
    rk = np.arange(24) != 2
    assert r['n_nonfinite'] == 3 and r['n_pred'] == 46 and r['n_real'] == 23 and r['mirror'] is False
    assert r['pred']['mean'] == float(b['nov_d'][keep].mean()) and r['real']['median'] == float(np.median(b['nov_real_d'][rk]))
    assert r['copy_threshold'] == float(np.percentile(b['nov_real_d'][rk], 5))
    assert r['nn_top1']['pred'] == float(np.array([1.0] * 23 + [0.0] * 23).mean()) and r['nn_top1']['real'] == 1.0
    assert r['mirrored'] == float(23 / 46.0)
    assert json.loads(json.dumps(r, allow_nan=False)) == r

    # --actions: the commanded class against the class of the nearest window
    c = _arrays()
    c['actions'] = np.array([2, 0], np.int32)
    c['act_nov_code'] = np.zeros((24, 2, 2), np.int32)
    c['act_nov_code'][:, 0], c['act_nov_code'][:, 1, 0], c['act_nov_code'][:, 1, 1] = 8, 0, 4       # class 2 hit twice, class 0 hit once
    c['act_nov_d'] = np.ones((24, 2, 2))
    assert evaluate.summarise_novelty(c)['nn_top1']['commanded'] == 0.75

    empty = {k: v[:0] if k != 'nov_window_action' else v for k, v in _arrays().items()}
    r = evaluate.summarise_novelty(empty)
    assert r['pred'] == {'mean': None, 'median': None, 'p05': None} and r['ratio'] is None and r['nn_top1']['pred'] is None and r['mirrored'] is None


def test_evaluate_novelty_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval')]
    for extra, text in ((['--novelty'], '--novelty adds to the scores of --metrics and needs it'),
                        (['--novelty', '--samples', '2'], 'needs it'),
                        (['--metrics', '--novelty', '--synthetic', '2'], '--synthetic inputs have neither'),
                        (['--novelty', '--synthetic', '2'], '--synthetic inputs have neither'),
                        (['--metrics', '--novelty-sheets'], 'need it'), (['--metrics', '--novelty-no-mirror'], 'need it'),
                        (['--metrics', '--novelty', '--novelty-sheets', '--no-save'], 'writes none'),
                        (['--metrics', '--novelty', '--novelty-sheets', '--samples', '32'], 'at most 31'),
                        (['--metrics', '--sheet-frames', '3,7'], '--novelty-sheets and needs it')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_the_wrapper_and_the_entry_refuse_bad_arguments_without_a_gpu():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib, ops
    from kpx_amd._lib import KpxError, lib
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt)
    launched = _lib.abi_calls[0]
    with pytest.raises(KpxError, match='seq_nearest: .*no CPU fallback'):
        ops.seq_nearest(z(torch.float32, 64), z(torch.int64, 1), z(torch.int32, 1, 4), z(torch.int32, 64), z(torch.int32, 2), z(torch.float32, 1, 32, 1, 2))
    assert _lib.abi_calls[0] == launched
    a = 1 << 20                                                       # an aligned fake address
    call = lambda labels=a, off=a, win=a, w=35, order=a, first=a, groups=4, q=a, excl=None, nq=3, k=5, na=9, mirror=1, work=a, nbytes=1 << 20, d2=a, code=a: \
        lib.kpx_seq_nearest_f32(labels, off, win, w, order, first, groups, q, excl, nq, k, na, mirror, work, nbytes, d2, code, None)
    for bad in (dict(labels=None), dict(off=None), dict(win=None), dict(order=None), dict(first=None), dict(q=None), dict(work=None), dict(d2=None),
                dict(code=None), dict(w=0), dict(w=1 << 30), dict(groups=0), dict(groups=11), dict(nq=0), dict(nq=4097), dict(k=0), dict(k=257),
                dict(na=0), dict(na=257), dict(mirror=2), dict(nbytes=4 * 3 * 12 - 1), dict(labels=a + 4), dict(q=a + 4), dict(d2=a + 4), dict(work=a + 4),
                dict(win=a + 2), dict(excl=a + 2), dict(code=a + 1)):
        assert call(**bad) == -1, bad
    assert lib.kpx_seq_nearest_workspace_bytes(4, 3) == 4 * 3 * 12 and lib.kpx_seq_nearest_workspace_bytes(620, 1024) == 620 * 1024 * 12
    assert lib.kpx_seq_nearest_workspace_bytes(0, 3) == 0 and lib.kpx_seq_nearest_workspace_bytes(4, 4097) == 0


def test_the_restatement_knows_its_own_tie_rules():
    """novelty_ref.nearest on a hand-made store: the lowest code of equal distances, the runner-up, the exclusion and non-finite candidates."""
    k = 2
    base = np.zeros((32, k, 2), np.float32)
    frames = np.stack([base + 1, base + 1, base + 3, base + np.float32(np.inf)])              # windows 0 and 1 are equal
    frames[2, ..., 0] = 0.0                                                                   # window 2: x = 0, so it ties with its mirror
    table = np.array([[0, 0, 1, 1], [1, 0, 1, 1], [2, 0, 1, 2], [3, 0, 1, 2]], np.int32)
    q = np.stack([base + 1, base])
    d2, code, runner = N.nearest(q, frames, table, 4)
    assert code.tolist() == [[-1, 0, 4, -1], [-1, 0, 4, -1]] and d2[0, 1] == 0.0 and d2[1, 2] == 9.0 and d2[0, 2] == 5.0
    assert runner[0, 1] == 0.0 and runner[0, 2] == 5.0 and np.isinf(d2[:, [0, 3]]).all() and np.isinf(runner[:, 0]).all()
    assert not N.clear_margin(d2, runner)[:, [1, 2]].any() and N.clear_margin(d2, runner)[:, [0, 3]].all()
    d2, code, _ = N.nearest(q, frames, table, 4, mirror=False, exclude=np.array([0, 2]))
    assert code.tolist() == [[-1, 2, 4, -1], [-1, 0, -1, -1]] and np.isinf(d2[1, 2])
