"""CPU: evaluate.py --actions without a GPU -- the two 8-bit quantisers of the sheet restatement against the bytes evaluate._save_img
writes through PIL, summarise_actions on hand-made arrays, the parser errors, and the argument checks of kpx_sheet_paste_u8_f32."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import sheet_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _edges_with_neighbours(lo, hi, to_value):
    """every bucket edge to_value(k / 255) of the 8-bit scale as float32, and its two float32 neighbours, kept inside [lo, hi]"""
    edges = to_value(np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    v = np.concatenate([edges, np.nextafter(edges, np.float32(9)), np.nextafter(edges, np.float32(-9))])
    return v[(v >= lo) & (v <= hi)]


@pytest.mark.parametrize('name,rescale,lo,hi,to_value', [('raw', False, 0.0, 1.0, lambda u: u), ('unit', True, -1.0, 1.0, lambda u: u * 2 - 1)])
def test_quantisers_are_the_bytes_save_img_writes(tmp_path, name, rescale, lo, hi, to_value):
    from PIL import Image
    import evaluate
    v = _edges_with_neighbours(lo, hi, to_value)
    assert 3 * 256 - 2 <= v.size <= 3 * 256
    pad = (-v.size) % 3
    img = np.concatenate([v, np.full(pad, lo, np.float32)])
    for shape in ((1, -1, 3), (-1, 1, 1)):                            # an RGB strip and a grey one (PIL mode 'L')
        x = img.reshape(shape)
        path = str(tmp_path / ('%s_%d.png' % (name, x.shape[2])))
        evaluate._save_img(path, x.copy(), rescale=rescale)
        back = np.asarray(Image.open(path), np.uint8).reshape(x.shape)
        assert np.array_equal(R.QUANTISERS[name](x), back)
    q = R.QUANTISERS[name](v)
    assert q.min() == 0 and q.max() == 255 and np.unique(q).size == 256       # every byte value is reached


def test_quantisers_clamp_and_send_nan_to_zero():
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 3e38, -3e38, 2.0, -2.0], np.float32)
    assert R.raw8(x).tolist() == [0, 255, 0, 0, 255, 0, 255, 0]
    assert R.unit8(x).tolist() == [0, 255, 0, 127, 255, 0, 255, 0]


def test_paste_restatement_on_a_case_worked_by_hand():
    src = np.zeros((1, 3, 1, 2, 1), np.float32)
    src[0, :, 0, :, 0] = [[0.0, 1.0], [0.5, 0.25], [1.0, 0.0]]
    canvas = np.full((1, 2, 6, 3), 0xA5, np.uint8)
    R.paste(canvas, src, [2, 1], 1, 1, 'raw')
    assert canvas[0, 0].tolist() == [[0xA5] * 3] * 6
    assert canvas[0, 1].tolist() == [[0xA5] * 3, [0xA5] * 3, [255] * 3, [0] * 3, [127] * 3, [63] * 3]


def _l2(scores, draws=2, frames=4):
    """act_kp_l2 [S, A, D, T] whose mean over (D, T) is scores[s][a], not constant over draws and frames"""
    s = np.asarray(scores, np.float64)
    wobble = np.linspace(-0.25, 0.25, draws * frames).reshape(draws, frames)
    return (s[:, :, None, None] + wobble).astype(np.float32)


def test_summarise_actions_a_model_that_ignores_the_class_scores_zero():
    import evaluate
    actions, own = [3, 7, 0], [3, 7, 0, 7]
    l2 = _l2(np.full((4, 3), 0.5))
    div = np.zeros((4, 2, 4), np.float32)
    score, rank = evaluate.action_ranks(actions, own, l2)
    assert rank.dtype == np.int32 and rank.tolist() == [2, 2, 2, 2]           # ties count against the model: rank A - 1
    blk = evaluate.summarise_actions(actions, own, l2, div, div)
    assert blk['n_ranked'] == 4 and blk['top1'] == 0.0 and blk['mean_rank'] == 2.0 and blk['chance'] == 1.0 / 3
    assert blk['confusion'] == [[1, 0, 0], [2, 0, 0], [1, 0, 0]]              # a tie goes to the lowest list position
    assert blk['kp_div']['mean'] == 0.0 and blk['div_mse']['per_frame'] == [0.0] * 4


def test_summarise_actions_own_class_strictly_lowest_everywhere():
    import evaluate
    actions, own = [3, 7, 0], [0, 3, 7, 3]
    scores = np.full((4, 3), 0.9)
    for s, o in enumerate(own):
        scores[s, actions.index(o)] = 0.1 + 0.01 * s
    l2 = _l2(scores)
    div = np.full((4, 2, 4), 0.25, np.float32)
    blk = evaluate.summarise_actions(actions, own, l2, div, 2 * div)
    assert blk['top1'] == 1.0 and blk['mean_rank'] == 0 and blk['n_ranked'] == 4
    assert blk['confusion'] == [[2, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert blk['kp_div']['mean'] == 0.25 and blk['div_mse']['mean'] == 0.5 and len(blk['kp_l2']['per_frame']) == 4
    assert abs(blk['kp_l2']['mean'] - l2.astype(np.float64).mean()) <= 1e-12
    assert blk['definition'] == evaluate.ACTIONS_DEFINITION and blk['actions'] == actions


def test_summarise_actions_unlisted_own_class_is_excluded_and_nan_ranks_last():
    import evaluate
    actions, own = [3, 7, 0], [3, 5, 0]                                        # sample 1's class 5 is not listed
    scores = np.array([[0.1, 0.5, 0.9], [0.1, 0.2, 0.3], [0.4, 0.2, 0.1]])
    l2 = _l2(scores)
    l2[2, 2, 1, 3] = np.nan                                                    # one frame of sample 2's own class: its score is +inf
    div = np.full((3, 2, 4), 0.5, np.float32)
    div[0, 0, 0] = np.inf
    score, rank = evaluate.action_ranks(actions, own, l2)
    assert rank.tolist() == [0, -1, 2] and np.isposinf(score[2, 2])
    blk = evaluate.summarise_actions(actions, own, l2, div, div)
    assert blk['n_ranked'] == 2 and blk['top1'] == 0.5 and blk['mean_rank'] == 1.0
    assert blk['confusion'] == [[1, 0, 0], [0, 0, 0], [0, 1, 0]]
    assert blk['kp_l2']['mean'] is None and blk['kp_l2']['per_frame'][3] is None and blk['kp_l2']['per_frame'][0] is not None
    assert blk['kp_div']['mean'] is None and blk['kp_div']['per_frame'][0] is None and blk['kp_div']['per_frame'][1] == 0.5
    json.dumps(blk, allow_nan=False)
    # every score non-finite: every listed class ties at +inf, rank A - 1
    _, rank = evaluate.action_ranks(actions, own, np.full_like(l2, np.nan))
    assert rank.tolist() == [2, -1, 2]


def test_summarise_actions_one_class_and_no_ranked_sample():
    import evaluate
    l2 = _l2(np.array([[0.3], [0.4]]))
    blk = evaluate.summarise_actions([5], [3, 7], l2)
    assert blk['n_ranked'] == 0 and blk['top1'] is None and blk['mean_rank'] is None and blk['chance'] == 1.0 and blk['confusion'] == [[0]]
    assert 'kp_div' not in blk and 'div_mse' not in blk and 'kp_l2' in blk
    assert json.loads(json.dumps(blk, allow_nan=False))['top1'] is None
    blk = evaluate.summarise_actions([5], [5, 7], l2)                          # A = 1 and ranked: alone, so first
    assert blk['n_ranked'] == 1 and blk['top1'] == 1.0 and blk['mean_rank'] == 0.0 and 'kp_div' not in blk
    with pytest.raises(ValueError):
        evaluate.summarise_actions([5, 3], [5, 7], _l2(np.zeros((2, 2))))      # two classes come with their diversity
    with pytest.raises(ValueError):
        evaluate.summarise_actions([5, 3], [5, 7], l2, l2[:, 0], l2[:, 0])     # act_kp_l2 of another A


def test_evaluate_actions_argument_errors_need_no_gpu(tmp_path, monkeypatch, capsys):
    import evaluate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    monkeypatch.setitem(sys.modules, 'kpx_amd', None)                 # any import of the package would now fail: the errors come first
    base = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--checkpoint_stage2', str(ck),
            '--save_dir', str(tmp_path / 'eval'), '--synthetic', '2']                   # n_action = 9
    for extra, text in ((['--actions', '9'], 'in [0, 9)'), (['--actions', '0,-1'], 'in [0, 9)'), (['--actions', '3,7,3'], 'twice'),
                        (['--actions', ''], 'nothing'), (['--actions', '1,x'], 'integers'),
                        (['--sheet-frames', '3,7'], 'needs it'),
                        (['--actions', 'all', '--sheet-frames', '32'], 'in [0, 32)'), (['--actions', 'all', '--sheet-frames', '7,3'], 'increasing'),
                        (['--actions', 'all', '--sheet-frames', '3,3'], 'twice'), (['--actions', 'all', '--sheet-frames', ''], 'nothing'),
                        (['--actions', 'all', '--samples', '456'], 'at most 4096'), (['--actions', '1', '--samples', '4097'], 'at most 4096')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2, extra
        assert text in capsys.readouterr().err, extra
    assert not (tmp_path / 'eval').exists()


def test_sheet_paste_entry_refuses_bad_arguments_without_a_gpu():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'kpx_sheet_paste_u8_f32') and 'kpx_sheet_paste_u8_f32' in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 14 and _lib.lib.kpx_abi_version() == _lib.ABI_VERSION
    a = 1 << 20                                                       # an aligned fake address: never touched
    fr = lambda *idx: (ctypes.c_int * max(1, len(idx)))(*idx)

    def paste(src=a, b=2, f=4, h=8, w=8, c=3, frames=fr(0, 1, 3), j=3, canvas=a, rows=2, cols=4, row=1, col=1, premap=0):
        return _lib.lib.kpx_sheet_paste_u8_f32(src, b, f, h, w, c, frames, j, canvas, rows, cols, row, col, premap, None)

    bad = [dict(src=None), dict(canvas=None), dict(frames=None), dict(src=a + 2),
           dict(c=2), dict(c=0), dict(c=4),
           dict(j=0), dict(frames=fr(*([0] * 65)), j=65, cols=64, col=0), dict(j=-1),
           dict(col=2), dict(col=-1), dict(cols=2), dict(row=2), dict(row=-1),                      # col + J > cols; row >= rows
           dict(frames=fr(0, 4, 1)), dict(frames=fr(0, 1, -1)),                                     # a frame index equal to F; below 0
           dict(premap=2), dict(premap=-1),
           dict(b=0), dict(f=0), dict(h=0), dict(h=1025), dict(w=0), dict(w=1025), dict(rows=0), dict(rows=65), dict(cols=65), dict(cols=0)]
    for kw in bad:
        assert paste(**kw) == -1, kw
