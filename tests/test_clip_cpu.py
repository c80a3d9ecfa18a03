"""CPU: the restatements of the clipped Adam update and the per-variable gradient statistics (tests/clip_ref.py, tests/grad_stats_ref.py)
against hand-worked cases, the chunk table of a bucket, the new entries' refusals before any device call, and train.py's handling of
--clip-norm and --grad-stats."""
import numpy as np
import pytest

import clip_ref as C
import grad_stats_ref as S
import guard_ref as G
import loss_optim_ref as L

CFG = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 2},
       'model': {'n_pts': 5, 'n_action': 4, 'cell_info': [32, 32], 'vae_dim': 8, 'classifier_cells': [32, 16]}, 'paths': {'log_dir': '/tmp/kpx_test'}}


def test_clip_scale_on_the_three_four_five_triangle():
    g = np.array([3.0, 4.0], np.float32)
    assert C.sumsq(g) == 25.0
    assert C.clip_scale(25.0, 5.0) == (5.0, 1.0, 1.0)                       # N == clip exactly: not clipped
    assert C.clip_scale(25.0, 2.5) == (5.0, 0.5, 0.5)
    assert C.clip_scale(25.0, 2.5, gscale=0.5) == (2.5, 1.0, 0.5)           # the norm is that of the averaged gradient
    assert C.clip_scale(25.0, 1.25, gscale=0.5) == (2.5, 0.5, 0.25)
    assert C.clip_scale(0.0, 1.0) == (0.0, 1.0, 1.0) and C.clip_scale(25.0, np.inf) == (5.0, 1.0, 1.0)


def test_clipped_adam_restatement_is_adam_on_the_scaled_gradient_and_counts():
    n = 1003
    p, m, v = L.adam_state(n)
    g = L.adam_grad(n, 1)
    alpha = L.adam_alpha(1)
    norm = float(np.sqrt(C.sumsq(g)))
    counters, state = G.new_counters(), C.new_state()
    out, counters, state = C.clipped_adam(p, g, m, v, alpha, 0, 2 * norm, counters, state)
    for got, want in zip(out, L.adam_step(p, g, m, v, alpha)):
        assert np.array_equal(got, want)
    assert state == dict(norm=norm, scale=1.0, clipped_total=0)
    out, counters, state = C.clipped_adam(p, g, m, v, alpha, 0, norm / 4, counters, state)
    gs = C.clip_scale(C.sumsq(g), norm / 4)[2]
    assert gs == pytest.approx(0.25, rel=1e-6) and state['scale'] == gs and state['clipped_total'] == 1
    for got, want in zip(out, L.adam_step(p, g, m, v, alpha, gscale=gs)):
        assert np.array_equal(got, want)
    kept = dict(state)
    out, counters, state = C.clipped_adam(p, g, m, v, alpha, 3, norm / 4, counters, state)      # a dirty record: skipped, the clip state stays
    assert all(np.array_equal(a, b) for a, b in zip(out, (p, m, v))) and state == kept
    assert counters == dict(skipped_total=1, skipped_run=1, updates=3)
    assert 2.0 ** -25 < C.scale_bound(n, 0.25) < 2.0 ** -25 + 1e-13       # one fp32 ulp of 0.25, and the sum's slack far below it


def test_segment_restatement_on_a_hand_worked_bucket():
    b = S.FlatBucket((2, 5, 1), shift=1)
    assert list(b.entries.values()) == [(1, (2,)), (5, (5,)), (13, (1,))] and b.size == 17
    g = np.full(b.size + 4, np.nan, np.float32)
    g[1:3], g[5:10], g[13] = (3, 4), (1, -2, np.inf, 2, np.nan), -7
    p = np.ones_like(g)
    r = S.segment_stats(b, g, p)
    assert r['sumsq_g'].tolist() == [25.0, 9.0, 49.0] and r['sumsq_p'].tolist() == [2.0, 5.0, 1.0]
    assert r['maxabs_g'].tolist() == [4.0, 2.0, 7.0] and r['nonfinite_g'].tolist() == [0, 2, 0] and r['numel'].tolist() == [2, 5, 1]
    assert S.segment_stats(b, g)['sumsq_p'].tolist() == [0.0, 0.0, 0.0]
    assert S.plant_positions(1) == [0] and S.plant_positions(S.CHUNK) == [0, S.CHUNK - 1]
    assert S.plant_positions(2 * S.CHUNK + 7) == [0, S.CHUNK - 1, S.CHUNK, 2 * S.CHUNK - 1, 2 * S.CHUNK, 2 * S.CHUNK + 6]
    assert S.synthetic_bucket(3).size < 200000


def _check_table(bucket, names, chunks, ranges):
    assert names == list(bucket.entries)
    assert [tuple(c) for c in chunks.tolist()] == S.chunk_table(bucket)
    assert chunks[:, 1].min() >= 1 and chunks[:, 1].max() <= S.CHUNK
    at = 0
    for seg, (offset, shape) in enumerate(bucket.entries.values()):
        first, count = ranges[seg]
        assert first == at and count == -(-int(np.prod(shape)) // S.CHUNK)
        mine = chunks[first:first + count]
        assert np.all(mine[:, 2] == seg) and mine[0, 0] == offset and mine[:, 1].sum() == int(np.prod(shape))
        assert np.all(mine[1:, 0] == mine[:-1, 0] + mine[:-1, 1]) and np.all(mine[:-1, 1] == S.CHUNK)     # contiguous, in order, only the last one short
        at += count
    assert at == len(chunks)


def test_chunk_table_covers_every_variable_in_order_with_the_cap():
    from kpx_amd import ops, variables
    assert ops.SEG_CHUNK == S.CHUNK
    for shift in S.SHIFTS:
        b = S.synthetic_bucket(shift)
        _check_table(b, *ops.grad_segment_chunks(b))
    real = variables.Bucket('G')
    for i, shape in enumerate(((3, 3, 64, 128), (128,), (1,), (7, 5), (2 * S.CHUNK + 1,))):
        real.add('var%d' % i, shape)
    names, chunks, ranges = ops.grad_segment_chunks(real)
    _check_table(real, names, chunks, ranges)
    assert np.all(chunks[ranges[:, 0], 0] % 4 == 0)              # Bucket.add starts every variable 16-byte aligned
    covered = np.zeros(real.size, bool)
    for start, n, _ in chunks:
        assert not covered[start:start + n].any()
        covered[start:start + n] = True
    assert covered.sum() == sum(int(np.prod(s)) for _, s in real.entries.values()) and real.size - covered.sum() == 3 + 1 + 3     # the padding behind the variables of 1, 35 and 32769 elements
    table = ops.grad_segment_table(real, 'cpu')
    assert table.names == names and table.numel == [int(np.prod(s)) for _, s in real.entries.values()] and table.size == real.size
    packed = table.chunks.numpy()
    assert np.array_equal(packed[:, 0], chunks[:, 0]) and np.array_equal(packed[:, 1] & 0xffffffff, chunks[:, 1])
    assert np.array_equal(packed[:, 1] >> 32, chunks[:, 2]) and np.array_equal(table.ranges.numpy(), ranges)
    bad = S.FlatBucket((4,))
    bad.size = 3
    with pytest.raises(Exception):
        ops.grad_segment_chunks(bad)


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                 # an aligned fake address; nothing is launched

    def adam(p=a, g=a, m=a, v=a, n=8, alpha=a, clip_norm=1.0, health=a, clip=a):
        return lib.kpx_adam_tf_flat_clipped_f32(p, g, m, v, n, alpha, 0.5, 0.999, 1e-8, 1.0, clip_norm, health, clip, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(alpha=None), dict(health=None), dict(clip=None), dict(n=0),
               dict(p=a + 4), dict(g=a + 8), dict(m=a + 4), dict(v=a + 12), dict(alpha=a + 2), dict(health=a + 4), dict(clip=a + 2),
               dict(clip_norm=0.0), dict(clip_norm=-1.0), dict(clip_norm=float('nan')), dict(clip_norm=-float('inf'))):
        assert adam(**kw) == -1, kw
    assert lib.kpx_grad_segment_stats_workspace_bytes(1) == 24 and lib.kpx_grad_segment_stats_workspace_bytes(1000) == 24000

    def stats(g=a, p=None, n=8, chunks=a, n_chunks=1, ranges=a, n_segs=1, work=a, out=a):
        return lib.kpx_grad_segment_stats_f32(g, p, n, chunks, n_chunks, ranges, n_segs, work, out, None)
    for kw in (dict(g=None), dict(chunks=None), dict(ranges=None), dict(work=None), dict(out=None), dict(n=0), dict(n_chunks=0), dict(n_segs=0),
               dict(n_chunks=1 << 31), dict(n_segs=1 << 31), dict(g=a + 2), dict(p=a + 1), dict(chunks=a + 4), dict(ranges=a + 2), dict(work=a + 4),
               dict(out=a + 4)):
        assert stats(**kw) == -1, kw


def test_new_ops_refuse_cpu_tensors():
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    f = torch.zeros(8)
    health, clip = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(KpxError):
        ops.adam_tf_flat_clipped_(f, f, f, f, torch.zeros(1), 0.5, 0.999, 1e-8, health, clip, 1.0)
    with pytest.raises(KpxError):
        ops.grad_segment_stats(f, None, ops.grad_segment_table(S.FlatBucket((8,)), 'cpu'))


def test_clip_norm_implies_guard_and_bad_values_are_refused(tmp_path, capsys):
    import train
    base = ['--mode', 'motion_generator', '--config', str(tmp_path / 'absent.yaml'), '--synthetic']
    args = train.parse_args(base)
    assert args.clip_norm is None and args.grad_stats is None and not args.guard
    assert train._clip_kw(args) == {} and train._guard_kw(args) == {}          # without the flags the constructors are called as before
    args = train.parse_args(base + ['--clip-norm', '1.5'])
    assert args.clip_norm == 1.5 and args.guard is True
    assert train._clip_kw(args) == {'clip_norm': 1.5} and train._guard_kw(args) == {'guard': True}
    assert train.parse_args(base + ['--grad-stats']).grad_stats == 5
    args = train.parse_args(base + ['--grad-stats', '2'])
    assert args.grad_stats == 2 and not args.guard and train._clip_kw(args) == {'grad_stats': True}
    for flags in (['--clip-norm', '0'], ['--clip-norm', '-1'], ['--clip-norm', 'nan'], ['--grad-stats', '0']):
        with pytest.raises(SystemExit) as e:
            train.main(base + flags)
        assert e.value.code == 2 and flags[0] in capsys.readouterr().err


def test_clip_norm_is_refused_on_a_non_training_model_and_checked_on_a_training_one():
    import kpx_amd
    with pytest.raises(ValueError, match='clip_norm'):
        kpx_amd.ActionClassifierModel(CFG, is_training=False, device='cpu', clip_norm=1.0)
    with pytest.raises(ValueError, match='clip_norm'):
        kpx_amd.MotionGeneratorModel(CFG, is_training=False, device='cpu', clip_norm=1.0)
    with pytest.raises(ValueError, match='grad_stats'):
        kpx_amd.ActionClassifierModel(CFG, is_training=False, device='cpu', grad_stats=True)
    for bad in (0, -2.0, float('nan'), '1.0', True):
        with pytest.raises(ValueError, match='clip_norm'):
            kpx_amd.ActionClassifierModel(CFG, device='cpu', clip_norm=bad)
    m = kpx_amd.ActionClassifierModel(CFG, device='cpu', clip_norm=2)
    assert m.clip_norm == 2.0 and m.guard is True and not m.grad_stats_on          # clipping reads the guard's record
    m = kpx_amd.ActionClassifierModel(CFG, device='cpu')
    assert m.clip_norm is None and m.guard is False
    with pytest.raises(ValueError):
        m.clip_report()
    with pytest.raises(ValueError):
        m.grad_stats()
