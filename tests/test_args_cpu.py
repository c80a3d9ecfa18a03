"""CPU: the argument checker of the per-batch wrappers (kpx_amd/_args.py) on CPU tensors -- every branch of the pure comparison, the GPU
test of the checker proper, the output helper -- and every wrapper that goes through it: reached as ``ops.<name>``, it refuses correctly
shaped CPU tensors with KpxError before any launch.  No device is involved in any of it."""
import pytest
import torch

F32, F64, U8, I32, I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64


# ----------------------------------------------------------------------------------------------- the pure comparison
def test_mismatch_accepts_what_the_spec_describes():
    from kpx_amd._args import mismatch
    t = torch.zeros(2, 3, 4)
    assert mismatch(t, F32, (2, 3, 4)) is None
    assert mismatch(t, F32, (None, 3, None)) is None                               # a None extent matches any size
    assert mismatch(torch.zeros(0, 3, 4), F32, (None, 3, 4)) is None
    assert mismatch(t, F32, 24) is None and mismatch(t.view(-1), F32, 24) is None  # the flat form: an element count, any shape
    assert mismatch(t, F32, None) is None and mismatch(torch.zeros(()), F32, None) is None
    assert mismatch(torch.zeros(2, 1, 3).transpose(0, 1), F32, (1, 2, 3)) is None  # contiguous is what torch calls contiguous
    assert mismatch(torch.zeros(8, dtype=F64), F64, (8,), 8) is None and mismatch(torch.zeros(8), F32, (8,), 16) is None
    assert mismatch(torch.zeros(8)[4:], F32, (4,), 16) is None                     # 16 bytes into an aligned allocation


def test_mismatch_describes_every_kind_of_wrong_tensor():
    from kpx_amd._args import mismatch
    t = torch.zeros(2, 4, 6)
    wrong = {'dtype': mismatch(t.double(), F32, (2, 4, 6)),
             'bf16 for fp32': mismatch(t.bfloat16(), F32, (2, 4, 6)),
             'dimensions': mismatch(t, F32, (2, 24)),
             'dimensions, all wildcards': mismatch(t, F32, (None, None)),
             'one extent': mismatch(t, F32, (2, 4, 5)),
             'one extent beside a wildcard': mismatch(t, F32, (None, 3, 6)),
             'strided view': mismatch(t[:, ::2], F32, (2, 2, 6)),
             'transposed view': mismatch(t.transpose(1, 2), F32, (2, 6, 4)),
             'element count': mismatch(t, F32, 47),
             'strided view, flat': mismatch(t[:, ::2], F32, 24),
             'strided view, any shape': mismatch(t[:, ::2], F32, None),
             'fp32 one element past 16 bytes': mismatch(torch.zeros(9)[1:], F32, (8,), 16),
             'fp64 one element past 16 bytes': mismatch(torch.zeros(9, dtype=F64)[1:], F64, (8,), 16),
             'fp32 one element past 8 bytes': mismatch(torch.zeros(9)[1:], F32, (8,), 8),
             'uint8 one element past 8 bytes': mismatch(torch.zeros(9, dtype=U8)[1:], U8, (8,), 8),
             'a list': mismatch([1.0, 2.0], F32, (2,)),
             'a number': mismatch(3, F32, None),
             'a numpy array': mismatch(torch.zeros(2).numpy(), F32, (2,)),
             'absent': mismatch(None, F32, (2,))}
    for case, why in wrong.items():
        assert isinstance(why, str) and why.startswith('must be '), (case, why)
    # the description says what was expected and what was passed
    assert 'torch.float32' in wrong['dtype'] and 'torch.float64' in wrong['dtype'] and '[2,4,6]' in wrong['dtype']
    assert '[*,3,6]' in wrong['one extent beside a wildcard'] and '[2, 4, 6]' in wrong['one extent beside a wildcard']
    assert 'contiguous=False' in wrong['strided view'] and 'contiguous=False' in wrong['transposed view']
    assert '47 elements' in wrong['element count']
    assert '16-byte' in wrong['fp32 one element past 16 bytes'] and '4 bytes past' in wrong['fp32 one element past 16 bytes']
    assert '8-byte' in wrong['fp32 one element past 8 bytes'] and '1 bytes past' in wrong['uint8 one element past 8 bytes']
    assert 'list' in wrong['a list'] and 'NoneType' in wrong['absent']
    # the fp64 view one element in is 8 bytes in: fine for alignment 8, not for 16
    assert mismatch(torch.zeros(9, dtype=F64)[1:], F64, (8,), 8) is None


def test_mismatch_skips_an_absent_optional_tensor_only():
    from kpx_amd._args import OPTIONAL, mismatch
    assert mismatch(None, F32, (2,), 1, True) is None and mismatch(None, F32, (2,), *OPTIONAL) is None
    assert mismatch(None, F32, (2,)) is not None and mismatch(None, F32, (2,), 1, False) is not None
    assert mismatch(torch.zeros(3), F32, (2,), *OPTIONAL) is not None                # a present optional tensor is checked like any other
    assert mismatch(torch.zeros(2), F32, (2,), *OPTIONAL) is None


# ----------------------------------------------------------------------------------------------- the checker proper, the output helper
def test_check_tensors_refuses_cpu_tensors_and_names_op_and_argument():
    from kpx_amd._args import OPTIONAL, check_tensors
    from kpx_amd._lib import KpxError
    with pytest.raises(KpxError, match=r'some_op: second .*no CPU fallback'):
        check_tensors('some_op', [('first', None, F32, (2,), *OPTIONAL), ('second', torch.zeros(2), F32, (2,))])
    with pytest.raises(KpxError, match='no CPU fallback'):                           # whatever else is wrong with it
        check_tensors('some_op', [('x', torch.zeros(3, dtype=F64), F32, (2,))])
    with pytest.raises(KpxError, match=r'some_op: x must be a tensor \(got list\)'):
        check_tensors('some_op', [('x', [0.0], F32, (1,))])
    with pytest.raises(KpxError, match='some_op: x must be a tensor'):
        check_tensors('some_op', [('x', None, F32, (1,))])
    assert check_tensors('some_op', [('x', None, F32, (1,), *OPTIONAL)]) is None     # nothing present: no device to report
    assert check_tensors('some_op', [('x', None, F32, (1,), *OPTIONAL)], torch.device('cpu')) == torch.device('cpu')


def test_check_out_allocates_or_checks():
    from kpx_amd._args import check_out, mismatch
    from kpx_amd._lib import KpxError
    for dtype, shape in ((F32, (2, 3)), (F64, (4,)), (U8, (1, 2, 3, 4)), (I32, (0, 5))):
        out = check_out('some_op', 'out', None, dtype, shape, torch.device('cpu'))
        assert mismatch(out, dtype, shape) is None and out.device.type == 'cpu'
    for bad in (torch.zeros(2, 3), torch.zeros(3, 2, dtype=F64), [0.0]):
        with pytest.raises(KpxError, match='some_op: out'):
            check_out('some_op', 'out', bad, F64, (2, 3), torch.device('cpu'))


# ----------------------------------------------------------------------------------------------- every wrapper that uses the checker
def _z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def _wrapper_calls():
    """name -> a call of ops.<name> on CPU tensors of the smallest sizes the op takes: right in everything but the device."""
    from kpx_amd import ops
    health, clip = _z(I64, 4), _z(I32, 4)
    flat = lambda: _z(F32, 8)
    pts, target, mask = _z(F32, 1, 1, 2), _z(F32, 1, 1, 2), _z(U8, 1, 1)
    table = ops.SegmentTable(['v'], [8], 8, _z(I64, 1, 2), _z(I32, 1, 2))
    return {
        'point_maps_rgb': lambda: ops.point_maps_rgb(_z(F32, 1, 1, 2), 1, 1, _z(F32, 1, 3)),
        'point_seq_strip_rgb': lambda: ops.point_seq_strip_rgb(_z(F32, 1, 1, 3, 2), 1, 1, _z(F32, 3, 3)),
        'summary_image_u8': lambda: ops.summary_image_u8(_z(F32, 1, 1, 1, 1)),
        'frame_metrics': lambda: ops.frame_metrics(_z(F32, 1, 11, 11, 1), _z(F32, 1, 11, 11, 1)),
        'feature_pair_metrics': lambda: ops.feature_pair_metrics(_z(F32, 1, 1, 1, 4), _z(F32, 1, 1, 1, 4)),
        'feature_pool': lambda: ops.feature_pool(_z(F32, 1, 1, 1, 4)),
        'moments_add': lambda: ops.moments_add(_z(F64, 1, 1), _z(F64, 1), _z(F64, 1, 1)),
        'draw_moments_add': lambda: ops.draw_moments_add(_z(F32, 1), _z(I32, 1), _z(I32, 1)),
        'draw_diversity': lambda: ops.draw_diversity(_z(I32, 1), _z(I32, 1), 2, (1, 1, 1)),
        'keypoint_draw_metrics': lambda: ops.keypoint_draw_metrics(_z(F32, 2, 1, 1, 1, 2), _z(F32, 1, 1, 1, 2)),
        'sheet_paste': lambda: ops.sheet_paste(_z(U8, 1, 1, 1, 3), _z(F32, 1, 1, 1, 1, 1), [0], 0, 0, 'unit'),
        'cell_frames': lambda: ops.cell_frames(_z(U8, 1, 2, 1, 1, 3), _z(F32, 1, 1, 1, 1), _z(F32, 1, 1, 1, 1, 1), 0, 0, 'unit'),
        'color_hist_add': lambda: ops.color_hist_add(_z(U8, 1, 1, 3), _z(I32, 1, ops.HIST_CELLS, 4)),
        'palette_map': lambda: ops.palette_map(_z(U8, 1, 1, 1, 1, 3), _z(U8, 1, 256, 3), torch.ones(1, dtype=I32)),
        'gif_indices': lambda: ops.gif_indices(_z(U8, 1, 1, 1, 1, 3)),
        'points_retarget': lambda: ops.points_retarget(_z(F32, 1, 1, 2), 'hold', frames=1),
        'affine_warp': lambda: ops.affine_warp(_z(F32, 1, 1, 1, 1), _z(I32, 1), _z(F64, 1, 6)),
        'equivariance_scores': lambda: ops.equivariance_scores(_z(F32, 1, 1, 2), _z(F32, 1, 1, 2), _z(I32, 1), _z(F64, 1, 6)),
        'joint_targets': lambda: ops.joint_targets(_z(F32, 1, 1, 2), _z(U8, 1, 1), _z(F32, 1, 4), _z(F64, 4)),
        'joint_moments_add': lambda: ops.joint_moments_add(pts, target, mask, _z(F64, 1, 3, 3), _z(F64, 1, 3, 2), _z(I64, 1)),
        'joint_scores': lambda: ops.joint_scores(pts, target, mask, _z(F32, 1), _z(F64, 1, 3, 2), _z(F64, 1)),
        'class_scores': lambda: ops.class_scores(_z(F32, 1, 1), _z(I32, 1)),
        'softmax_xent': lambda: ops.softmax_xent(_z(F32, 1, 1), _z(F32, 1, 1)),
        'grad_health': lambda: ops.grad_health(flat(), health, work=_z(F64, 64)),
        'adam_tf_flat_guarded_': lambda: ops.adam_tf_flat_guarded_(flat(), flat(), flat(), flat(), _z(F32, 1), 0.5, 0.999, 1e-8, health),
        'adam_tf_flat_clipped_': lambda: ops.adam_tf_flat_clipped_(flat(), flat(), flat(), flat(), _z(F32, 1), 0.5, 0.999, 1e-8, health, clip, 1.0),
        'guard_restore_': lambda: ops.guard_restore_(flat(), flat(), health),
        'grad_segment_stats': lambda: ops.grad_segment_stats(flat(), flat(), table, work=_z(F64, 64), out=_z(I64, 1, 4)),
        'ema_flat_': lambda: ops.ema_flat_(flat(), flat(), _z(F32, 1), health),
        'swap_flat_': lambda: ops.swap_flat_(flat(), flat()),
    }


def test_the_table_names_every_wrapper_of_the_moved_module():
    import inspect
    from kpx_amd import ops, tool_ops
    moved = {n for n, v in vars(tool_ops).items() if inspect.isfunction(v) and v.__module__ == tool_ops.__name__ and not n.startswith('_')}
    assert moved == {n for n in tool_ops.__all__ if not n.isupper()}
    assert moved <= set(_wrapper_calls())
    for name in tool_ops.__all__:                                                    # the re-export: the same objects under ops
        assert getattr(ops, name) is getattr(tool_ops, name), name
    for name in ('_stream', '_ptr', 'scratch', '_workspace', '_lib', 'lib', '_require_gpu'):
        assert hasattr(ops, name), name


def test_every_wrapper_refuses_cpu_tensors_before_any_launch():
    from kpx_amd import _lib
    from kpx_amd._lib import KpxError
    calls = _wrapper_calls()
    assert len(calls) == 30
    launched = _lib.abi_calls[0]
    for name, call in calls.items():
        with pytest.raises(KpxError, match='%s: .*no CPU fallback' % name):
            call()
        assert _lib.abi_calls[0] == launched, name
