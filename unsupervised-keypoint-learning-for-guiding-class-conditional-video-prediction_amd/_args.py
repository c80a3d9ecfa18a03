"""Plumbing shared by ops.py (the train step) and tool_ops.py (the forward-only wrappers of the evaluation tools): the current HIP stream,
the per-stream scratch buffers, and the argument checker of the wrappers that run once per batch or once per step.  The per-launch wrappers
of ops.py (convolutions, batch norm, losses: ~2 400 calls a step) check by hand with ``ops._require_gpu`` and never come through here.
"""
import torch

from . import _lib
from ._lib import lib

# raw handle of torch's current HIP stream on the current device: the private accessors are ~10x cheaper than
# torch.cuda.current_stream().cuda_stream, which was 2 x 2 ms of host time per train step (one lookup per kernel launch)
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)


def _stream():
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _Scratch:
    """Per-device, per-stream scratch buffers; kernels on one stream are ordered, so consecutive ops may share them."""

    def __init__(self):
        self._bufs = {}

    def get(self, key, nbytes, device):
        k = (key, device, _stream())
        b = self._bufs.get(k)
        if b is None or b.numel() < nbytes:
            b = torch.empty(int(max(nbytes, 1 << 16)), dtype=torch.uint8, device=device)
            self._bufs[k] = b
        return b

    def reduce(self, c, device):
        return self.get('reduce', lib.kpx_chan_reduce_scratch_bytes(int(c)), device)


scratch = _Scratch()


def _workspace(key, nbytes, device):
    """The (workspace, workspace_bytes) arguments of an entry whose *_workspace_bytes query answered ``nbytes``: the scratch buffer ``key``
    of the current stream, or (None, 0) where the launch needs none."""
    return (scratch.get(key, nbytes, device).data_ptr() if nbytes else None), nbytes


OPTIONAL = (1, True)     # the options (align, optional) of a spec whose tensor may be None


def mismatch(t, dtype, shape, align=1, optional=False):
    """What keeps ``t`` from being the argument a spec asks for, or None when it is that argument: a contiguous tensor of ``dtype`` whose
    ``data_ptr()`` is a multiple of ``align`` bytes.  ``shape``: a tuple of extents, a None in it matching any; an int: any shape of that
    many elements (the flat buckets); None: any shape.  ``optional``: None may stand for the tensor.  The device is not looked at (that
    is ``check_tensors``), so this runs on CPU tensors."""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor):
        return 'must be a tensor (got %s)' % type(t).__name__
    if isinstance(shape, int):
        fits, want = t.numel() == shape, 'of %d elements ' % shape
    elif shape is None:
        fits, want = True, ''
    else:
        fits = t.dim() == len(shape) and all(s is None or s == g for s, g in zip(shape, t.shape))
        want = '[%s] ' % ','.join('*' if s is None else str(s) for s in shape)
    if t.dtype == dtype and fits and t.is_contiguous() and t.data_ptr() % align == 0:
        return None
    return ('must be a contiguous %s %stensor%s (got %s %s, contiguous=%s%s)'
            % (dtype, want, ' on a %d-byte boundary' % align if align > 1 else '', t.dtype, list(t.shape), t.is_contiguous(),
               ', %d bytes past one' % (t.data_ptr() % align) if t.data_ptr() % align else ''))


def check_tensors(what, specs, device=None):
    """Every (name, tensor, dtype, shape[, options of ``mismatch``]) of ``specs`` is that argument of the op ``what``, on a GPU, and all
    of them on ``device`` (None: the device of the first) -> that device.  Anything else is a KpxError naming the op and the argument."""
    for name, t, dtype, shape, *options in specs:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise _lib.KpxError('%s: %s is a %s tensor; kpx ops run on MI355X only, there is no CPU fallback' % (what, name, t.device))
        why = mismatch(t, dtype, shape, *options)
        if why is None and t is not None:
            device = t.device if device is None else device
            if t.device != device:
                why = 'must be on %s (got %s)' % (device, t.device)
        if why is not None:
            raise _lib.KpxError('%s: %s %s' % (what, name, why))
    return device


def check_out(what, name, out, dtype, shape, device):
    """The output tensor of the op ``what``: a new one where the caller passed none, otherwise the caller's, checked like an argument."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    check_tensors(what, ((name, out, dtype, shape),), device)
    return out
