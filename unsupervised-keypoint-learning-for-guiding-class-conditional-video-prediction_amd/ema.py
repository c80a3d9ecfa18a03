"""The averaged generator (train.py --ema): the schedule of the average, and reading a checkpoint under its averages (numpy only).

A model built with ``ema=DECAY`` keeps, beside every variable of its 'G' bucket, an exponential moving average
``shadow += (variable - shadow) * rate`` (tf.train.ExponentialMovingAverage; the update itself is the HIP kernel kpx_ema_flat_f32).
Its checkpoints carry each average as ``<variable name>/ExponentialMovingAverage``, TF's shadow naming, beside the variable.

    python -m kpx_amd.ema IN OUT [--ckpt-format npz|tf]

writes an inference checkpoint in which the averages stand under the variable names (Adam slots and shadow keys dropped), in either
container: what the reference's own restore, or any tool that knows nothing of averages, reads as an averaged model.
"""
import numpy as np

SUFFIX = '/ExponentialMovingAverage'
_SLOTS = ('/Adam', '/Adam_1')


def rate(decay, t, warmup=True):
    """The step of the average at update index ``t`` (global_step before its increment) as a numpy float32, op for op in float32:
    1 - min(decay, (1 + t) / (10 + t)), tf.train.ExponentialMovingAverage(decay, num_updates=t); ``warmup=False`` drops the min."""
    d = np.float32(decay)
    if warmup:
        t32 = np.float32(t)
        d = min(d, np.float32((np.float32(1) + t32) / (np.float32(10) + t32)))
    return np.float32(np.float32(1) - d)


def has_shadows(arrays):
    return any(k.endswith(SUFFIX) for k in arrays)


def select(arrays, strict=True):
    """{name: array} of a checkpoint read under its averages: every ``<name>/ExponentialMovingAverage`` moved onto ``<name>``; variables
    without a shadow (the discriminator, batch-norm moving statistics, counters) pass through; Adam slots and the shadow keys are dropped.
    ``strict``: a checkpoint none of whose keys carries the suffix is an error (otherwise it comes back without its slots)."""
    if strict and not has_shadows(arrays):
        raise KeyError('the checkpoint holds no averaged weights (no key ends in %s among its %d): it was written by a run without '
                       'train.py --ema' % (SUFFIX, len(arrays)))
    out = {}
    for k, v in arrays.items():
        if not k.endswith(SUFFIX) and not k.endswith(_SLOTS):
            out[k] = v
    for k, v in arrays.items():
        if k.endswith(SUFFIX):
            out[k[:-len(SUFFIX)]] = v
    return out


def read_selected(checkpoint_path):
    """read_checkpoint + select; the error of a checkpoint without averages names it."""
    from .base_model import BaseModel
    try:
        return select(BaseModel.read_checkpoint(checkpoint_path))
    except KeyError as e:
        raise Exception('--ema: %s: %s' % (checkpoint_path, e.args[0]))


def main(argv=None):
    from argparse import ArgumentParser
    import os
    from . import tf_bundle
    from .base_model import BaseModel, TMP_SUFFIX
    parser = ArgumentParser(prog='python -m kpx_amd.ema', description='write an inference checkpoint whose variables are the averages of IN')
    parser.add_argument('input', metavar='IN', help='a training checkpoint written under train.py --ema (an .npz or a bundle prefix)')
    parser.add_argument('output', metavar='OUT', help="the file to write ('npz': the name as given; 'tf': the prefix of the bundle)")
    parser.add_argument('--ckpt-format', choices=['npz', 'tf'], default='npz')
    args = parser.parse_args(argv)
    if not (os.path.isfile(args.input) or tf_bundle.is_bundle(args.input)):
        parser.error('%s: no such checkpoint (an .npz file or the prefix of a bundle)' % args.input)
    raw = BaseModel.read_checkpoint(args.input)
    try:
        arrays = select(raw)
    except KeyError as e:
        parser.error('%s: %s' % (args.input, e.args[0]))
    if args.ckpt_format == 'tf':
        tf_bundle.write_bundle(args.output, arrays)
    else:
        tmp = args.output + TMP_SUFFIX
        with open(tmp, 'wb') as f:
            np.savez(f, **{k.replace('/', '|'): v for k, v in arrays.items()})
        os.replace(tmp, args.output)
    print('%s: %d variables, %d of them averages' % (args.output, len(arrays), sum(1 for k in raw if k.endswith(SUFFIX))))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
