"""Key-point sequences resampled in time, and how fast they move (csrc/resample.hip, include/kpx.h): FinalModel.run(frames=, rate=),
animate.py and evaluate.py --frames / --rate / --resample.

A rollout is 32 key-point frames at the training frame gap.  ``points_resample`` puts F - 1 frames between every two of them (and between the
detected frame 0 and the first), linearly or on a Catmull-Rom cubic; the translator renders a frame for any pose, so nothing is learned for the
frames in between.  ``points_speed`` is the mean distance the points move per frame: the number in which the seam of a chained rollout shows
(``seam_ratio``).  Definitions, to the bit, in include/kpx.h and DESIGN.md section 2; nothing is clamped.
"""
import numpy as np

# mirrors of include/kpx.h (tests/test_resample_cpu.py holds them equal to the header)
RESAMPLE_MODES = {'linear': 0, 'cubic': 1}                       # = KPX_RESAMPLE_*
RESAMPLE_MAX_POINTS, RESAMPLE_MAX_RATE = 1024, 64
SEGMENT = 32                                                     # frames of one motion-generator call: a chained rollout is whole segments


def _error(msg):
    from ._lib import KpxError
    return KpxError(msg)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_rollout_args(what, frames=SEGMENT, rate=1, resample='cubic'):
    """The (frames, rate, resample) of a rollout, as FinalModel.run and the tools take them -> (segments, frames * rate).  ``KpxError`` naming
    the argument for anything else.  Host only."""
    if not _is_int(frames) or frames < SEGMENT or frames % SEGMENT:
        raise _error('%s: frames must be a positive multiple of %d (got %r)' % (what, SEGMENT, frames))
    if not _is_int(rate) or not 1 <= rate <= RESAMPLE_MAX_RATE:
        raise _error('%s: rate must be an integer in [1, %d] (got %r)' % (what, RESAMPLE_MAX_RATE, rate))
    if resample not in RESAMPLE_MODES:
        raise _error('%s: resample must be one of %s (got %r)' % (what, sorted(RESAMPLE_MODES), resample))
    return int(frames) // SEGMENT, int(frames) * int(rate)


def _sizes(what, first, seq, name='seq'):
    """(B, N, K) of a knot pair by its shapes alone, before anything looks at a device: the limits are refused on any tensor"""
    import torch
    for n_, t, d in (('first', first, 3), (name, seq, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != d or t.shape[-1] != 2:
            raise _error('%s: %s must be an fp32 tensor [%s,2] (got %s)' % (what, n_, 'B,K' if d == 3 else 'B,N,K',
                                                                            list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    b, n, k, _ = seq.shape
    if b < 1 or n < 1 or not 1 <= k <= RESAMPLE_MAX_POINTS:
        raise _error('%s: %s needs B, N >= 1 and 1 <= K <= %d (got B = %d, N = %d, K = %d)' % (what, name, RESAMPLE_MAX_POINTS, b, n, k))
    return b, n, k


def points_resample(first, seq, rate, mode='cubic', out=None):
    """kpx_points_resample_f32.  first fp32 [B,K,2]: the knot at time 0; seq fp32 [B,N,K,2]: the knots at the times 1..N -> fp32 [B,N*rate,K,2],
    frame j = 1..N*rate at the time j / rate, stored at index j - 1.  Every rate-th frame is a knot, bit for bit (rate = 1: a copy of seq);
    the others in fp64 from the two ('linear') or up to four ('cubic': Catmull-Rom, one-sided tangents at both ends) knots around them, rounded
    to fp32 once.  Nothing is clamped: a cubic may overshoot [-1, 1] slightly.  1 <= K <= 1024, 1 <= rate <= 64, N >= 2 for 'cubic',
    B*N*rate*K*2 < 2^31.  One launch on the current stream, capturable."""
    import torch
    from ._args import _stream, check_out, check_tensors
    from ._lib import lib, check
    if mode not in RESAMPLE_MODES:
        raise _error('points_resample: mode must be one of %s (got %r)' % (sorted(RESAMPLE_MODES), mode))
    if not _is_int(rate) or not 1 <= rate <= RESAMPLE_MAX_RATE:
        raise _error('points_resample: rate must be an integer in [1, %d] (got %r)' % (RESAMPLE_MAX_RATE, rate))
    b, n, k = _sizes('points_resample', first, seq)
    if mode == 'cubic' and n < 2:
        raise _error("points_resample: seq needs N >= 2 knots after the first for mode 'cubic' (got N = %d); 'linear' takes N = 1" % n)
    if b * n * int(rate) * k * 2 >= 2 ** 31:
        raise _error('points_resample: out would hold B*N*rate*K*2 = %d values, the launch takes fewer than 2^31 (seq %s, rate %d)'
                     % (b * n * int(rate) * k * 2, list(seq.shape), rate))
    f32 = torch.float32
    dev = check_tensors('points_resample', [('first', first, f32, (b, k, 2), 4), ('seq', seq, f32, (b, n, k, 2), 4)])
    out = check_out('points_resample', 'out', out, f32, (b, n * int(rate), k, 2), dev)
    check(lib.kpx_points_resample_f32(first.data_ptr(), seq.data_ptr(), b, n, k, int(rate), RESAMPLE_MODES[mode], out.data_ptr(), _stream()),
          'kpx_points_resample_f32')
    return out


def points_speed(first, seq, scale=1.0):
    """kpx_points_speed_f64.  first fp32 [B,K,2], seq fp32 [B,T,K,2] -> fp64 [B,T]: scale times the mean over the K points of the distance
    between frame t and frame t - 1 (frame 0 = first), in fp64, the points added in ascending order.  ``scale``: the rate of a resampled
    sequence, so that the unit stays "per source frame".  1 <= K <= 1024, B*T*K*2 < 2^31.  One launch on the current stream, capturable."""
    import torch
    from ._args import _stream, check_tensors
    from ._lib import lib, check
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale):
        raise _error('points_speed: scale must be a finite number (got %r)' % (scale,))
    b, t, k = _sizes('points_speed', first, seq)
    if b * t * k * 2 >= 2 ** 31:
        raise _error('points_speed: seq holds B*T*K*2 = %d values, the launch takes fewer than 2^31' % (b * t * k * 2))
    dev = check_tensors('points_speed', [('first', first, torch.float32, (b, k, 2), 4), ('seq', seq, torch.float32, (b, t, k, 2), 4)])
    speed = torch.empty((b, t), dtype=torch.float64, device=dev)
    check(lib.kpx_points_speed_f64(first.data_ptr(), seq.data_ptr(), b, t, k, float(scale), speed.data_ptr(), _stream()), 'kpx_points_speed_f64')
    return speed


def seam_ratio(speed, frames, rate):
    """speed: the mean speed curve [frames * rate] of a chained rollout of ``frames`` = 32 S source frames -> mean speed at the first frame of
    the segments 1..S-1 over the mean speed at all other frames; None for S = 1 or where the quotient is not a finite number.  numpy only."""
    speed = np.asarray(speed, np.float64).reshape(-1)
    s = frames // SEGMENT
    if s < 2:
        return None
    seam = np.zeros(speed.shape[0], bool)
    seam[[SEGMENT * rate * i for i in range(1, s)]] = True           # index of output frame 32 i rate + 1: the first that leaves knot 32 i
    with np.errstate(all='ignore'):
        ratio = float(speed[seam].mean() / speed[~seam].mean())
    return ratio if np.isfinite(ratio) else None
