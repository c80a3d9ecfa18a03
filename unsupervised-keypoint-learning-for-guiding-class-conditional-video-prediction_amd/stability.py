"""Host side of the detector's equivariance score (make_pseudo_labels.py --stability; not in the reference).

Move a frame by a known similarity map, detect again, and the detected points should have moved by the same map.  ``draw_warps`` draws the
maps, ``KeypointModel.stability`` warps, detects and scores on the device (csrc/stability.hip), ``video_record`` and ``summarise_stability``
reduce the scores on the host.  Everything here is numpy float64 and runs the same with or without a GPU.

Conventions: a map is six numbers (m0 .. m5), q = (m0 x + m1 y + m2, m3 x + m4 y + m5).  ``fwd`` maps a point of the original frame to its
place in the warped frame, in the key points' normalised coordinates ([-1, 1], pixel i at -1 + 2 i / (res - 1), as ``get_coord``); ``coef_px``
is its inverse in pixel units, which is what a resampler needs (where does output pixel (x, y) come from).  Frames are square.
"""
import math

import numpy as np

# The default draw: a rotation within 15 degrees, a scale within a factor 1.2 either way and a shift within 0.1 (a twentieth of the frame's
# side), two maps per frame.  A judgement, not a measurement: the range of the training augmentation (the sequence loader turns by up to 15
# degrees and scales by 0.7 .. 1.2), small enough that most points stay inside the frame.  No flip is drawn: left and right points of a
# symmetric body swap under a flip, and a detector that follows the body would be scored as wrong.
DEFAULT_ROT_DEG, DEFAULT_LOG_SCALE, DEFAULT_SHIFT, DEFAULT_WARPS = 15.0, math.log(1.2), 0.1, 2

NOTE = ("equivariance error of the key-point detector under random similarity maps: this project's own quantity, not a published "
        "benchmark figure and not comparable with one; it says whether the points follow the image, not whether they mean anything")


def invert_maps(m):
    """The inverse of each affine map of m [..., 6], in float64."""
    m = np.asarray(m, np.float64)
    det = m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]
    i0, i1, i3, i4 = m[..., 4] / det, -m[..., 1] / det, -m[..., 3] / det, m[..., 0] / det
    return np.stack([i0, i1, -(i0 * m[..., 2] + i1 * m[..., 5]), i3, i4, -(i3 * m[..., 2] + i4 * m[..., 5])], axis=-1)


def to_pixel_units(m, res):
    """A map between normalised coordinates, m [..., 6], as the same map between pixel coordinates of a res x res frame: with h = (res - 1) / 2
    pixel i sits at i / h - 1, so x' = h (m0 (x / h - 1) + m1 (y / h - 1) + m2 + 1) = m0 x + m1 y + h (m2 + 1 - m0 - m1)."""
    m = np.asarray(m, np.float64)
    if int(res) != res or res < 2:
        raise ValueError('to_pixel_units: res must be an integer >= 2 (got %r)' % (res,))
    h = (np.float64(res) - 1.0) / 2.0
    return np.stack([m[..., 0], m[..., 1], h * (m[..., 2] + 1.0 - m[..., 0] - m[..., 1]),
                     m[..., 3], m[..., 4], h * (m[..., 5] + 1.0 - m[..., 3] - m[..., 4])], axis=-1)


def draw_warps(n_frames, n_warps=DEFAULT_WARPS, seed=0, rot_deg=DEFAULT_ROT_DEG, log_scale=DEFAULT_LOG_SCALE, shift=DEFAULT_SHIFT, res=128):
    """n_warps similarity maps about the frame centre for each of n_frames frames, from ``np.random.RandomState(seed)`` (an integer or a
    sequence of integers): an angle in +-rot_deg degrees, a scale exp(U(+-log_scale)) and a translation in +-shift (normalised units) per
    axis, all uniform.  -> (coef_px [n_frames, n_warps, 6], fwd [n_frames, n_warps, 6]), float64: the inverse in pixel units of a res x res
    frame (``ops.affine_warp``'s coef) and the forward map in normalised units (``ops.equivariance_scores``'s fwd)."""
    if n_frames < 0 or n_warps < 1:
        raise ValueError('draw_warps: needs n_frames >= 0 and n_warps >= 1 (got %r, %r)' % (n_frames, n_warps))
    u = np.random.RandomState(seed).uniform(-1.0, 1.0, size=(int(n_frames), int(n_warps), 4))
    theta, s = np.deg2rad(np.float64(rot_deg)) * u[..., 0], np.exp(np.float64(log_scale) * u[..., 1])
    a, b = s * np.cos(theta), s * np.sin(theta)
    fwd = np.stack([a, -b, np.float64(shift) * u[..., 2], b, a, np.float64(shift) * u[..., 3]], axis=-1)
    return to_pixel_units(invert_maps(fwd), res), fwd


def video_record(subset, idx, scores, valid, frame_mean, n_valid):
    """What ``summarise_stability`` keeps of one video: the per-frame arrays as they come from ``KeypointModel.stability`` (frame_mean
    [F,W,2] float32, n_valid [F,W] int32) and, from scores [F,W,K,2] and valid [F,W,K], the per-point sums over the valid entries in
    float64 (point_sum [K,2], point_count [K])."""
    scores, valid = np.asarray(scores, np.float64), np.asarray(valid).astype(bool)
    k = scores.shape[2]
    masked = np.where(valid[..., None], scores, 0.0).reshape(-1, k, 2)
    return {'subset': str(subset), 'idx': int(idx), 'frame_mean': np.asarray(frame_mean, np.float32), 'n_valid': np.asarray(n_valid, np.int64),
            'point_sum': masked.sum(axis=0), 'point_count': valid.reshape(-1, k).sum(axis=0).astype(np.int64), 'n_total': int(valid.size)}


def _frame_sums(rec):
    """(sum of err, sum of moved, number) over the valid (frame, warp, point) entries of a record: per frame the mean times its count;
    frames without a valid point (mean NaN, count 0) add nothing."""
    n = rec['n_valid'].astype(np.float64)
    mean = np.where(rec['n_valid'][..., None] > 0, rec['frame_mean'].astype(np.float64), 0.0)
    return float((mean[..., 0] * n).sum()), float((mean[..., 1] * n).sum()), int(rec['n_valid'].sum())


def _div(a, b):
    return float(a) / float(b) if b else float('nan')


def _summary(records, res):
    sums = [_frame_sums(r) for r in records]
    err, moved, n = sum(s[0] for s in sums), sum(s[1] for s in sums), sum(s[2] for s in sums)
    total = sum(r['n_total'] for r in records)
    out = {'videos': len(records), 'frame_warps': int(sum(r['n_valid'].size for r in records)), 'entries': total, 'valid_entries': n,
           'equiv': _div(err, n), 'moved': _div(moved, n), 'valid_fraction': _div(n, total)}
    out['equiv_px'] = out['equiv'] * (res - 1) / 2.0
    out['ratio'] = _div(out['equiv'], out['moved']) if n else float('nan')
    if records:
        psum, pcount = sum(r['point_sum'] for r in records), sum(r['point_count'] for r in records)
        with np.errstate(invalid='ignore', divide='ignore'):
            pp = psum / pcount[:, None].astype(np.float64)
        out['per_point'] = {'equiv': pp[:, 0].tolist(), 'moved': pp[:, 1].tolist(), 'count': pcount.tolist()}
    else:
        out['per_point'] = {'equiv': [], 'moved': [], 'count': []}
    return out


def summarise_stability(records, res, draw):
    """records: the ``video_record`` of every video, in the order they were scored; res: the frames' side; draw: the parameters of the draw
    ({'warps', 'seed', 'rot_deg', 'log_scale', 'shift'}), copied into the result.  -> {'note', 'res', 'draw', 'overall', 'subsets': {name:
    ...}} with, overall and per subset: ``equiv`` the mean err over the valid (frame, warp, point) entries in normalised units and
    ``equiv_px`` the same times (res - 1) / 2; ``moved`` the mean distance the maps moved those points; ``ratio`` = equiv / moved (0: the
    points follow the map; 1: the detector ignores the image, its points stay where they were); ``per_point`` both means per key point;
    ``valid_fraction`` the share of entries whose target stayed inside the frame; and the counts.  NaN where nothing is valid."""
    subsets = []
    for r in records:
        if r['subset'] not in subsets:
            subsets.append(r['subset'])
    return {'note': NOTE, 'res': int(res), 'draw': dict(draw), 'overall': _summary(list(records), res),
            'subsets': {name: _summary([r for r in records if r['subset'] == name], res) for name in subsets}}


def jsonable(x):
    """The summary as standard JSON: a value that is not finite (a mean over nothing) becomes null."""
    if isinstance(x, dict):
        return {k: jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [jsonable(v) for v in x]
    if isinstance(x, float) and not math.isfinite(x):
        return None
    return x


def per_video_arrays(records):
    """The per-video arrays of stability.npz: subset, idx, err and moved (the means over the video's valid entries, NaN without any),
    n_valid and n_total."""
    sums = [_frame_sums(r) for r in records]
    return {'subset': np.array([r['subset'] for r in records], dtype='U16'), 'idx': np.array([r['idx'] for r in records], np.int64),
            'err': np.array([_div(s[0], s[2]) for s in sums], np.float64), 'moved': np.array([_div(s[1], s[2]) for s in sums], np.float64),
            'n_valid': np.array([s[2] for s in sums], np.int64), 'n_total': np.array([r['n_total'] for r in records], np.int64)}
