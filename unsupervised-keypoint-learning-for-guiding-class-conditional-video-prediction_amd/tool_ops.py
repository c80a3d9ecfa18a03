"""Forward-only wrappers around the C ABI (include/kpx.h) for the tools around training: evaluate.py, animate.py, make_pseudo_labels.py
and the summaries.  None of them runs inside a train step; each is called once per batch, so its tensors go through the spec checker of
``_args`` (one list of (name, tensor, dtype, shape) per op) and only what is specific to the op -- value ranges, mode rules, table
read-backs -- is written out.  ``ops`` re-exports every name here: ``ops.sheet_paste``, ``ops.MAX_DRAWS`` ... are the public names.  ``seq_nearest`` (evaluate.py --novelty)
is written beside its tables in ``novelty`` and reaches ``tool_ops`` and ``ops`` by the import at the end of each; so do ``points_resample``
and ``points_speed`` of ``resample``, ``set_neighbours`` and ``prdc`` of ``prdc`` (evaluate.py --prdc) and ``jpeg_scans`` and ``jpeg_encode`` of
``mjpeg`` (evaluate.py --video) and ``latent_stats_add``, ``latent_sample`` and ``latent_path`` of ``posterior`` (evaluate.py --posterior).
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from ._args import OPTIONAL, _ptr, _stream, check_out, check_tensors, scratch

__all__ = ['point_maps_rgb', 'point_seq_strip_rgb', 'summary_image_u8', 'frame_metrics', 'feature_pair_metrics', 'feature_pool', 'moments_add',
           'draw_moments_add', 'draw_diversity', 'keypoint_draw_metrics', 'sheet_paste', 'cell_frames', 'color_hist_add', 'palette_map',
           'gif_indices', 'points_retarget', 'affine_warp', 'equivariance_scores', 'joint_targets', 'joint_moments_add', 'joint_scores',
           'class_scores', 'SUMMARY_PREMAPS', 'SUMMARY_SLICES', 'MAX_MOMENT_ROWS', 'MAX_MOMENT_DIM', 'MAX_DRAWS', 'SHEET_PREMAPS',
           'SHEET_MAX_FRAMES', 'CELL_MAX_POINTS', 'CELL_MAX_RADIUS', 'HIST_CELLS', 'HIST_MAX_PIXELS', 'GIF_MAX_DITHER', 'RETARGET_MODES',
           'RETARGET_MAX_POINTS', 'WARP_MAX_ROWS', 'EQUIV_MAX_ROWS', 'EQUIV_MAX_POINTS', 'JOINT_MAX_POINTS', 'JOINT_MAX_JOINTS',
           'JOINT_MAX_FRAMES', 'JOINT_MAX_ALPHAS', 'MAX_CLASS_ROWS', 'MAX_CLASSES']

F32, F64, U8, I32, I64 = torch.float32, torch.float64, torch.uint8, torch.int32, torch.int64
ANY = None               # an extent of a spec's shape that matches any size


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


# ----------------------------------------------------------------------------------------------- key-point pictures, summaries
def point_maps_rgb(mu, h, w, colors, inv_std=14.3, out=None):
    """colorize_point_maps(get_gaussian_maps(mu, [h, w], inv_std), colors) (reference utils/model.py:42-60) in one launch, forward only:
    mu [N,K,2] (x,y), colors [K,3] fp32 on mu's device -> [N,h,w,3].  The Gaussian factor has the bits of ``gaussian_maps``."""
    mu, colors = mu.contiguous(), colors.contiguous()
    dev = check_tensors('point_maps_rgb', [('mu', mu, F32, (ANY, ANY, 2))])
    n, k, _ = mu.shape
    check_tensors('point_maps_rgb', [('colors', colors, F32, (k, 3))], dev)
    out = check_out('point_maps_rgb', 'out', out, F32, (n, h, w, 3), dev)
    check(lib.kpx_point_maps_rgb_f32(mu.data_ptr(), n, k, int(h), int(w), float(inv_std), colors.data_ptr(), out.data_ptr(), _stream()),
          'kpx_point_maps_rgb_f32')
    return out


def point_seq_strip_rgb(mu, h, w, colors, recolour=True, inv_std=14.3, max_outputs=None):
    """The reference's pose-sequence strip (motion_generator_model.py:225-248, 258-263) in one launch, forward only: mu [N,T,K,2] (x,y)
    -> [N,h,T*w,3], frame t (= ``point_maps_rgb`` of mu[:, t], same bits) in columns [t*w, (t+1)*w).  ``recolour``: the summary's second
    colorize_point_maps over the 3-channel strip, out[...,c] = max_{i<3} strip[...,i] * colors[i][c] (K >= 3).  ``max_outputs``: render
    only the first images."""
    if max_outputs is not None:
        mu = mu[:max_outputs]
    mu, colors = mu.contiguous(), colors.contiguous()
    dev = check_tensors('point_seq_strip_rgb', [('mu', mu, F32, (ANY, ANY, ANY, 2))])
    n, t, k, _ = mu.shape
    check_tensors('point_seq_strip_rgb', [('colors', colors, F32, (k, 3))], dev)
    if recolour and k < 3:
        raise _lib.KpxError('point_seq_strip_rgb: the recolour reads colors[0:3] and needs K >= 3 (got K = %d)' % k)
    out = torch.empty((n, h, t * w, 3), dtype=F32, device=dev)
    check(lib.kpx_point_seq_strip_rgb_f32(mu.data_ptr(), n, t, k, int(h), int(w), float(inv_std), colors.data_ptr(), 1 if recolour else 0,
                                          out.data_ptr(), _stream()), 'kpx_point_seq_strip_rgb_f32')
    return out


SUMMARY_PREMAPS = {'identity': 0, 'x255': 1, 'unit255': 2, 'unit255_clip': 3}   # = KPX_PREMAP_* of include/kpx.h
SUMMARY_SLICES = 64                                                               # = KPX_SUMMARY_SLICES


def summary_image_u8(x, premap='identity', max_outputs=2):
    """tf.summary.image's float -> uint8 conversion (TF 1.12 SummaryImageOp / NormalizeFloatImage) of the first ``max_outputs`` images of
    x [N,H,W,C] fp32 (C in 1, 3, 4), after the pre-map ``premap``: 'identity' x, 'x255' x*255 (the mask), 'unit255' (x+1)/2*255 (the
    input frames), 'unit255_clip' clip((x+1)/2*255, 0, 255) (the predictions).  -> uint8 [min(N, max_outputs),H,W,C] on x's device."""
    if premap not in SUMMARY_PREMAPS:
        raise _lib.KpxError('summary_image_u8: premap must be one of %s (got %r)' % (sorted(SUMMARY_PREMAPS), premap))
    if int(max_outputs) < 1:
        raise _lib.KpxError('summary_image_u8: max_outputs must be >= 1 (got %r)' % (max_outputs,))
    if isinstance(x, torch.Tensor) and x.dim() == 4:
        x = x[:int(max_outputs)].contiguous()
    dev = check_tensors('summary_image_u8', [('x', x, F32, (ANY,) * 4)])
    n, h, w, c = x.shape
    if c not in (1, 3, 4) or min(n, h, w) < 1:
        raise _lib.KpxError('summary_image_u8: x must be non-empty with C in (1, 3, 4) (got %s)' % (tuple(x.shape),))
    work = torch.empty(2 * SUMMARY_SLICES * n, dtype=F32, device=dev)
    out = torch.empty((n, h, w, c), dtype=U8, device=dev)
    check(lib.kpx_summary_image_u8_f32(x.data_ptr(), n, h, w, c, SUMMARY_PREMAPS[premap], work.data_ptr(), out.data_ptr(), _stream()),
          'kpx_summary_image_u8_f32')
    return out


# ----------------------------------------------------------------------------------------------- frame and feature metrics
def frame_metrics(a, b, max_val=1.0, png8=False, out=None):
    """Per-frame SSIM, MSE and PSNR (TF 1.12 tf.image.ssim / tf.image.psnr) of a against b, both contiguous fp32
    [N,H,W,C] on one device, C in (1, 3), H and W in [11, 1024], dynamic range ``max_val`` > 0 -> fp32 [N,3] = (ssim, mse, psnr) on that
    device, in one launch.  ``png8``: score the 8-bit frames evaluate.py writes (each value quantised as ``_save_img(rescale=True)``,
    scored as q / 255 with max_val 1).  ``out``: a contiguous fp32 [N,3] tensor to write into."""
    dev = check_tensors('frame_metrics', [('a', a, F32, (ANY,) * 4)])
    check_tensors('frame_metrics', [('b', b, F32, tuple(a.shape))], dev)
    n, h, w, c = a.shape
    if n < 1 or not (11 <= h <= 1024 and 11 <= w <= 1024) or c not in (1, 3):
        raise _lib.KpxError('frame_metrics: needs N >= 1, H and W in [11, 1024] and C in (1, 3) (got %s)' % (tuple(a.shape),))
    L = float(max_val)
    if not (0.0 < L < float('inf')):
        raise _lib.KpxError('frame_metrics: max_val must be a finite value > 0 (got %r)' % (max_val,))
    out = check_out('frame_metrics', 'out', out, F32, (n, 3), dev)
    check(lib.kpx_frame_metrics_f32(a.data_ptr(), b.data_ptr(), n, h, w, c, L, 1 if png8 else 0, out.data_ptr(), _stream()),
          'kpx_frame_metrics_f32')
    return out


def _feature_sizes(what, shape):
    n, h, w, c = shape
    if n < 1 or not (1 <= h <= 1024 and 1 <= w <= 1024) or c % 4 or not 4 <= c <= 512:
        raise _lib.KpxError('%s: needs N >= 1, H and W in [1, 1024] and C a multiple of 4 in [4, 512] (got %s)' % (what, tuple(shape)))
    return n, h, w, c


def feature_pair_metrics(fa, fb, out=None):
    """Per-frame VGG feature-space metrics of one layer's features fa against fb, both contiguous fp32 [N,H,W,C] on
    one device at 16-byte aligned addresses, C a multiple of 4 in [4, 512], H and W in [1, 1024] -> fp32 [N,2] = (cos_layer, l1_layer): the
    mean over positions of the channel cosine (1 where both sides are zero, 0 where one is) and the mean of |a - b|.  ``out``: a contiguous
    fp32 [N,2] tensor to write into.  Two launches on the current stream; frame n's result is bitwise independent of the batch."""
    dev = check_tensors('feature_pair_metrics', [('fa', fa, F32, (ANY,) * 4, 16)])
    check_tensors('feature_pair_metrics', [('fb', fb, F32, tuple(fa.shape), 16)], dev)
    n, h, w, c = _feature_sizes('feature_pair_metrics', fa.shape)
    out = check_out('feature_pair_metrics', 'out', out, F32, (n, 2), dev)
    work = scratch.get('feature_pair', lib.kpx_feature_pair_metrics_workspace_bytes(n, h, w, c), dev)
    check(lib.kpx_feature_pair_metrics_f32(fa.data_ptr(), fb.data_ptr(), n, h, w, c, work.data_ptr(), out.data_ptr(), _stream()),
          'kpx_feature_pair_metrics_f32')
    return out


def feature_pool(f, out=None):
    """The mean over the H * W positions of one layer's features (the Fréchet distance): f contiguous fp32 [N,H,W,C]
    at a 16-byte aligned address, C a multiple of 4 in [4, 512], H and W in [1, 1024] -> fp64 [N,C], every value converted to fp64 before
    its first addition.  ``out``: a contiguous fp64 [N,C] tensor to write into.  Two launches on the current stream; frame n's row is
    bitwise independent of the batch."""
    dev = check_tensors('feature_pool', [('f', f, F32, (ANY,) * 4, 16)])
    n, h, w, c = _feature_sizes('feature_pool', f.shape)
    out = check_out('feature_pool', 'out', out, F64, (n, c), dev)
    work = scratch.get('feature_pool', lib.kpx_feature_pool_workspace_bytes(n, h, w, c), dev)
    check(lib.kpx_feature_pool_f64(f.data_ptr(), n, h, w, c, work.data_ptr(), out.data_ptr(), _stream()), 'kpx_feature_pool_f64')
    return out


MAX_MOMENT_ROWS, MAX_MOMENT_DIM = 1 << 20, 1024                                   # kpx_moments_add_f64's limits on M and D


def moments_add(x, sum, outer):
    """Rows into the moment accumulators of the Fréchet distance: x contiguous fp64 [M,D], 1 <= M <= 2^20,
    1 <= D <= 1024; sum [D] += the column sums, outer [D,D] += x^T x, both contiguous fp64 on x's device, zeroed by the caller before the
    first call.  One launch on the current stream; each element adds the rows in ascending order, so the result is bitwise reproducible
    and ``outer`` stays bitwise symmetric.  -> (sum, outer)."""
    dev = check_tensors('moments_add', [('x', x, F64, (ANY, ANY), 8)])
    m, d = x.shape
    if not 1 <= m <= MAX_MOMENT_ROWS or not 1 <= d <= MAX_MOMENT_DIM:
        raise _lib.KpxError('moments_add: x must be [M,D] with 1 <= M <= %d and 1 <= D <= %d (got %s)'
                            % (MAX_MOMENT_ROWS, MAX_MOMENT_DIM, tuple(x.shape)))
    check_tensors('moments_add', [('sum', sum, F64, (d,), 8), ('outer', outer, F64, (d, d), 8)], dev)
    check(lib.kpx_moments_add_f64(x.data_ptr(), m, d, sum.data_ptr(), outer.data_ptr(), _stream()), 'kpx_moments_add_f64')
    return sum, outer


# ----------------------------------------------------------------------------------------------- draws of z
MAX_DRAWS = 4096                                                                 # draws of z the uint32 accumulators hold exactly


def draw_moments_add(x, sum, sumsq):
    """One draw of z into the accumulators of the draw diversity: per value of x (contiguous fp32, any shape), the
    8-bit value q evaluate.py writes (as ``frame_metrics(png8=True)``): sum += q, sumsq += q * q.  ``sum`` / ``sumsq``: contiguous int32
    tensors (the bits of uint32) of x's size on x's device, zeroed before the first draw; exact for up to 4096 draws.  One launch."""
    dev = check_tensors('draw_moments_add', [('x', x, F32, None)])
    check_tensors('draw_moments_add', [('sum', sum, I32, x.numel()), ('sumsq', sumsq, I32, x.numel())], dev)
    if sum.data_ptr() == sumsq.data_ptr() and x.numel():
        raise _lib.KpxError('draw_moments_add: sum and sumsq must be two buffers')
    check(lib.kpx_draw_moments_add_f32(x.data_ptr(), x.numel(), sum.data_ptr(), sumsq.data_ptr(), _stream()), 'kpx_draw_moments_add_f32')


def draw_diversity(sum, sumsq, draws, frame_shape, std_map=False, out=None):
    """The diversity of ``draws`` draws of z from the accumulators ``draw_moments_add`` filled.  ``frame_shape`` =
    (H, W, C) of one frame, C in (1, 3), H and W in [1, 1024]; the accumulators hold N = numel / (H W C) >= 1 frames; 2 <= draws <= 4096.
    -> div_mse fp32 [N]: per frame the mean over pairs of draws of the MSE between their 8-bit frames (q / 255 scale), exact up to its one
    rounding.  ``std_map``: also the per-pixel spread uint8 [N,H,W] = floor(2 * sqrt(mean over channels of the variance of q)), capped at
    255 -> (div_mse, std_map); True allocates it, a contiguous uint8 [N,H,W] tensor is written into.  ``out``: a contiguous fp32 [N]
    tensor for div_mse.  One launch."""
    dev = check_tensors('draw_diversity', [('sum', sum, I32, None)])
    check_tensors('draw_diversity', [('sumsq', sumsq, I32, sum.numel())], dev)
    try:
        h, w, c = (int(v) for v in frame_shape)
        d = int(draws)
    except (TypeError, ValueError):
        raise _lib.KpxError('draw_diversity: frame_shape must be (H, W, C) and draws an integer (got %r, %r)' % (frame_shape, draws))
    if not (1 <= h <= 1024 and 1 <= w <= 1024) or c not in (1, 3):
        raise _lib.KpxError('draw_diversity: needs H and W in [1, 1024] and C in (1, 3) (got %r)' % (tuple(frame_shape),))
    if not 2 <= d <= MAX_DRAWS:
        raise _lib.KpxError('draw_diversity: needs 2 <= draws <= %d (got %d)' % (MAX_DRAWS, d))
    n = sum.numel() // (h * w * c)
    if n < 1 or n * h * w * c != sum.numel():
        raise _lib.KpxError('draw_diversity: the accumulators must hold N >= 1 frames of %d x %d x %d (got %d values)' % (h, w, c, sum.numel()))
    out = check_out('draw_diversity', 'out', out, F32, (n,), dev)
    smap = None
    if isinstance(std_map, torch.Tensor) or std_map:
        smap = check_out('draw_diversity', 'std_map', std_map if isinstance(std_map, torch.Tensor) else None, U8, (n, h, w), dev)
    check(lib.kpx_draw_diversity_f32(sum.data_ptr(), sumsq.data_ptr(), n, h, w, c, d, out.data_ptr(), _ptr(smap), _stream()),
          'kpx_draw_diversity_f32')
    return out if smap is None else (out, smap)


def keypoint_draw_metrics(pts, real, diversity=True, out=None):
    """Key-point error and diversity of D draws of z: pts contiguous fp32 [D,N,T,K,2], real contiguous fp32 [N,T,K,2]
    (the labels) on one device, D <= 4096 -> (l2, div): l2 fp32 [D,N,T] = the mean over the K points of the Euclidean distance to the label,
    div fp32 [N,T] = the mean over pairs of draws and points of the distance between the draws (None with ``diversity=False``; needs
    D >= 2).  fp64 arithmetic in a fixed order, rounded once.  ``out``: (l2, div) tensors to write into.  One launch."""
    dev = check_tensors('keypoint_draw_metrics', [('pts', pts, F32, (ANY, ANY, ANY, ANY, 2))])
    d, n, t, k, _ = pts.shape
    check_tensors('keypoint_draw_metrics', [('real', real, F32, (n, t, k, 2))], dev)
    if min(d, n, t, k) < 1 or d > MAX_DRAWS:
        raise _lib.KpxError('keypoint_draw_metrics: needs 1 <= D <= %d and N, T, K >= 1 (got %s)' % (MAX_DRAWS, tuple(pts.shape)))
    if diversity and d < 2:
        raise _lib.KpxError('keypoint_draw_metrics: the diversity needs D >= 2 draws (got %d); pass diversity=False' % d)
    l2, div = out if out is not None else (None, None)
    if div is not None and not diversity:
        raise _lib.KpxError('keypoint_draw_metrics: out has a div tensor but diversity=False')
    l2 = check_out('keypoint_draw_metrics', 'out l2', l2, F32, (d, n, t), dev)
    div = check_out('keypoint_draw_metrics', 'out div', div, F32, (n, t), dev) if diversity else None
    check(lib.kpx_keypoint_draw_metrics_f32(pts.data_ptr(), real.data_ptr(), d, n, t, k, l2.data_ptr(), _ptr(div), _stream()),
          'kpx_keypoint_draw_metrics_f32')
    return l2, div


# ----------------------------------------------------------------------------------------------- contact sheets, animated grids, GIFs
SHEET_PREMAPS = {'unit': 0, 'raw': 1}                                             # = KPX_SHEET_* of include/kpx.h
SHEET_MAX_FRAMES = 64                                                             # = KPX_SHEET_MAX_FRAMES


def sheet_paste(canvas, src, frames, row, col, premap):
    """Frames of a rollout into a contact sheet, as the bytes evaluate.py writes.  canvas: contiguous uint8
    [B, rows*H, cols*W, 3]; src: contiguous fp32 [B,F,H,W,C], C in (1, 3) (C = 1 goes to the three channels), on canvas's device; frames:
    1 <= J <= 64 ints in [0, F), any order, repeats allowed.  canvas[b, row*H:(row+1)*H, (col+j)*W:(col+j+1)*W] = q(src[b, frames[j]]) for
    every b and j; nothing else is written.  ``premap``: 'unit' the bytes of ``_save_img(rescale=True)`` (``frame_metrics(png8=True)``'s
    quantiser), 'raw' those of ``_save_img(rescale=False)`` for values in [0, 1]; both clamp to [0, 255] and send NaN to 0.  rows and cols
    (from the canvas shape) in [1, 64], H and W in [1, 1024], row < rows, col + J <= cols.  One launch on the current stream; the frame
    indices travel in the launch arguments (capturable)."""
    check_tensors('sheet_paste', [('canvas', canvas, U8, (ANY, ANY, ANY, 3)), ('src', src, F32, (ANY,) * 5)])
    if premap not in SHEET_PREMAPS:
        raise _lib.KpxError('sheet_paste: premap must be one of %s (got %r)' % (sorted(SHEET_PREMAPS), premap))
    b, f, h, w, c = src.shape
    if b < 1 or f < 1 or not (1 <= h <= 1024 and 1 <= w <= 1024) or c not in (1, 3):
        raise _lib.KpxError('sheet_paste: src needs B, F >= 1, H and W in [1, 1024] and C in (1, 3) (got %s)' % (tuple(src.shape),))
    if canvas.shape[0] != b or canvas.shape[1] % h or canvas.shape[2] % w:
        raise _lib.KpxError('sheet_paste: canvas must be [%d, rows * %d, cols * %d, 3] (got %s)' % (b, h, w, tuple(canvas.shape)))
    rows, cols = canvas.shape[1] // h, canvas.shape[2] // w
    if not (1 <= rows <= 64 and 1 <= cols <= 64):
        raise _lib.KpxError('sheet_paste: a sheet has 1 to 64 rows and columns of cells (got %d x %d)' % (rows, cols))
    try:
        idx = [int(v) for v in frames]
        row, col = int(row), int(col)
    except (TypeError, ValueError):
        raise _lib.KpxError('sheet_paste: frames must be a sequence of integers, row and col integers (got %r, %r, %r)' % (frames, row, col))
    if any(i != v for i, v in zip(idx, frames)):
        raise _lib.KpxError('sheet_paste: frames must be integers (got %r)' % (frames,))
    if not 1 <= len(idx) <= SHEET_MAX_FRAMES or any(not 0 <= i < f for i in idx):
        raise _lib.KpxError('sheet_paste: needs 1 to %d frame indices in [0, %d) (got %r)' % (SHEET_MAX_FRAMES, f, idx))
    if not 0 <= row < rows or col < 0 or col + len(idx) > cols:
        raise _lib.KpxError('sheet_paste: %d cells from (row %d, col %d) do not fit a sheet of %d x %d cells' % (len(idx), row, col, rows, cols))
    check(lib.kpx_sheet_paste_u8_f32(src.data_ptr(), b, f, h, w, c, (_lib.c_int * len(idx))(*idx), len(idx), canvas.data_ptr(), rows, cols,
                                     row, col, SHEET_PREMAPS[premap], _stream()), 'kpx_sheet_paste_u8_f32')
    return canvas


CELL_MAX_POINTS = 64                                                              # markers per frame of kpx_cell_frames_u8_f32
CELL_MAX_RADIUS = 16


def cell_frames(canvas, first, seq, row, col, premap, pts_first=None, pts_seq=None, colors=None, radius=0):
    """One cell of an animated grid, optionally with key-point markers (DESIGN.md sections 2 and 4.4).  canvas: contiguous uint8
    [B, T+1, rows*H, cols*W, 3]; first: contiguous fp32 [B,H,W,C] and seq: contiguous fp32 [B,T,H,W,C], C in (1, 3), on canvas's device.
    canvas[b, 0, cell] = q(first[b]) and canvas[b, t+1, cell] = q(seq[b, t]) with ``premap`` as in ``sheet_paste``; nothing outside cell
    (row, col) is written.  ``radius`` r in [1, 16]: pts_first fp32 [B,K,2] and pts_seq fp32 [B,T,K,2] (x, y in [-1, 1], the convention of
    ``gaussian_maps``), 1 <= K <= 64, and colors uint8 [K,3] on the device draw a disc of radius r - 1 in colors[k] with a one-pixel black
    outline at every key point (centres in 1/16 pixel, integer distances, the lowest k on top, clipped to the cell; a non-finite point or
    one beyond +-4 draws nothing).  r = 0 draws none and takes no points.  rows and cols (from the canvas shape) in [1, 64], H and W in
    [1, 1024].  One launch on the current stream; capturable."""
    dev = check_tensors('cell_frames', [('canvas', canvas, U8, (ANY, ANY, ANY, ANY, 3)), ('seq', seq, F32, (ANY,) * 5)])
    if premap not in SHEET_PREMAPS:
        raise _lib.KpxError('cell_frames: premap must be one of %s (got %r)' % (sorted(SHEET_PREMAPS), premap))
    b, t_, h, w, c = seq.shape
    if b < 1 or t_ < 1 or not (1 <= h <= 1024 and 1 <= w <= 1024) or c not in (1, 3):
        raise _lib.KpxError('cell_frames: seq needs B, T >= 1, H and W in [1, 1024] and C in (1, 3) (got %s)' % (tuple(seq.shape),))
    check_tensors('cell_frames', [('first', first, F32, (b, h, w, c))], dev)
    if canvas.shape[0] != b or canvas.shape[1] != t_ + 1 or canvas.shape[2] % h or canvas.shape[3] % w:
        raise _lib.KpxError('cell_frames: canvas must be [%d, %d, rows * %d, cols * %d, 3] (got %s)' % (b, t_ + 1, h, w, tuple(canvas.shape)))
    rows, cols = canvas.shape[2] // h, canvas.shape[3] // w
    if not (1 <= rows <= 64 and 1 <= cols <= 64):
        raise _lib.KpxError('cell_frames: a grid has 1 to 64 rows and columns of cells (got %d x %d)' % (rows, cols))
    if not (_is_int(row) and _is_int(col) and _is_int(radius)):
        raise _lib.KpxError('cell_frames: row, col and radius are integers (got %r, %r, %r)' % (row, col, radius))
    if not (0 <= row < rows and 0 <= col < cols):
        raise _lib.KpxError('cell_frames: cell (row %d, col %d) is outside a grid of %d x %d cells' % (row, col, rows, cols))
    if not 0 <= radius <= CELL_MAX_RADIUS:
        raise _lib.KpxError('cell_frames: radius must be in [0, %d] (got %d)' % (CELL_MAX_RADIUS, radius))
    k = 0
    if radius == 0:
        if pts_first is not None or pts_seq is not None or colors is not None:
            raise _lib.KpxError('cell_frames: radius 0 draws no markers and takes no points or colours')
    else:
        check_tensors('cell_frames', [('pts_first', pts_first, F32, (b, ANY, 2))], dev)
        k = int(pts_first.shape[1])
        if not 1 <= k <= CELL_MAX_POINTS:
            raise _lib.KpxError('cell_frames: needs 1 <= K <= %d key points (got %s)' % (CELL_MAX_POINTS, tuple(pts_first.shape)))
        check_tensors('cell_frames', [('pts_seq', pts_seq, F32, (b, t_, k, 2)), ('colors', colors, U8, (k, 3))], dev)
    check(lib.kpx_cell_frames_u8_f32(first.data_ptr(), seq.data_ptr(), b, t_, h, w, c, _ptr(pts_first), _ptr(pts_seq), k, _ptr(colors), radius,
                                     canvas.data_ptr(), rows, cols, row, col, SHEET_PREMAPS[premap], _stream()), 'kpx_cell_frames_u8_f32')
    return canvas


HIST_CELLS = 32768                                                          # 5-5-5 colour cells
HIST_MAX_PIXELS = 1 << 24                                                         # per group and call: the uint32 sums cannot overflow
GIF_MAX_DITHER = 64


def color_hist_add(rgb, hist):
    """Colour statistics of 8-bit RGB pixels.  rgb: contiguous uint8 [G, n, 3] (any storage offset), 1 <= n <= 2^24;
    hist: contiguous int32 [G, 32768, 4] (the bits of uint32) on rgb's device, updated in place: hist[g, cell] += (count, sum r, sum g,
    sum b) over group g's pixels with cell = (r >> 3) << 10 | (g >> 3) << 5 | b >> 3.  Zero hist first (``hist.zero_()``: a memset node
    under capture).  Integer adds: the same bits in any order.  One launch."""
    dev = check_tensors('color_hist_add', [('rgb', rgb, U8, (ANY, ANY, 3))])
    g, n = int(rgb.shape[0]), int(rgb.shape[1])
    if g < 1 or g > 65535 or not 1 <= n <= HIST_MAX_PIXELS:
        raise _lib.KpxError('color_hist_add: rgb must be [G, n, 3] with 1 <= G <= 65535 and 1 <= n <= 2^24 (got %s)' % (tuple(rgb.shape),))
    check_tensors('color_hist_add', [('hist', hist, I32, (g, HIST_CELLS, 4))], dev)
    check(lib.kpx_color_hist_add_u32(rgb.data_ptr(), g, n, hist.data_ptr(), _stream()), 'kpx_color_hist_add_u32')
    return hist


def palette_map(rgb, palette, sizes, dither=0, pmax=256, out=None):
    """The nearest palette entry of every pixel.  rgb: contiguous uint8 [G,T,H,Wc,3]; palette: contiguous uint8
    [G,256,3]; sizes: contiguous int32 [G] ON THE DEVICE, each in [1, pmax] (clamped into it) -> idx uint8 [G,T,H,Wc] = the smallest
    j < sizes[g] that minimises the squared RGB distance (int32).  ``dither`` A in [0, 64]: the 4 x 4 ordered dither of ``kpx_amd.gif.BAYER4``
    added to every channel before the search, A = 0 the plain search.  Any width and storage offset.  One launch."""
    dev = check_tensors('palette_map', [('rgb', rgb, U8, (ANY, ANY, ANY, ANY, 3))])
    g, t, h, w = (int(v) for v in rgb.shape[:4])
    if min(g, t, h, w) < 1 or g > 65535 or t * h * w > 0x7fffffff:
        raise _lib.KpxError('palette_map: rgb must be [G,T,H,Wc,3] with 1 <= G <= 65535 and T H Wc < 2^31 (got %s)' % (tuple(rgb.shape),))
    check_tensors('palette_map', [('palette', palette, U8, (g, 256, 3)), ('sizes', sizes, I32, (g,))], dev)
    if not _is_int(dither) or not 0 <= dither <= GIF_MAX_DITHER:
        raise _lib.KpxError('palette_map: dither is an integer in [0, %d] (got %r)' % (GIF_MAX_DITHER, dither))
    if not _is_int(pmax) or not 1 <= pmax <= 256:
        raise _lib.KpxError('palette_map: pmax is an integer in [1, 256] (got %r)' % (pmax,))
    out = check_out('palette_map', 'out', out, U8, (g, t, h, w), dev)
    check(lib.kpx_palette_map_u8(rgb.data_ptr(), g, t, h, w, palette.data_ptr(), sizes.data_ptr(), pmax, dither, out.data_ptr(), _stream()),
          'kpx_palette_map_u8')
    return out


def gif_indices(canvas, dither=0):
    """An 8-bit canvas to palette indices, one palette per group from all its frames.  canvas: contiguous uint8
    [G,T,H,Wc,3] with T H Wc <= 2^24 -> (idx uint8 [G,T,H,Wc] on the device, palettes uint8 numpy [G,256,3] zero-padded, sizes int numpy [G]).
    ``color_hist_add`` on the device, ``kpx_amd.gif.median_cut`` on the host (512 KB per group cross over), ``palette_map`` on the device."""
    from . import gif as _gif
    dev = check_tensors('gif_indices', [('canvas', canvas, U8, (ANY, ANY, ANY, ANY, 3))])
    g = int(canvas.shape[0])
    hist = torch.zeros((g, HIST_CELLS, 4), dtype=I32, device=dev)
    color_hist_add(canvas.view(g, -1, 3), hist)
    host = hist.cpu().numpy().view(np.uint32)
    palettes, sizes = np.zeros((g, 256, 3), np.uint8), np.zeros((g,), np.int32)
    for i in range(g):
        pal = _gif.median_cut(host[i])
        palettes[i, :pal.shape[0]], sizes[i] = pal, pal.shape[0]
    idx = palette_map(canvas, torch.from_numpy(palettes).to(dev), torch.from_numpy(sizes).to(dev), dither)
    return idx, palettes, sizes


# ----------------------------------------------------------------------------------------------- driven rollouts
RETARGET_MODES = {'hold': 0, 'absolute': 1, 'relative': 2}                       # = KPX_RETARGET_* of include/kpx.h ('relative' + scaled: 3)
RETARGET_MAX_POINTS = 1024


def points_retarget(src_first, mode, drv_first=None, drv_seq=None, shift=0, scaled=False, frames=None, out=None):
    """The key-point sequence of a driven rollout: src_first contiguous fp32 [B,K,2], the source images' key points;
    drv_first [B,K,2] and drv_seq [B,T,K,2], the drivers' key points at frame 0 and at frames 1..T; sample b is driven by sample
    (b + shift) mod B -> out fp32 [B,T,K,2]:
      'hold'      out[b,t] = src_first[b] (T from ``frames``; takes no driver)
      'absolute'  out[b,t] = drv_seq[j,t] (drv_first is not read and may be omitted)
      'relative'  out[b,t] = src_first[b] + s_b * (drv_seq[j,t] - drv_first[j]); s_b = 1, or with ``scaled`` the ratio of the spreads of
                  the two frame-0 constellations about their means (1 when either is 0 or non-finite)
    'hold' and 'absolute' are bit copies, 'relative' is computed in fp64 and rounded once.  1 <= K <= 1024, 0 <= shift < B,
    B*T*K*2 < 2^31.  One launch on the current stream; capturable."""
    if mode not in RETARGET_MODES:
        raise _lib.KpxError('points_retarget: mode must be one of %s (got %r)' % (sorted(RETARGET_MODES), mode))
    if scaled and mode != 'relative':
        raise _lib.KpxError("points_retarget: scaled belongs to mode 'relative' (got %r)" % (mode,))
    if mode == 'hold':
        if drv_first is not None or drv_seq is not None:
            raise _lib.KpxError("points_retarget: mode 'hold' takes no driver")
    elif drv_seq is None or (mode == 'relative' and drv_first is None):
        raise _lib.KpxError('points_retarget: mode %r needs %s' % (mode, 'drv_first and drv_seq' if mode == 'relative' else 'drv_seq'))
    elif frames is not None:
        raise _lib.KpxError("points_retarget: frames belongs to mode 'hold'; mode %r takes T from drv_seq" % (mode,))
    dev = check_tensors('points_retarget', [('src_first', src_first, F32, (ANY, ANY, 2))])
    b, k, _ = src_first.shape
    if mode == 'hold':
        if not _is_int(frames):
            raise _lib.KpxError("points_retarget: mode 'hold' takes the number of frames as frames= (got %r)" % (frames,))
        t_ = frames
    else:
        check_tensors('points_retarget', [('drv_seq', drv_seq, F32, (b, ANY, k, 2)), ('drv_first', drv_first, F32, (b, k, 2), *OPTIONAL)], dev)
        t_ = drv_seq.shape[1]
    if b < 1 or t_ < 1 or not 1 <= k <= RETARGET_MAX_POINTS or b * t_ * k * 2 >= 2 ** 31:
        raise _lib.KpxError('points_retarget: needs B, T >= 1, 1 <= K <= %d and B*T*K*2 < 2^31 (got B = %d, T = %d, K = %d)'
                            % (RETARGET_MAX_POINTS, b, t_, k))
    if not _is_int(shift) or not 0 <= shift < b:
        raise _lib.KpxError('points_retarget: shift must be an integer in [0, B = %d) (got %r)' % (b, shift))
    out = check_out('points_retarget', 'out', out, F32, (b, t_, k, 2), dev)
    check(lib.kpx_points_retarget_f32(src_first.data_ptr(), _ptr(drv_first) if mode == 'relative' else None, _ptr(drv_seq), b, t_, k, shift,
                                      RETARGET_MODES[mode] + (1 if scaled else 0), out.data_ptr(), _stream()), 'kpx_points_retarget_f32')
    return out


# ----------------------------------------------------------------------------------------------- the detector's stability
WARP_MAX_ROWS = 1 << 16                                                           # = KPX_WARP_MAX_ROWS
EQUIV_MAX_ROWS, EQUIV_MAX_POINTS = 1 << 20, 1024                                  # = KPX_EQUIV_MAX_ROWS; K of kpx_equivariance_scores_f32


def _table_rows(what, rows, maps, maps_name, n, max_rows, dev, check_tables):
    """The two tables the stability entries share: rows contiguous int32 [R] (every value in [0, n)) and maps contiguous fp64 [R,6] (finite)
    on ``dev``, 1 <= R <= max_rows -> R.  The value checks read the tables back to the host; ``check_tables=False`` (or a stream that is
    capturing, where nothing can be read back) skips them."""
    check_tensors(what, [('rows', rows, I32, (ANY,))], dev)
    r = rows.shape[0]
    if not 1 <= r <= max_rows:
        raise _lib.KpxError('%s: needs 1 <= R <= %d rows (got %d)' % (what, max_rows, r))
    check_tensors(what, [(maps_name, maps, F64, (r, 6))], dev)
    if check_tables and not torch.cuda.is_current_stream_capturing():
        lo, hi = (int(v) for v in torch.aminmax(rows))
        if lo < 0 or hi >= n:
            raise _lib.KpxError('%s: every frame number must lie in [0, %d) (got values from %d to %d)' % (what, n, lo, hi))
        if not bool(torch.isfinite(maps).all()):
            raise _lib.KpxError('%s: %s has a non-finite coefficient' % (what, maps_name))
    return r


def affine_warp(frames, rows, coef, out=None, check_tables=True):
    """Frames resampled through affine maps (the detector's stability): frames contiguous fp32 [N,H,W,C], C in (1, 3),
    H and W in [1, 1024], finite; rows contiguous int32 [R], the source frame of each output row (any order, repeats allowed); coef contiguous
    fp64 [R,6], the INVERSE map of each row in pixel units: output pixel (x, y) reads the source at (c0 x + c1 y + c2, c3 x + c4 y + c5),
    clamped to the frame (edge replication), bilinear -> fp32 [R,H,W,C].  fp64 arithmetic, nothing fused, one rounding: the bits of the numpy
    float64 restatement; maps that send pixels to pixels copy input bits.  1 <= R <= 65536.  ``out``: a contiguous fp32 [R,H,W,C] tensor
    to write into.  One launch on the current stream (capturable with ``check_tables=False``, which skips reading the tables back for the
    range check of the frame numbers and the finiteness of the coefficients)."""
    dev = check_tensors('affine_warp', [('frames', frames, F32, (ANY,) * 4)])
    n, h, w, c = frames.shape
    if n < 1 or not (1 <= h <= 1024 and 1 <= w <= 1024) or c not in (1, 3):
        raise _lib.KpxError('affine_warp: needs N >= 1, H and W in [1, 1024] and C in (1, 3) (got %s)' % (tuple(frames.shape),))
    r = _table_rows('affine_warp', rows, coef, 'coef', n, WARP_MAX_ROWS, dev, check_tables)
    out = check_out('affine_warp', 'out', out, F32, (r, h, w, c), dev)
    check(lib.kpx_affine_warp_f32(frames.data_ptr(), n, h, w, c, rows.data_ptr(), coef.data_ptr(), r, out.data_ptr(), _stream()),
          'kpx_affine_warp_f32')
    return out


def equivariance_scores(pts, pts_w, rows, fwd, out=None, check_tables=True):
    """The detector's equivariance error: pts contiguous fp32 [N,K,2] (x, y), the key points of the original frames;
    pts_w contiguous fp32 [R,K,2], those of the warped frames; rows contiguous int32 [R], the original frame of each row; fwd contiguous fp64
    [R,6], the FORWARD map of each row in the key points' normalised coordinates -> (scores fp32 [R,K,2], valid uint8 [R,K], frame_mean fp32
    [R,2], n_valid int32 [R]): scores = (err, moved) = (|pts_w - target|, |target - p|) with target = M p + t; valid = 1 where p, pts_w and
    the target are finite and the target lies in [-1, 1]^2; frame_mean = the means of both over the row's valid points (NaN without any);
    n_valid their number.  fp64 arithmetic in a fixed order, rounded once.  1 <= K <= 1024, 1 <= R <= 2^20.  ``out``: the four tensors to
    write into.  One launch on the current stream (``check_tables`` as in ``affine_warp``)."""
    dev = check_tensors('equivariance_scores', [('pts', pts, F32, (ANY, ANY, 2))])
    n, k, _ = pts.shape
    if n < 1 or not 1 <= k <= EQUIV_MAX_POINTS:
        raise _lib.KpxError('equivariance_scores: pts [N,K,2] needs N >= 1 and K in [1, %d] (got %s)' % (EQUIV_MAX_POINTS, tuple(pts.shape)))
    check_tensors('equivariance_scores', [('pts_w', pts_w, F32, (ANY, k, 2))], dev)
    r = _table_rows('equivariance_scores', rows, fwd, 'fwd', n, EQUIV_MAX_ROWS, dev, check_tables)
    if pts_w.shape[0] != r:
        raise _lib.KpxError('equivariance_scores: pts_w must have one entry per row (got %s for %d rows)' % (tuple(pts_w.shape), r))
    outs = list(out) if out is not None else [None] * 4
    if len(outs) != 4:
        raise _lib.KpxError('equivariance_scores: out must be (scores, valid, frame_mean, n_valid)')
    specs = (('scores', F32, (r, k, 2)), ('valid', U8, (r, k)), ('frame_mean', F32, (r, 2)), ('n_valid', I32, (r,)))
    outs = [check_out('equivariance_scores', 'out ' + name, o, dtype, shape, dev) for o, (name, dtype, shape) in zip(outs, specs)]
    check(lib.kpx_equivariance_scores_f32(pts.data_ptr(), pts_w.data_ptr(), rows.data_ptr(), fwd.data_ptr(), r, k, outs[0].data_ptr(),
                                          outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), _stream()), 'kpx_equivariance_scores_f32')
    return tuple(outs)


# ----------------------------------------------------------------------------------------------- landmark regression
JOINT_MAX_POINTS, JOINT_MAX_JOINTS, JOINT_MAX_FRAMES, JOINT_MAX_ALPHAS = 64, 32, 1 << 20, 8     # = KPX_JOINT_MAX_* of include/kpx.h


def _joint_sizes(what, f, k, j):
    if not (1 <= f <= JOINT_MAX_FRAMES and 1 <= k <= JOINT_MAX_POINTS and 1 <= j <= JOINT_MAX_JOINTS):
        raise _lib.KpxError('%s: needs 1 <= F <= %d, 1 <= K <= %d and 1 <= J <= %d (got F = %d, K = %d, J = %d)'
                            % (what, JOINT_MAX_FRAMES, JOINT_MAX_POINTS, JOINT_MAX_JOINTS, f, k, j))


def joint_targets(xy, vis, bbox, crop_map):
    """Annotated joints in the key points' coordinates (landmark regression): xy contiguous fp32 [F,J,2], the joints in
    the original frame's pixels; vis contiguous uint8 [F,J]; bbox contiguous fp32 [F,4] = (x0, y0, x1, y1); crop_map contiguous fp64 [4] =
    (ax, bx, ay, by) on the same device (``kpx_amd.joints.crop_map``) -> (target fp32 [F,J,2] = (ax x + bx, ay y + by) in fp64, rounded once;
    mask uint8 [F,J] = visible, finite and inside [-1,1]^2; norm fp32 [F] = max(|ax| (x1 - x0), |ay| (y1 - y0)), NaN for a box that is not
    finite or not positive).  1 <= F <= 2^20, 1 <= J <= 32.  One launch on the current stream."""
    dev = check_tensors('joint_targets', [('xy', xy, F32, (ANY, ANY, 2))])
    f, j, _ = xy.shape
    check_tensors('joint_targets', [('vis', vis, U8, (f, j)), ('bbox', bbox, F32, (f, 4)), ('crop_map', crop_map, F64, (4,))], dev)
    _joint_sizes('joint_targets', f, 1, j)
    target = torch.empty((f, j, 2), dtype=F32, device=dev)
    mask = torch.empty((f, j), dtype=U8, device=dev)
    norm = torch.empty((f,), dtype=F32, device=dev)
    check(lib.kpx_joint_targets_f32(xy.data_ptr(), vis.data_ptr(), bbox.data_ptr(), crop_map.data_ptr(), f, j, target.data_ptr(), mask.data_ptr(),
                                    norm.data_ptr(), _stream()), 'kpx_joint_targets_f32')
    return target, mask, norm


def _joint_frames(what, pts, target, mask):
    """The three per-frame tensors the regression entries share: pts fp32 [F,K,2], target fp32 [F,J,2], mask uint8 [F,J] -> (F, K, J, device)."""
    dev = check_tensors(what, [('pts', pts, F32, (ANY, ANY, 2))])
    f, k, _ = pts.shape
    check_tensors(what, [('target', target, F32, (f, ANY, 2))], dev)
    j = target.shape[1]
    check_tensors(what, [('mask', mask, U8, (f, j))], dev)
    return f, k, j, dev


def joint_moments_add(pts, target, mask, g, bm, n):
    """Frames into the masked normal equations of the landmark regression: pts contiguous fp32 [F,K,2]; target
    contiguous fp32 [F,J,2]; mask contiguous uint8 [F,J]; in place g fp64 [J,D,D] += sum_f phi_f phi_f^T, bm fp64 [J,D,2] += sum_f phi_f
    target[f,j]^T and n int64 [J] += the number of frames, over the frames with mask[f,j] set and finite key points, phi_f = (pts[f], 1),
    D = 2K + 1; zeroed by the caller before the first call.  Every element takes its frames in ascending order with one fma each, so any
    split of the frames into consecutive calls gives the same bits and g stays bitwise symmetric.  1 <= K <= 64, 1 <= J <= 32,
    1 <= F <= 2^20.  One launch on the current stream.  -> (g, bm, n)."""
    f, k, j, dev = _joint_frames('joint_moments_add', pts, target, mask)
    d = 2 * k + 1
    check_tensors('joint_moments_add', [('g', g, F64, (j, d, d)), ('bm', bm, F64, (j, d, 2)), ('n', n, I64, (j,))], dev)
    _joint_sizes('joint_moments_add', f, k, j)
    check(lib.kpx_joint_moments_add_f64(pts.data_ptr(), target.data_ptr(), mask.data_ptr(), f, k, j, g.data_ptr(), bm.data_ptr(), n.data_ptr(),
                                        _stream()), 'kpx_joint_moments_add_f64')
    return g, bm, n


def joint_scores(pts, target, mask, norm, w, alpha):
    """The landmark regressor applied: pts contiguous fp32 [F,K,2]; target contiguous fp32 [F,J,2]; mask contiguous
    uint8 [F,J]; norm contiguous fp32 [F]; w contiguous fp64 [J,D,2], D = 2K + 1; alpha contiguous fp64 [A], 1 <= A <= 8 -> (pred fp32
    [F,J,2] = phi_f W[j], err fp32 [F,J] = |pred - target|, hits uint8 [F,J] with bit a set when the entry is valid, norm[f] is finite and
    err <= alpha[a] norm[f]; per call sum_err fp64 [J] and count int64 [J] over the valid entries (mask set, finite key points) in ascending
    f, pck_count int64 [J] those of them with a finite norm, hit_count int64 [J,A]).  fp64 arithmetic in a fixed order, nothing fused, each
    stored value rounded once.  One launch on the current stream."""
    f, k, j, dev = _joint_frames('joint_scores', pts, target, mask)
    check_tensors('joint_scores', [('norm', norm, F32, (f,)), ('w', w, F64, (j, 2 * k + 1, 2)), ('alpha', alpha, F64, (ANY,))], dev)
    _joint_sizes('joint_scores', f, k, j)
    a = alpha.shape[0]
    if not 1 <= a <= JOINT_MAX_ALPHAS:
        raise _lib.KpxError('joint_scores: needs 1 <= A <= %d thresholds (got %d)' % (JOINT_MAX_ALPHAS, a))
    pred = torch.empty((f, j, 2), dtype=F32, device=dev)
    err = torch.empty((f, j), dtype=F32, device=dev)
    hits = torch.empty((f, j), dtype=U8, device=dev)
    sum_err = torch.empty((j,), dtype=F64, device=dev)
    count = torch.empty((j,), dtype=I64, device=dev)
    pck_count = torch.empty((j,), dtype=I64, device=dev)
    hit_count = torch.empty((j, a), dtype=I64, device=dev)
    check(lib.kpx_joint_scores_f32(pts.data_ptr(), target.data_ptr(), mask.data_ptr(), norm.data_ptr(), w.data_ptr(), alpha.data_ptr(), f, k, j, a,
                                   pred.data_ptr(), err.data_ptr(), hits.data_ptr(), sum_err.data_ptr(), count.data_ptr(), pck_count.data_ptr(),
                                   hit_count.data_ptr(), _stream()), 'kpx_joint_scores_f32')
    return pred, err, hits, sum_err, count, pck_count, hit_count


# ----------------------------------------------------------------------------------------------- action classifier
MAX_CLASS_ROWS, MAX_CLASSES = 1 << 20, 1024                                      # limits of the three classifier entries on B / M and A


def class_scores(logits, target, confusion=None, out=None, check_target=True):
    """Per row of logits (contiguous fp32 [M,A]) against target (contiguous int32 [M], every value in [0, A)) -> (pred int32 [M], rank
    int32 [M], logp fp32 [M]): pred = the lowest index among the row's maxima, rank = 1 + the number of other
    classes whose logit is >= the target's (a tie counts against the model), logp = the target's log-softmax.  ``confusion``: a contiguous
    int32 [A,A] tensor, [target, pred] += 1 (zeroed by the caller before the first call).  A row with a non-finite logit gets pred = -1,
    rank = A, logp = NaN and is left out of ``confusion``.  ``out``: (pred, rank, logp) tensors to write into.  One launch.  The range
    check of the targets reads them back to the host before the launch; a caller that has checked them (or is capturing a graph, where
    nothing can be read back) passes ``check_target=False``."""
    dev = check_tensors('class_scores', [('logits', logits, F32, (ANY, ANY))])
    m, a = logits.shape
    if not 1 <= m <= MAX_CLASS_ROWS or not 1 <= a <= MAX_CLASSES:
        raise _lib.KpxError('class_scores: needs 1 <= rows <= %d and 1 <= classes <= %d (got %s)' % (MAX_CLASS_ROWS, MAX_CLASSES, tuple(logits.shape)))
    check_tensors('class_scores', [('target', target, I32, (m,)), ('confusion', confusion, I32, (a, a), *OPTIONAL)], dev)
    pred, rank, logp = out if out is not None else (None, None, None)
    pred = check_out('class_scores', 'out pred', pred, I32, (m,), dev)
    rank = check_out('class_scores', 'out rank', rank, I32, (m,), dev)
    logp = check_out('class_scores', 'out logp', logp, F32, (m,), dev)
    if check_target and not torch.cuda.is_current_stream_capturing():
        lo, hi = (int(v) for v in torch.aminmax(target))
        if lo < 0 or hi >= a:
            raise _lib.KpxError('class_scores: every target must lie in [0, %d) (got values from %d to %d)' % (a, lo, hi))
    check(lib.kpx_class_scores_f32(logits.data_ptr(), target.data_ptr(), m, a, pred.data_ptr(), rank.data_ptr(), logp.data_ptr(),
                                   _ptr(confusion), _stream()), 'kpx_class_scores_f32')
    return pred, rank, logp


# ----------------------------------------------------------------------------------------------- nearest training motion
from .novelty import seq_nearest, NEAREST_GROUP, NEAREST_MAX_QUERIES, NEAREST_MAX_WINDOWS      # noqa: E402,F401

# ----------------------------------------------------------------------------------------------- key-point resampling in time
from .resample import points_resample, points_speed, RESAMPLE_MODES, RESAMPLE_MAX_POINTS, RESAMPLE_MAX_RATE      # noqa: E402,F401

# ----------------------------------------------------------------------------------------------- k nearest rows of a set; precision / recall / density / coverage
from .prdc import set_neighbours, prdc, SET_MAX_K, SET_MAX_DIM, SET_MAX_QUERIES, SET_MAX_REFS      # noqa: E402,F401

# evaluate.py --video: the wrappers are written beside the tables and the container in mjpeg.py
from .mjpeg import jpeg_scans, jpeg_encode, JPEG_MIN_SIDE, JPEG_MAX_SIDE, JPEG_BUDGET      # noqa: E402,F401

# evaluate.py --posterior, animate.py --interpolate / --motion-from: the wrappers are written beside the host-side summary in posterior.py
from .posterior import (latent_stats_add, latent_sample, latent_path, LATENT_MAX_DIM, LATENT_STATE_FIELDS,      # noqa: E402,F401
                        LATENT_PATH_MAX_STEPS, LATENT_PATH_MODES)
