#!/usr/bin/env python3
"""Evaluation entry point with the reference's CLI (reference: evaluate.py:13-163):

    python evaluate.py --config configs/penn.yaml --checkpoint_stage1 S1.npz --checkpoint_stage2 S2.npz [--save_dir results/eval]
                       [--synthetic N] [--colors_seed S] [--no-save]
                       [--metrics [--samples N] [--vgg-metrics [--synthetic-vgg] [--frechet]] [--motion-metrics]]
                       [--actions all|i,j,k [--sheet-frames f,g,h]]
                       [--drive labels,hold,transfer [--drive-scaled] [--drive-only] [--sheet-frames f,g,h]]
                       [--metrics --action-accuracy CKPT]
                       [--gif [--gif-fps N] [--gif-dither A] [--frames N] [--rate F [--resample linear|cubic]]]
                       [--video [--video-fps N] [--video-quality Q] [--frames N] [--rate F [--resample linear|cubic]]]
                       [--metrics --novelty [--novelty-sheets] [--novelty-no-mirror]]
                       [--metrics --prdc [--prdc-k K]]
                       [--posterior [--posterior-transfer] [--posterior-au T]]

One source image -> 32 predicted frames per sample (FinalModel).  PNG writer semantics as the reference (:137-156).  Per sample, as the
reference: input_im.png, real_seq/ (data path only), pred_seq/, mask/, crude/, and the colourised key-points current_points.png and
pred_points/ (:96-97, :107-109, :126-128) in the palette of ``random.Random(--colors_seed)``.  The
test subset of ``paths.data_dir`` is read through kpx_amd.data.SequenceDataLoader (the reference's data/sequence_dataloader.py);
``--synthetic N`` feeds N random images with random one-hot action codes instead.  Checkpoints: the ``.npz`` containers written
by this repo or TensorFlow V2 bundle prefixes (TF variable names either way).

``--metrics`` (data path only) scores every predicted frame against the real future frame -- SSIM and PSNR of the 8-bit frames the script
writes (``kpx_amd.ops.frame_metrics``, one launch per rollout) -- and writes ``<save_dir>/metrics.npz`` (``ssim``, ``psnr``, ``mse``:
[samples, draws, 32]) and ``<save_dir>/metrics.json`` (``summarise_metrics``).  ``--samples N`` runs the rollout N times per batch with
fresh z; the PNGs come from draw 0.

``--vgg-metrics`` (with ``--metrics``) adds the VGG19 feature-space scores of the same 8-bit frames (``kpx_amd.FeatureScorer``: the
network of ``paths.vggnet`` -- ``--synthetic-vgg`` for He-normal weights --, the real frames' features computed once per batch and reused
by every draw): ``vgg_cos`` and ``vgg_l1`` [samples, draws, 32] and their per-layer parts ``vgg_cos_layers`` / ``vgg_l1_layers``
[samples, draws, 32, 5] in metrics.npz, ``vgg_cos`` / ``vgg_l1`` blocks in metrics.json.  DESIGN.md section 2 has the definition.

``--frechet`` (with ``--metrics --vgg-metrics``) adds a set-level score, which does not punish a draw of z for being a plausible but different
future: the Frechet distance between the feature distributions of the real and the predicted frames, in the feature space of the same VGG19
(this project's own quantity: NOT FID and NOT FVD, which are defined on Inception / I3D features, and not comparable with published figures).
The features the scorer computes anyway are pooled over positions (``kpx_amd.ops.feature_pool``) and their fp64 moments accumulated on the
device (``kpx_amd.ops.moments_add``, ``kpx_amd.frechet.FrechetAccumulator``) over the whole test set, per layer at two levels: frames, and
rollouts of 32 frames (mean pooled feature and mean absolute frame-to-frame change).  metrics.npz gains ``vgg_fd_layers``,
``vgg_fvd_layers`` (all draws against all real frames), ``vgg_fd_draw0_layers`` (the written PNGs) and ``vgg_fd_floor_layers`` /
``vgg_fvd_floor_layers`` (the real even-numbered samples against the real odd-numbered ones: the finite-sample noise floor), each [5], NaN
where a set has fewer than two rows; metrics.json a ``frechet`` block (``summarise_frechet``); and ``<save_dir>/frechet.npz`` holds n, mean
and covariance per set, layer and level (about 120 MB at full width), which ``python -m kpx_amd.frechet a.npz b.npz`` compares later without
a GPU.  The rollouts of ``--actions`` and ``--drive`` are not accumulated.

``--motion-metrics`` (with ``--metrics``; at most 4096 ``--samples``) adds what needs no network: ``kp_l2`` [samples, draws, 32], the mean
distance of each draw's predicted key points to the pseudo labels of the real frames (``kpx_amd.ops.keypoint_draw_metrics``), and with
``--samples`` >= 2 how far the draws lie apart: ``kp_div`` [samples, 32] in key-point space and ``div_mse`` [samples, 32], the mean over
pairs of draws of the MSE between their 8-bit frames (``draw_moments_add`` per draw, ``draw_diversity`` per batch: exact integers), plus
per sample ``pred_std/``, the per-pixel spread of the draws as 8-bit grey PNGs.  Blocks of the same names in metrics.json.

``--actions`` (data path and ``--synthetic``) rolls every source image out under each listed action class at ONE z: per batch and draw
the script draws z itself, gives it to the batch's own rollout (the source of everything above) and to one further rollout per listed
class, whose action code is that class's one-hot row, so the rows of a sheet differ by the class alone.  Per sample, from draw 0:
``classes.png`` (a ``real`` row on the data path, then one row per class; columns: the input image, then the ``--sheet-frames`` frames,
default 3,7,...,31) and ``classes_points.png`` (the colourised key points of the same cells), composed and quantised on the device
(``kpx_amd.ops.sheet_paste``: only the bytes cross to the host), and ``<save_dir>/actions.json``.  With ``--metrics`` the classes at one z
are scored as draws are: ``act_kp_l2`` [samples, classes, draws, 32], ``act_kp_div`` / ``act_div_mse`` [samples, draws, 32] (two or more
classes), ``act_own``, ``act_rank`` and ``actions`` in metrics.npz, an ``actions`` block in metrics.json (``summarise_actions``): under
which class does the rollout land closest to the real motion?  DESIGN.md section 2 has the definitions.

``--drive MODES`` (a comma list of ``labels``, ``hold``, ``transfer``) rolls the translator out on key points that come from outside the motion
generator (``FinalModel.run(drive=...)``, ``kpx_amd.ops.points_retarget``), once per batch, whatever ``--samples`` is -- no z is involved:
``labels`` (data path only) on the pseudo labels of the real frames, the translator's ceiling; ``hold`` on the detected key points of the
input image at every frame, the static-pose floor; ``transfer`` (data path only) on the detected key points moved as the NEXT sample of the
batch moves (its labels minus its frame-0 labels; ``--drive-scaled`` scales that motion by the ratio of the two constellations' spreads; a
batch of one drives itself).  Per sample ``drive_labels/``, ``drive_hold/``, ``drive_transfer/`` (32 predicted PNGs each),
``drive_transfer_points/`` (the colourised driven key points) and ``drive.png``, one sheet composed on the device with the rows ``real``,
``labels``, ``model`` (the sample's own rollout, draw 0), ``hold``, ``driver`` (the driving sample's input image and real frames),
``transfer`` -- those that apply -- and the columns of ``classes.png``; ``<save_dir>/drive.json`` records them.  With ``--metrics``, ``labels``
and ``hold`` are scored against the real frames as the model's frames are: ``drive_labels_ssim`` ... ``drive_hold_mse`` [samples, 32] in
metrics.npz and a ``drive`` block in metrics.json (``summarise_drive``) with ``skill`` = (model - hold) / (labels - hold) per metric.
``--drive-only`` skips the model's own rollout (no ``model`` row, no pred_seq/ ..., metrics.npz holds the ``drive_*`` arrays alone) and needs
no ``--checkpoint_stage2``: a stage-1 checkpoint can be evaluated before a stage-2 checkpoint exists.

``--action-accuracy CKPT`` (with ``--metrics``; data path only) asks a recogniser whether a rollout looks like its class: CKPT is a checkpoint
of ``train.py --mode action_classifier`` (``kpx_amd.ActionClassifierModel``, built from the same config: ``model.classifier_cells``), a
stacked LSTM over the 32 key-point sets trained on the pseudo labels stage 2 learns from.  Per batch it classifies the real key points (the
ceiling) and every draw's predicted key points against the sample's own class, and with ``--actions`` every class rollout of the sweep
against the class that was COMMANDED (``kpx_amd.ops.class_scores``, one launch each).  metrics.npz gains ``cls_own`` [samples],
``cls_real_pred`` / ``_rank`` / ``_logp`` [samples], ``cls_pred_pred`` / ``_rank`` / ``_logp`` [samples, draws], ``cls_confusion_real`` /
``cls_confusion_pred`` [A, A] and, with ``--actions``, ``cls_act_pred`` / ``_rank`` / ``_logp`` [samples, classes, draws] and
``cls_confusion_commanded``; ``kp_fd``, ``kp_fd_draw0`` and ``kp_fd_floor`` are Frechet distances in the recogniser's feature space (fp64
moments on the device, ``kpx_amd.ops.moments_add``); metrics.json an ``action_accuracy`` block (``summarise_action_accuracy``).  This is the
project's own key-point-space quantity: the recogniser never sees a pixel, and the figures are not comparable with published
action-recognition accuracies or FVD.

``--gif`` (data path and ``--synthetic``; not with ``--no-save``) writes the rollout as something that can be watched: per sample ``pred.gif``,
the input image and then the 32 predicted frames of draw 0 -- the frames of input_im.png and pred_seq/ --, and ``compare.gif``, the same
33 frames as one row of cells ``real | pred | points`` (``pred | points`` with ``--synthetic``): frame 0 holds the input image and
current_points, frame t the t-th real frame, predicted frame and pred_points map.  With ``--drive-only`` the pred and points columns are
those of the first driven mode.  The canvases are composed with ``kpx_amd.ops.sheet_paste`` and reduced to ONE palette of at most 256
colours per GIF on the device (``kpx_amd.ops.gif_indices``: colour histogram, median cut, nearest-entry search), so one byte per pixel
crosses to the host, where ``kpx_amd.gif.write_gif`` packs it (LZW in the library's host code).  ``--gif-fps N`` (1..50, default 10) is
stored as the delay round(100 / N) centiseconds; ``--gif-dither A`` (0..64, default 0) adds a 4 x 4 ordered dither of that amplitude
before the search.  ``<save_dir>/gif.json`` records the columns, fps, dither, the frame count and the palette size per sample.  DESIGN.md
section 2 has the definition.  Without the flag every file keeps its bytes.

``--video`` (data path and ``--synthetic``; not with ``--no-save``; with or without ``--gif``) writes the same frames and columns in true
colour: per sample ``pred.avi`` and ``compare.avi``, Motion-JPEG in an AVI container.  Every frame is a baseline JPEG (4:2:0) whose scan is
coded on the device (``kpx_amd.ops.jpeg_encode``: integers only), so only compressed bytes cross to the host, where
``kpx_amd.mjpeg`` adds the headers and the container.  ``--video-fps N`` (1..240, default 10), ``--video-quality Q`` (1..100, default 90:
the IJG quality scale).  ``<save_dir>/video.json`` records the columns, fps, quality, the frame count and the bytes per file;
``python -m kpx_amd.mjpeg FILE.avi --png DIR`` unpacks a file without a GPU.  With ``--frames`` / ``--rate`` also ``long.avi``, played at
F x ``--video-fps`` (a product above 240 is refused; the 2^24-pixel limit of long.gif does not apply to it).

``--frames N`` / ``--rate F`` (with ``--gif`` or ``--video``; data path and ``--synthetic``) add a longer and smoother rollout beside the ordinary one, which
is produced first and keeps every file, metric and byte.  Per batch a second rollout (``FinalModel.run(frames=N, rate=F, resample=...)``,
DESIGN.md section 2) chains N / 32 calls of the motion generator -- segment 0 at draw 0's z, the later ones at z from
``numpy.random.RandomState(first sample index of the batch)`` -- and puts F - 1 key-point frames between every two (``--resample``, default
cubic).  Per sample ``long.gif`` (``pred | points``, 1 + N F frames, played at F x ``--gif-fps``; a product above 50 is refused) and
``long_points.npy`` [N F, K, 2]; per run ``long.json``: ``speed``, the mean over all samples of the mean distance the key points move per
source frame (``kpx_amd.ops.points_speed``), and ``seam_ratio``, the mean speed at the first frame of the segments after the first over the
mean speed at all other frames (null for N = 32).  A chain whose seams jump shows up there as a number; no value is called good.

``--novelty`` (with ``--metrics``; data path only) asks whether the motion generator invents motions or replays training sequences: the
pseudo labels of ``train_set.txt`` are kept in HBM once (``kpx_amd.novelty.MotionStore``) and every draw's predicted key points, the pseudo
labels of the real future and, with ``--actions``, every class rollout are searched in the set of sequences the stage-2 loader can draw
without augmentation -- every legal start frame of every listed video at its own gap, and their mirror images unless
``--novelty-no-mirror`` -- per action class, in fp64, by ``kpx_amd.ops.seq_nearest`` (two launches per batch).  A query never finds the
windows of its own source video.  metrics.npz gains ``nov_d`` [samples, draws] (the RMS point distance to the nearest window, in label
coordinates), ``nov_code`` (2 * window + mirrored, -1 when nothing was found), ``nov_class_d`` [samples, draws, A], ``nov_window`` [samples,
draws, 4] = (listing line, im_idx, gap, mirrored), ``nov_real_d`` / ``nov_real_code`` / ``nov_real_class_d`` / ``nov_real_window`` for the
real future, ``nov_own`` [samples], ``nov_window_action`` [W] and with ``--actions`` ``act_nov_d`` / ``act_nov_code`` [samples, classes,
draws]; metrics.json a ``novelty`` block (``summarise_novelty``): the distances of the rollouts beside those of fresh real motion, their
ratio, the share of rollouts closer than the closest 5 % of the real ones, and how often the nearest training motion belongs to the query's
class.  ``--novelty-sheets`` (at most 31 ``--samples``; not with ``--no-save``) writes per sample ``nearest.png``: a row for the real future,
then per draw the rollout and under it its nearest training window (``MotionStore.gather``), as colourised key points at the
``--sheet-frames`` frames.  This is the project's own key-point-space quantity, not comparable with published figures.  Without the flags
every output keeps its bytes.

``--prdc`` (with ``--metrics``; data path only; ``--prdc-k K``, 1..8, default 5) separates the two ways a class-conditional generator fails
-- collapsing to a few clean modes, or covering every mode and inventing motions beside them -- with the k-nearest-neighbour manifold
estimates of the literature: precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020).  The rows stay on
the device as float32 until the last batch -- in key-point space the 32 K 2 future key points (the pseudo labels of the real frames against
the rollouts), with ``--action-accuracy`` also the recogniser's features (its own classify calls are reused) -- are converted to fp64 once
and scored once by ``kpx_amd.ops.prdc``: four launches of the exact fp64 all-pairs search ``kpx_amd.ops.set_neighbours`` per comparison.
Comparisons per space: ``draw0`` (draw 0 against the real rows, equal set sizes: the headline), ``all_draws``, ``ceiling`` (the even real
samples as generated rows against the odd ones), each again ``_per_class`` (neighbours and balls inside the sample's own class) and with
``--actions`` ``commanded_<a>`` (the draw-0 rollouts under class a against the real rows of class a).  metrics.npz gains the ``prdc_*``
arrays (per comparison the four scores, the set sizes, every row's squared radius, inside count and nearest generated row), metrics.json a
``prdc`` block (``kpx_amd.prdc.summarise``, with ``k``, the set sizes and a definition), and ``<save_dir>/prdc.npz`` keeps the rows, classes
and parities, which ``python -m kpx_amd.prdc prdc.npz [--k K]`` re-scores on the CPU.  These are the project's own key-point-space and
recogniser-space quantities, not comparable with published figures; precision and recall are unstable for unequal set sizes.  Without the
flag every output keeps its bytes.

``--posterior`` (data path only; not with ``--drive-only``; the stage-2 checkpoint must hold ``vae_encoder/*``) reads the one trained network
the other flags ignore: per batch, after everything else of the batch, ``FinalModel.encode`` maps the pseudo labels of the real motion to
logit = [mu | sigma], ``kpx_amd.ops.latent_stats_add`` accumulates them per class and latent dimension on the device (fp64, a fixed order:
a set fed in pieces leaves the bits of one call), and one more rollout runs at z = mu (``kpx_amd.ops.latent_sample(logit, None, 0)``): per
sample ``post_seq/`` and ``post_points/``; with ``--metrics`` ``post_ssim``, ``post_psnr``, ``post_mse`` [samples, 32] in metrics.npz, with
``--motion-metrics`` also ``post_kp_l2``; a ``posterior`` block in metrics.json (``kpx_amd.posterior.summarise_posterior`` and
``summarise_recon``): KL per dimension, active units (``--posterior-au T``, default 0.01), dead mu / sigma shares, the KL of the aggregate
posterior's marginals to the prior, the same per class, the ``recon`` scores and, with ``--drive hold``, ``z_skill`` = (model - hold) /
(posterior - hold).  ``--posterior-transfer`` (not with ``--no-save``) also decodes the mu of sample (b + 1) mod B from sample b's image, first
pose and class: ``post_transfer/`` and the sheet ``posterior.png`` with the rows real | recon | model (draw 0) | driver | transfer at the
``--sheet-frames`` frames.  ``<save_dir>/posterior.npz`` keeps the logit rows, classes, state and counts, which
``python -m kpx_amd.posterior posterior.npz [--au T]`` summarises again without a GPU.  Nothing here draws a random number: without the flags
every output keeps its bytes, and with them every other output does.  This project's own diagnostics on its own pseudo labels, not
comparable with published figures.
"""
import json
import os
import sys
import time
from argparse import ArgumentParser
from os import path as osp

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _save_img(file_path, img, rescale=False, raw=False):
    """reference :137-149; ``raw``: img holds the bytes to write"""
    from PIL import Image
    mode = None
    if img.shape[2] <= 2:
        img = np.squeeze(img, axis=2)
        mode = 'L'
    if rescale:
        img = 0.5 * (img + 1.0)
    if not raw:
        img = (img * 255).astype(np.uint8)
    Image.fromarray(img, mode=mode).save(file_path)


METRICS_DEFINITION = (
    'Per predicted frame against the real future frame, both as the 8-bit PNGs written to pred_seq/ and real_seq/ '
    '(q = uint8(trunc(fl32(fl32(0.5 * fl32(x + 1)) * 255))), scored as q / 255 with dynamic range 1): '
    'SSIM as TF 1.12 tf.image.ssim (11x11 Gaussian window, sigma 1.5, VALID, k1 = 0.01, k2 = 0.03; mean over positions, then channels), '
    'MSE = mean (a - b)^2 over pixels and channels, PSNR = -10 log10(MSE) dB as tf.image.psnr (+inf for MSE = 0). '
    'mean / per_frame: over samples and draws of z. best_of_draws / best_of_draws_per_frame: per sample the draw with the best mean over '
    'its 32 frames, chosen per metric (highest SSIM, highest PSNR, lowest MSE; a tie goes to the lowest draw), then the mean over samples. '
    'Non-finite values are null; n_nonfinite counts the frames with a non-finite metric.')


VGG_FEATURE_LAYERS = ['conv1_2', 'conv2_2', 'conv3_4', 'conv4_4', 'conv5_4']      # = kpx_amd.vgg.FEATURE_LAYERS
VGG_METRICS_DEFINITION = (
    'vgg_cos / vgg_l1: the same 8-bit frames q through the VGG19 of this project (input q on the 0..255 scale, BGR, minus VGG_MEAN; features '
    'conv1_2, conv2_2, conv3_4, conv4_4, conv5_4 as listed in vgg_layers). Per layer and spatial position over the C channels '
    'saa = sum a^2, sbb = sum b^2, dot = sum a b; the position scores 1 if saa == 0 and sbb == 0, 0 if exactly one of them is 0, else '
    'min(1, dot / sqrt(saa sbb)); cos_layer = mean over positions, l1_layer = mean |a - b| over positions and channels (the perceptual '
    'L1 term of stage-1 training, per frame). vgg_cos = mean of cos_layer over the five layers, in [0, 1], higher is better (best draw: '
    'highest); vgg_l1 = mean of l1_layer over the five layers, lower is better (best draw: lowest). Defined on this VGG19 and these layers: '
    'not numerically comparable with published VGG16- or LPIPS-weight figures.')
MOTION_METRICS_DEFINITION = (
    'kp_l2: per draw and predicted frame the mean over the K key points of the Euclidean distance between the predicted point and the '
    'pseudo label of the real frame, in the [-1, 1] image coordinates of the labels, lower is better (best draw: lowest). kp_div: per sample '
    'and frame the mean over the D (D - 1) / 2 pairs of draws and the K points of the distance between the two predictions. div_mse: per '
    'sample and frame the mean over the pairs of draws of the MSE between their 8-bit frames q / 255, computed exactly as '
    'sum (D sum_d q^2 - (sum_d q)^2) / (D (D - 1) / 2 * 255^2 * H W C). kp_div and div_mse exist for two or more draws and are averaged '
    'over samples (mean, per_frame); a model that ignores z scores 0 in both. pred_std/ holds floor(2 sqrt(mean over channels of the '
    'variance of q over the draws)) per pixel, capped at 255.')
MAX_MOTION_DRAWS = 4096                                                           # = kpx_amd.ops.MAX_DRAWS: the uint32 accumulators are exact
LOWER_IS_BETTER = ('mse', 'vgg_l1', 'kp_l2')


def _json_num(v):
    v = float(v)
    return v if np.isfinite(v) else None


def summarise_metrics(ssim, psnr, mse, extras=None, motion=None):
    """metrics.json content from per-frame metrics of shape [S, N, T] (S samples, N draws of z, T predicted frames); numpy only.
    ``extras``: further per-frame metrics by name ({'vgg_cos': [S, N, T], 'vgg_l1': [S, N, T]}), summarised like the three (the names in
    LOWER_IS_BETTER pick their lowest draw) and counted in n_nonfinite; without them the result is that of the three alone.
    ``motion`` (--motion-metrics): {'kp_l2': [S, N, T]}, summarised and counted like the others with the lowest draw as best, and for two or
    more draws {'kp_div': [S, T], 'div_mse': [S, T]}, which have no draw axis: mean and per_frame only, non-finite values null."""
    arrs = {'ssim': np.asarray(ssim, np.float64), 'psnr': np.asarray(psnr, np.float64), 'mse': np.asarray(mse, np.float64)}
    for name, x in (extras or {}).items():
        if name in arrs:
            raise ValueError('summarise_metrics: extras may not replace %r' % name)
        arrs[name] = np.asarray(x, np.float64)
    per_sample = {}
    if motion is not None:
        if 'kp_l2' not in motion or set(motion) - {'kp_l2', 'kp_div', 'div_mse'} or 'kp_l2' in arrs:
            raise ValueError('summarise_metrics: motion holds kp_l2 and optionally kp_div and div_mse (got %s)' % sorted(motion))
        arrs['kp_l2'] = np.asarray(motion['kp_l2'], np.float64)
        per_sample = {name: np.asarray(motion[name], np.float64) for name in ('kp_div', 'div_mse') if name in motion}
    shape = arrs['ssim'].shape
    if len(shape) != 3 or any(a.shape != shape for a in arrs.values()):
        raise ValueError('summarise_metrics: %s must share one [S, N, T] shape (got %s)'
                         % (', '.join(arrs) if extras or motion else 'ssim, psnr and mse', [a.shape for a in arrs.values()]))
    s, n, t = shape
    if any(a.shape != (s, t) for a in per_sample.values()):
        raise ValueError('summarise_metrics: kp_div and div_mse must be [S, T] = %s (got %s)' % ([s, t], [a.shape for a in per_sample.values()]))
    bad = ~np.logical_and.reduce([np.isfinite(a) for a in arrs.values()])
    out = {'definition': METRICS_DEFINITION, 'n_samples': s, 'n_draws': n, 'n_nonfinite': int(bad.sum())}
    if extras:
        out['definition'] = METRICS_DEFINITION + ' ' + VGG_METRICS_DEFINITION
        out['vgg_layers'] = list(VGG_FEATURE_LAYERS)
    if motion is not None:
        out['definition'] += ' ' + MOTION_METRICS_DEFINITION
    for name, x in arrs.items():
        lower_is_better = name in LOWER_IS_BETTER
        with np.errstate(invalid='ignore'):
            draw_mean = x.mean(axis=2)                                           # [S, N]
            key = np.where(np.isnan(draw_mean), np.inf if lower_is_better else -np.inf, draw_mean)
            best = np.argmin(key, axis=1) if lower_is_better else np.argmax(key, axis=1)   # first extreme: ties go to the lowest draw
            best_frames = x[np.arange(s), best]                                  # [S, T]
            out[name] = {'mean': _json_num(x.mean()), 'per_frame': [_json_num(v) for v in x.mean(axis=(0, 1))],
                         'best_of_draws': _json_num(best_frames.mean()),
                         'best_of_draws_per_frame': [_json_num(v) for v in best_frames.mean(axis=0)],
                         'best_draw': [int(i) for i in best]}
    for name, x in per_sample.items():
        with np.errstate(invalid='ignore'):
            out[name] = {'mean': _json_num(x.mean()), 'per_frame': [_json_num(v) for v in x.mean(axis=0)]}
    return out


FRECHET_DEFINITION = (
    'frechet: Frechet distance |m1 - m2|^2 + tr C1 + tr C2 - 2 tr (C1 C2)^(1/2) between the Gaussians fitted to two sets of feature vectors '
    'of the same VGG19 and 8-bit frames as vgg_cos, per layer of vgg_layers; vgg_fd / vgg_fvd are the values of conv5_4. This is the '
    'project\'s own VGG19 quantity: not FID/FVD (those use Inception / I3D features) and not comparable with published figures. Frame level '
    '(fd): one vector per frame, the mean of the layer\'s features over positions (D = C). Video level (fvd): one vector per rollout of T '
    'frames, concat(mean_t p_t, mean_t |p_(t+1) - p_t|) of its pooled frames p (D = 2 C; the second half is 0 for a frozen pose). Pooling '
    'and the first and second moments are accumulated in float64 on the device over the whole test set; cov = (sum x x^T - n mu mu^T) / '
    '(n - 1). fd, fvd: the predictions of all draws of z against all real frames; fd_draw0: draw 0 (the written PNGs) alone; fd_floor, '
    'fvd_floor: the real even-numbered samples against the real odd-numbered ones, the finite-sample noise floor that gives the others a '
    'scale. A value is null where a set has fewer than two rows; rank_deficient marks layers where a set has n <= D rows, whose covariance '
    'is singular and whose distance is a lower-quality estimate. The distance is not clamped at 0.')


def summarise_frechet(stats):
    """-> (the vgg_f*_layers arrays of metrics.npz, each float64 [layers], the ``frechet`` block of metrics.json); numpy only.  stats: the
    ``FrechetAccumulator.stats()`` of the sets 'real', 'pred', 'pred_draw0', 'real_even' and 'real_odd'."""
    from kpx_amd import frechet as F
    pairs = {'vgg_fd_layers': ('pred', 'real', 'frame'), 'vgg_fvd_layers': ('pred', 'real', 'video'),
             'vgg_fd_draw0_layers': ('pred_draw0', 'real', 'frame'),
             'vgg_fd_floor_layers': ('real_even', 'real_odd', 'frame'), 'vgg_fvd_floor_layers': ('real_even', 'real_odd', 'video')}
    arrays = {name: F.layer_distances(stats[a], stats[b], level) for name, (a, b, level) in pairs.items()}
    nums = lambda x: [_json_num(v) for v in x]
    dims = {level: [s['mean'].size if s['mean'] is not None else None for s in stats['real'][level]] for level in F.LEVELS}
    count = lambda name, level: int(stats[name][level][0]['n']) if stats[name][level] else 0
    head = len(arrays['vgg_fd_layers']) - 1                                      # conv5_4, the last layer of VGG_FEATURE_LAYERS
    block = {'definition': FRECHET_DEFINITION, 'vgg_layers': list(VGG_FEATURE_LAYERS),
             'vgg_fd': _json_num(arrays['vgg_fd_layers'][head]), 'vgg_fvd': _json_num(arrays['vgg_fvd_layers'][head]),
             'n_real': count('real', 'frame'), 'n_pred': count('pred', 'frame'),
             'n_real_videos': count('real', 'video'), 'n_pred_videos': count('pred', 'video'), 'dims': dims,
             'rank_deficient': {level: [d is None or min(count('real', level), count('pred', level)) <= d for d in dims[level]]
                                for level in F.LEVELS}}
    for name, x in arrays.items():
        block[name] = nums(x)
    return arrays, block


ACTIONS_DEFINITION = (
    'actions: every source image rolled out under each listed action class at the same z (one z per batch and draw, shared with the '
    'batch\'s own rollout). kp_l2: per class, draw and frame the key-point error of --motion-metrics against the pseudo labels of the real '
    'frames. score[s, a] = mean of kp_l2 over draws and frames (non-finite: +inf). A sample is ranked if its own class (the argmax of its '
    'action code) is listed; its rank is the number of OTHER listed classes with score <= the score of the own class, so ties count against '
    'the model: one that ignores the class has rank A - 1 and top1 0. top1 = share of ranked samples with rank 0, chance = 1 / A, '
    'mean_rank over ranked samples, confusion[i][j] = ranked samples whose own class is actions[i] and whose lowest score is at actions[j] '
    '(a tie goes to the lowest j). kp_div and div_mse (two or more classes): per draw the kp_div and div_mse of --motion-metrics with the '
    'classes in the place of the draws; a model that ignores the class scores 0 in both. A network-free stand-in for action-recognition '
    'accuracy, not that figure.')
SHEET_FRAMES_DEFAULT = (3, 7, 11, 15, 19, 23, 27, 31)
N_FUTURE_FRAMES = 32                                                              # = kpx_amd.final_model.N_FUTURE_FRAMES


def action_ranks(actions, act_own, act_kp_l2):
    """-> (score float64 [S, A], rank int32 [S]) of ACTIONS_DEFINITION from act_kp_l2 [S, A, D, T]; rank -1 where the own class is not listed."""
    actions = [int(a) for a in actions]
    own = np.asarray(act_own).reshape(-1).astype(np.int64)
    l2 = np.asarray(act_kp_l2, np.float64)
    if l2.ndim != 4 or l2.shape[:2] != (own.size, len(actions)) or not actions:
        raise ValueError('action_ranks: act_kp_l2 must be [S, A, D, T] for S = %d samples and A = %d classes (got %s)'
                         % (own.size, len(actions), l2.shape))
    with np.errstate(invalid='ignore', over='ignore'):
        score = l2.reshape(own.size, len(actions), -1).mean(axis=2) if l2.shape[2] * l2.shape[3] else np.full(l2.shape[:2], np.inf)
    score = np.where(np.isfinite(score), score, np.inf)
    rank = np.full(own.size, -1, np.int32)
    for s in range(own.size):
        if int(own[s]) in actions:
            i = actions.index(int(own[s]))
            rank[s] = int((score[s] <= score[s, i]).sum()) - 1
    return score, rank


def summarise_actions(actions, act_own, act_kp_l2, act_kp_div=None, act_div_mse=None):
    """The ``actions`` block of metrics.json (ACTIONS_DEFINITION) from the arrays of metrics.npz: actions [A], act_own [S], act_kp_l2
    [S, A, D, T] and, for two or more classes, act_kp_div and act_div_mse [S, D, T]; numpy only."""
    actions = [int(a) for a in actions]
    score, rank = action_ranks(actions, act_own, act_kp_l2)
    own = np.asarray(act_own).reshape(-1).astype(np.int64)
    ranked = rank >= 0
    n_ranked, n_cls = int(ranked.sum()), len(actions)
    confusion = [[0] * n_cls for _ in range(n_cls)]
    for s in np.nonzero(ranked)[0]:
        confusion[actions.index(int(own[s]))][int(np.argmin(score[s]))] += 1      # first minimum: a tie goes to the lowest list position
    out = {'definition': ACTIONS_DEFINITION, 'actions': actions, 'n_ranked': n_ranked, 'chance': 1.0 / n_cls,
           'top1': float((rank[ranked] == 0).mean()) if n_ranked else None,
           'mean_rank': float(rank[ranked].astype(np.float64).mean()) if n_ranked else None, 'confusion': confusion}
    parts = {'kp_l2': act_kp_l2}
    if n_cls >= 2:
        if act_kp_div is None or act_div_mse is None:
            raise ValueError('summarise_actions: two or more classes come with act_kp_div and act_div_mse')
        parts.update(kp_div=act_kp_div, div_mse=act_div_mse)
    for name, x in parts.items():
        x = np.asarray(x, np.float64)
        x = x.reshape(-1, x.shape[-1])
        with np.errstate(invalid='ignore', over='ignore'):
            out[name] = {'mean': _json_num(x.mean()) if x.size else None,
                         'per_frame': [_json_num(v) for v in x.mean(axis=0)] if x.shape[0] else [None] * x.shape[1]}
    return out


ACTION_ACCURACY_DEFINITION = (
    'action_accuracy: a recogniser trained by this project (train.py --mode action_classifier: stacked LSTM over the 32 key-point sets of '
    'a sequence, softmax over the A classes, trained on the pseudo labels) classifies key-point sequences. real: the pseudo labels of the '
    'real frames against the sample\'s own class, the ceiling. pred: the predicted key points of every draw of z against the sample\'s own '
    'class. commanded (with --actions): the rollout under each listed class at the shared z against the class that was commanded. Per '
    'sequence: pred = the lowest index among the maxima of its logits; rank = 1 + the number of OTHER classes whose logit is >= the '
    'target\'s, so a tie counts against the model; logp = the log-softmax at the target. A sequence with a non-finite logit has pred -1, '
    'rank A and logp NaN: it counts as wrong in top1 and mean_rank, is counted in n_nonfinite and is left out of nll and confusion. '
    'top1 = share with rank 1, chance = 1 / A, mean_rank, nll = -mean logp over the finite sequences, per_class_top1[c] = top1 of the '
    'sequences whose target is c (null for a class without one), confusion[t][p] = finite sequences with target t and pred p, '
    'best_of_draws_top1 = share of samples (commanded: of sample-class pairs) with rank 1 in at least one draw. kp_fd: the Frechet distance '
    '|m1 - m2|^2 + tr C1 + tr C2 - 2 tr (C1 C2)^(1/2) between the Gaussians fitted to the recogniser\'s features (its top LSTM layer at the '
    'last step, dimension dim) of all real sequences and of the predictions of all draws; kp_fd_draw0: draw 0 alone; kp_fd_floor: the real '
    'even-numbered samples against the odd-numbered ones, the finite-sample noise floor; null where a set has fewer than two rows, '
    'rank_deficient where a set has n <= dim rows; moments in float64, cov = (sum x x^T - n mu mu^T) / (n - 1), not clamped at 0. '
    'This is the project\'s own key-point-space quantity, computed by a recogniser that never sees a pixel and is trained on this '
    'project\'s pseudo labels: it is not comparable with published action-recognition accuracies or FVD figures.')


def summarise_action_accuracy(arrays):
    """The ``action_accuracy`` block of metrics.json (ACTION_ACCURACY_DEFINITION) from the arrays --action-accuracy puts into metrics.npz:
    cls_own [S], cls_real_{pred,rank,logp} [S], cls_pred_{pred,rank,logp} [S, D], cls_confusion_{real,pred} [A, A], kp_fd, kp_fd_draw0,
    kp_fd_floor, kp_fd_dim and, with --actions, actions [C], cls_act_{pred,rank,logp} [S, C, D] and cls_confusion_commanded; numpy only."""
    own = np.asarray(arrays['cls_own']).reshape(-1).astype(np.int64)
    n_cls = int(np.asarray(arrays['cls_confusion_real']).shape[0])
    s = own.size

    def block(prefix, target, confusion, draws_axis):
        pred, rank = np.asarray(arrays[prefix + 'pred']).astype(np.int64), np.asarray(arrays[prefix + 'rank']).astype(np.int64)
        logp = np.asarray(arrays[prefix + 'logp'], np.float64)
        if pred.shape != target.shape or rank.shape != target.shape or logp.shape != target.shape:
            raise ValueError('summarise_action_accuracy: %spred, rank and logp must be %s (got %s, %s, %s)'
                             % (prefix, list(target.shape), pred.shape, rank.shape, logp.shape))
        hit, finite = rank == 1, pred >= 0
        out = {'n': int(rank.size), 'chance': 1.0 / n_cls, 'top1': float(hit.mean()) if rank.size else None,
               'mean_rank': float(rank.astype(np.float64).mean()) if rank.size else None,
               'nll': _json_num(-logp[finite].mean()) if finite.any() else None,
               'per_class_top1': [float(hit[target == c].mean()) if (target == c).any() else None for c in range(n_cls)],
               'confusion': [[int(v) for v in row] for row in np.asarray(confusion)], 'n_nonfinite': int((~finite).sum())}
        if draws_axis is not None:
            any_hit = hit.any(axis=draws_axis)
            out['best_of_draws_top1'] = float(any_hit.mean()) if any_hit.size else None
        return out

    d = int(np.asarray(arrays['cls_pred_rank']).shape[1]) if np.asarray(arrays['cls_pred_rank']).ndim == 2 else 0
    res = {'definition': ACTION_ACCURACY_DEFINITION, 'n_samples': s, 'n_draws': d, 'n_classes': n_cls,
           'real': block('cls_real_', own, arrays['cls_confusion_real'], None),
           'pred': block('cls_pred_', np.broadcast_to(own[:, None], (s, d)), arrays['cls_confusion_pred'], 1)}
    if 'cls_act_rank' in arrays:
        actions = np.asarray(arrays['actions']).reshape(-1).astype(np.int64)
        shape = np.asarray(arrays['cls_act_rank']).shape
        res['actions'] = [int(a) for a in actions]
        res['commanded'] = block('cls_act_', np.broadcast_to(actions[None, :, None], shape), arrays['cls_confusion_commanded'], 2)
    dim = int(arrays['kp_fd_dim'])
    n_sets = {'kp_fd': (s, s * d), 'kp_fd_draw0': (s, s if d else 0), 'kp_fd_floor': ((s + 1) // 2, s // 2)}
    res['kp_fd'] = {'dim': dim, 'n_real': s, 'n_pred': s * d}
    for name, counts in n_sets.items():
        res['kp_fd'][name] = _json_num(arrays[name])
    res['kp_fd']['rank_deficient'] = {name: min(counts) <= dim for name, counts in n_sets.items()}
    return res


class _ActionAccuracy:
    """--action-accuracy: the recogniser, its scores per batch (device tensors until the end) and the moments of its features."""
    SETS = ('real_even', 'real_odd', 'pred', 'pred_draw0')

    def __init__(self, kpx_amd, config, checkpoint, dev, samples, actions, ema=False):
        self.ops, self.F, self.dev, self.samples, self.actions = kpx_amd.ops, kpx_amd.frechet, dev, samples, actions
        self.model = kpx_amd.ActionClassifierModel(config, is_training=False, device=dev)
        self.model.build(None)
        self.model.restore(None, checkpoint, strict=True, **({'ema': True} if ema else {}))
        a, u = self.model.n_action, self.model.cells[-1]
        self.n_action, self.dim = a, u
        zi = lambda: torch.zeros((a, a), dtype=torch.int32, device=dev)
        self.confusion = {'real': zi(), 'pred': zi()}
        if actions:
            self.confusion['commanded'] = zi()
            self.commanded = [torch.full((1,), c, dtype=torch.int32, device=dev) for c in actions]
        self.moments = {name: {'n': 0, 'sum': torch.zeros(u, dtype=torch.float64, device=dev),
                               'outer': torch.zeros((u, u), dtype=torch.float64, device=dev)} for name in self.SETS}
        self.own, self.real, self.pred, self.act = [], [], [], []
        self.n_scored = 0
        self.on_feats = None                         # --prdc: called with (kind, draw, class index, fp32 features) of every classify call made here

    def _add(self, name, rows):
        if rows.shape[0]:
            m = self.moments[name]
            self.ops.moments_add(rows.contiguous(), m['sum'], m['outer'])
            m['n'] += int(rows.shape[0])

    def begin_batch(self, batch):
        """The real key points of a batch against its own classes; the targets every draw of this batch is scored against."""
        bsz = batch['real_seq'].shape[0]
        self.target = batch['action_code'].argmax(dim=1).to(torch.int32).contiguous()
        self.own.append(self.target)
        logits, feats = self.model.classify(batch['real_seq'])
        self.real.append(self.ops.class_scores(logits, self.target, self.confusion['real'], check_target=False))
        if self.on_feats is not None:
            self.on_feats('real', None, None, feats)
        feats = feats.double()
        first = self.n_scored % 2                    # the parity of this batch's first sample among all samples
        self._add('real_even', feats[first::2])
        self._add('real_odd', feats[1 - first::2])
        self.n_scored += bsz
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.dev)
        self.pred.append(tuple(mk((self.samples, bsz), dt) for dt in (torch.int32, torch.int32, torch.float32)))
        if self.actions:
            self.act.append(tuple(mk((self.samples, len(self.actions), bsz), dt) for dt in (torch.int32, torch.int32, torch.float32)))

    def own_draw(self, draw, fut_pt_raw):
        """One draw of the batch's own rollout, enqueued before the next run() replays the graph over ``fut_pt_raw``."""
        logits, feats = self.model.classify(fut_pt_raw)
        self.ops.class_scores(logits, self.target, self.confusion['pred'], out=tuple(t[draw] for t in self.pred[-1]), check_target=False)
        if self.on_feats is not None:
            self.on_feats('fake', draw, None, feats)
        feats = feats.double()
        self._add('pred', feats)
        if draw == 0:
            self._add('pred_draw0', feats)

    def class_rollout(self, draw, a, fut_pt_raw):
        """The rollout under the listed class ``a`` at this draw's z, against the class that was commanded."""
        logits, feats = self.model.classify(fut_pt_raw)
        if self.on_feats is not None:
            self.on_feats('commanded', draw, a, feats)
        target = self.commanded[a].expand(logits.shape[0]).contiguous()
        self.ops.class_scores(logits, target, self.confusion['commanded'], out=tuple(t[draw, a] for t in self.act[-1]), check_target=False)

    def arrays(self):
        """-> the cls_* and kp_fd* arrays of metrics.npz (one copy to the host per kind)"""
        host = lambda ts, shape, dt, dim=0: torch.cat(ts, dim=dim).cpu().numpy() if ts else np.zeros(shape, dt)
        kinds = (('pred', np.int32), ('rank', np.int32), ('logp', np.float32))
        d, c = self.samples, len(self.actions or ())
        out = {'cls_own': host(self.own, (0,), np.int32)}
        for i, (name, dt) in enumerate(kinds):
            out['cls_real_' + name] = host([r[i] for r in self.real], (0,), dt)
            out['cls_pred_' + name] = np.ascontiguousarray(host([r[i] for r in self.pred], (d, 0), dt, 1).T)                        # [S, D]
            if self.actions:
                out['cls_act_' + name] = np.ascontiguousarray(host([r[i] for r in self.act], (d, c, 0), dt, 2).transpose(2, 1, 0))   # [S, C, D]
        for name, t in self.confusion.items():
            out['cls_confusion_' + name] = t.cpu().numpy()
        st = {name: self.F.stats_from_moments(m['n'], m['sum'].cpu().numpy(), m['outer'].cpu().numpy()) for name, m in self.moments.items()}
        even, odd = self.moments['real_even'], self.moments['real_odd']
        st['real'] = self.F.stats_from_moments(even['n'] + odd['n'], (even['sum'] + odd['sum']).cpu().numpy(),
                                               (even['outer'] + odd['outer']).cpu().numpy())
        fd = lambda x, y: np.float64(self.F.frechet_distance(st[x]['mean'], st[x]['cov'], st[y]['mean'], st[y]['cov']))
        out.update(kp_fd=fd('pred', 'real'), kp_fd_draw0=fd('pred_draw0', 'real'), kp_fd_floor=fd('real_even', 'real_odd'),
                   kp_fd_dim=np.int32(self.dim))
        return out


NOVELTY_DEFINITION = (
    'novelty: this project\'s own key-point-space quantity, not comparable with published figures. Candidates: every sequence the stage-2 '
    'loader can draw from train_set.txt without augmentation (per listing line every legal start frame at the video\'s own gap = '
    'int(n_files / 33), the interpolated form for videos shorter than 33 frames) and, when mirror is true, its mirror image (x negated). '
    'd2(query, candidate) = the mean over the 32 frames and K points of the squared Euclidean distance in label coordinates, in fp64; a '
    'query is every draw\'s predicted key points (pred), the pseudo labels of the real future frames (real) and with --actions every class '
    'rollout (commanded); the candidates of the query\'s own source video are left out. d = sqrt of the minimum of d2 over all candidates: '
    'an RMS point distance; ties go to the lowest code = 2 * window + mirrored. pred and real: mean, median and p05 (the 5th percentile, '
    'linear interpolation) of d over the queries that found a candidate. ratio = median pred / median real: near 1 the rollouts lie as far '
    'from the training set as fresh real motion does, well below 1 they replay it. copy_threshold = p05 of real, null below 20 real '
    'queries; copied = the share of pred queries with d below it. nn_top1: the share of queries whose nearest candidate was listed under '
    'the query\'s class (real: the sample\'s class, the ceiling; pred: the sample\'s class; commanded: the commanded class), chance = 1 / '
    'the number of classes with a candidate. mirrored = the share of pred queries whose nearest candidate is a mirror image. n_nonfinite: '
    'queries that found no candidate (a non-finite key point, or no candidate left); they enter no other figure.')


def nearest_over_classes(d2, code):
    """d2 float64 [..., A], code int [..., A] per class -> (d2 [...], code [...]) of the minimum over the classes, ties to the lowest code;
    +inf and -1 where no class found a candidate.  numpy only."""
    d2, code = np.asarray(d2, np.float64), np.asarray(code, np.int64)
    low = d2.min(axis=-1) if d2.shape[-1] else np.full(d2.shape[:-1], np.inf)
    at = (d2 == low[..., None]) & (code >= 0)
    best = np.where(at, code, np.iinfo(np.int64).max).min(axis=-1) if d2.shape[-1] else np.full(d2.shape[:-1], -1, np.int64)
    found = at.any(axis=-1) & np.isfinite(low)
    return np.where(found, low, np.inf), np.where(found, best, -1).astype(np.int32)


def summarise_novelty(arrays, mirror=True):
    """The ``novelty`` block of metrics.json (NOVELTY_DEFINITION) from the arrays --novelty puts into metrics.npz: nov_d / nov_code [S, D],
    nov_real_d / nov_real_code [S], nov_own [S], nov_window_action [W] and optionally actions [C] with act_nov_d / act_nov_code [S, C, D].
    numpy only."""
    win_action = np.asarray(arrays['nov_window_action'], np.int64)
    own = np.asarray(arrays['nov_own'], np.int64)
    n_cls = len(np.unique(win_action))
    n_bad = [0]

    def found(d, code):
        d, code = np.asarray(d, np.float64), np.asarray(code, np.int64)
        ok = (code >= 0) & np.isfinite(d)
        n_bad[0] += int((~ok).sum())
        return d, code, ok

    def stats(x):
        if not x.size:
            return {'mean': None, 'median': None, 'p05': None}
        return {'mean': _json_num(x.mean()), 'median': _json_num(np.median(x)), 'p05': _json_num(np.percentile(x, 5))}

    def top1(code, ok, target):
        hit = win_action[np.where(ok, code >> 1, 0)] == target
        return _json_num(hit[ok].mean()) if ok.any() else None

    pd, pc, pok = found(arrays['nov_d'], arrays['nov_code'])
    rd, rc, rok = found(arrays['nov_real_d'], arrays['nov_real_code'])
    out = {'definition': NOVELTY_DEFINITION, 'mirror': bool(mirror), 'n_windows': int(win_action.size), 'n_pred': int(pok.sum()),
           'n_real': int(rok.sum()), 'pred': stats(pd[pok]), 'real': stats(rd[rok])}
    pm, rm = out['pred']['median'], out['real']['median']
    out['ratio'] = _json_num(pm / rm) if pm is not None and rm else None
    out['copy_threshold'] = out['real']['p05'] if rok.sum() >= 20 else None
    out['copied'] = _json_num((pd[pok] < out['copy_threshold']).mean()) if out['copy_threshold'] is not None and pok.any() else None
    out['nn_top1'] = {'chance': 1.0 / n_cls if n_cls else None, 'real': top1(rc, rok, own), 'pred': top1(pc, pok, own[:, None])}
    if 'act_nov_code' in arrays:
        ad, ac, aok = found(arrays['act_nov_d'], arrays['act_nov_code'])
        out['nn_top1']['commanded'] = top1(ac, aok, np.asarray(arrays['actions'], np.int64)[None, :, None])
    out['mirrored'] = _json_num((pc[pok] & 1).mean()) if pok.any() else None
    out['n_nonfinite'] = n_bad[0]
    return out


class _Novelty:
    """--novelty: the store of training motions, the queries of a batch and their search; the results stay on the device until the end."""

    def __init__(self, kpx_amd, config, dev, samples, actions, mirror, sheet_frames, colors):
        data_dir = config['paths']['data_dir']
        with open(osp.join(data_dir, 'train_set.txt')) as f:
            listing = f.read().splitlines()
        self.ops, self.dev, self.samples, self.actions, self.mirror = kpx_amd.ops, dev, samples, actions or [], mirror
        self.store = kpx_amd.novelty.MotionStore(data_dir, listing, config['model']['n_pts'], config['model']['n_action'], dev)
        self.sheet_frames = sheet_frames
        self.colors = torch.tensor(colors, dtype=torch.float32, device=dev) if sheet_frames is not None else None
        self.d2, self.code, self.own = [], [], []

    def begin_batch(self, videos, batch):
        """Slot 0 of the batch's queries holds the real future; 1 .. samples the draws; then draw-major the class rollouts."""
        kp_real = batch['real_seq'].contiguous()
        self.bsz = kp_real.shape[0]
        n = 1 + self.samples * (1 + len(self.actions))
        self.queries = torch.empty((n,) + tuple(kp_real.shape), dtype=torch.float32, device=self.dev)
        self.ops.flat_copy_tensor(kp_real, self.queries[0].data_ptr())
        self.exclude = torch.tensor([self.store.video(v) for v in videos], dtype=torch.int32, device=self.dev).repeat(n)
        self.own.append(batch['action_code'].argmax(dim=1).to(torch.int32))

    def own_draw(self, draw, fut_pt_raw):
        self.ops.flat_copy_tensor(fut_pt_raw.contiguous(), self.queries[1 + draw].data_ptr())

    def class_rollout(self, draw, a, fut_pt_raw):
        self.ops.flat_copy_tensor(fut_pt_raw.contiguous(), self.queries[1 + self.samples + draw * len(self.actions) + a].data_ptr())

    def end_batch(self, save_dir, first_sample):
        q = self.queries.view((-1,) + tuple(self.queries.shape[2:]))
        d2, code = self.store.nearest(q, self.mirror, self.exclude)
        self.d2.append(d2.view(self.queries.shape[0], self.bsz, -1))
        self.code.append(code.view(self.queries.shape[0], self.bsz, -1))
        if self.sheet_frames is not None:
            self._write_sheets(save_dir, first_sample)

    def _write_sheets(self, save_dir, first_sample):
        from PIL import Image
        ops, frames, b, d = self.ops, self.sheet_frames, self.bsz, self.samples
        _, code = nearest_over_classes(self.d2[-1][1:1 + d].cpu().numpy(), self.code[-1][1:1 + d].cpu().numpy())       # [D, B]
        h = w = 128
        canvas = torch.zeros((b, (1 + 2 * d) * h, len(frames) * w, 3), dtype=torch.uint8, device=self.dev)

        def paste(row, seq, keep=None):
            pts = seq[:, frames].contiguous()                                                             # [n, J, K, 2]
            maps = ops.point_maps_rgb(pts.view((-1,) + tuple(pts.shape[2:])), h, w, self.colors).view(pts.shape[0], len(frames), h, w, 3)
            if keep is None:
                ops.sheet_paste(canvas, maps, list(range(len(frames))), row, 0, 'raw')
            else:                            # the samples that found a window, one by one; the others keep their black row
                for i, j in enumerate(keep):
                    ops.sheet_paste(canvas[j:j + 1], maps[i:i + 1].contiguous(), list(range(len(frames))), row, 0, 'raw')
        paste(0, self.queries[0])
        for draw in range(d):
            paste(1 + 2 * draw, self.queries[1 + draw])
            keep = [j for j in range(b) if code[draw, j] >= 0]
            if keep:
                paste(2 + 2 * draw, self.store.gather(code[draw, keep]), keep)
        host = _sheet_to_host(canvas)
        for batch_idx in range(b):
            dd = osp.join(save_dir, '%04d' % (first_sample + batch_idx))
            os.makedirs(dd, exist_ok=True)
            Image.fromarray(host[batch_idx]).save(osp.join(dd, 'nearest.png'))

    def arrays(self):
        """-> the nov_* arrays of metrics.npz (one copy to the host per kind)"""
        d, c, a = self.samples, len(self.actions), self.store.n_action
        cat = lambda ts, dt: torch.cat(ts, dim=1).cpu().numpy() if ts else np.zeros((1 + d * (1 + c), 0, a), dt)
        d2, code = cat(self.d2, np.float64), cat(self.code, np.int32)                                   # [1 + D + D C, S, A]
        win = self.store.windows
        out = {'nov_own': torch.cat(self.own).cpu().numpy() if self.own else np.zeros((0,), np.int32), 'nov_window_action': win.table[:, 3].copy()}
        low, best = nearest_over_classes(d2, code)
        out.update(nov_real_d=np.sqrt(low[0]), nov_real_code=best[0], nov_real_class_d=np.sqrt(d2[0]), nov_real_window=win.describe(best[0]),
                   nov_d=np.ascontiguousarray(np.sqrt(low[1:1 + d]).T), nov_code=np.ascontiguousarray(best[1:1 + d].T),
                   nov_class_d=np.ascontiguousarray(np.sqrt(d2[1:1 + d]).transpose(1, 0, 2)))
        out['nov_window'] = win.describe(out['nov_code'])
        if c:
            s = low.shape[1]
            out['act_nov_d'] = np.ascontiguousarray(np.sqrt(low[1 + d:]).reshape(d, c, s).transpose(2, 1, 0))
            out['act_nov_code'] = np.ascontiguousarray(best[1 + d:].reshape(d, c, s).transpose(2, 1, 0))
        return out


class _Prdc:
    """--prdc: the real and the generated rows of the run in key-point space and, with --action-accuracy, in the recogniser's feature space
    (its classify calls are reused through ``_ActionAccuracy.on_feats``); float32 on the device until the end, scored once."""

    def __init__(self, kpx_amd, dev, samples, actions, k, accuracy):
        self.P, self.dev, self.samples, self.actions, self.k = kpx_amd.prdc, dev, samples, actions or [], k
        self.spaces = ['kp'] + (['cls'] if accuracy is not None else [])
        self.real = {sp: [] for sp in self.spaces}
        self.fake = {sp: [[] for _ in range(samples)] for sp in self.spaces}
        self.commanded = {sp: [[] for _ in self.actions] for sp in self.spaces}
        self.own = []
        if accuracy is not None:
            accuracy.on_feats = self._feats

    @staticmethod
    def _rows(t):
        return t.reshape(t.shape[0], -1).to(torch.float32).clone()        # a copy: the rollout's buffers are overwritten by the next replay

    def _add(self, sp, kind, draw, a, t):
        if kind == 'real':
            self.real[sp].append(self._rows(t))
        elif kind == 'fake':
            self.fake[sp][draw].append(self._rows(t))
        elif draw == 0:                              # commanded: the draw-0 rollouts under the listed class a
            self.commanded[sp][a].append(self._rows(t))

    def _feats(self, kind, draw, a, feats):
        self._add('cls', kind, draw, a, feats)

    def begin_batch(self, batch):
        self._add('kp', 'real', None, None, batch['real_seq'])
        self.own.append(batch['action_code'].argmax(dim=1).to(torch.int32))

    def own_draw(self, draw, fut_pt_raw):
        self._add('kp', 'fake', draw, None, fut_pt_raw)

    def class_rollout(self, draw, a, fut_pt_raw):
        self._add('kp', 'commanded', draw, a, fut_pt_raw)

    def arrays(self, save_dir):
        """-> the prdc_* arrays of metrics.npz; writes <save_dir>/prdc.npz (the rows as the float32 they were born as, classes, parities)"""
        if not self.own:
            return {'prdc_k': np.int32(self.k)}
        own = torch.cat(self.own)
        rows = {'own': own, 'parity': (torch.arange(own.shape[0], device=self.dev) % 2).to(torch.int32)}
        for sp in self.spaces:
            rows[sp + '_real'] = torch.cat(self.real[sp])
            rows[sp + '_fake'] = torch.stack([torch.cat(per_draw) for per_draw in self.fake[sp]])
            if self.actions:
                rows[sp + '_commanded'] = torch.stack([torch.cat(per_class) for per_class in self.commanded[sp]])
        stored = {key: v.cpu().numpy() for key, v in rows.items()}
        stored['k'] = np.int32(self.k)
        store = {key: v.double() if v.dtype == torch.float32 else v for key, v in rows.items()}       # to fp64 once
        if self.actions:
            stored['actions'] = store['actions'] = np.asarray(self.actions, np.int32)
        os.makedirs(save_dir, exist_ok=True)
        np.savez(osp.join(save_dir, 'prdc.npz'), **stored)
        return self.P.score_store(store, self.k, self.P.prdc)


DRIVE_MODES = ('labels', 'hold', 'transfer')                                      # the order of the runs and of the sheet's rows
DRIVE_METRICS = ('ssim', 'psnr', 'mse')
DRIVE_DEFINITION = (
    'drive: the translator rolled out on key points that do not come from the motion generator; no z is drawn. labels: the 32 key-point '
    'frames are the pseudo labels of the real frames, that is, the output of this project\'s own key-point detector on the real frames, not '
    'human annotations: what the translator reaches when it is handed the true motion (a ceiling). hold: the detected key points of the '
    'input image at all 32 frames: what it reaches when the pose never moves (a floor). Both are scored against the real frames exactly as '
    'the model\'s own frames are (the 8-bit SSIM, PSNR and MSE above), once per sample: mean over samples and frames, per_frame over '
    'samples. skill = (model - hold) / (labels - hold) on the means of a metric, the model\'s mean taken over samples, draws and frames: '
    '0 is the static pose, 1 the true motion; it is null when the denominator is 0 or any of the three means is non-finite, and absent '
    'unless labels, hold and the model\'s own rollout were all scored. transfer (the detected key points moved as the next sample of the '
    'batch moves; with scaled, that motion times sqrt(v_src / v_drv), v the summed squared distance of a frame-0 constellation to its '
    'mean) has no ground truth and is not scored.')


def summarise_drive(drive, model=None):
    """The ``drive`` block of metrics.json (DRIVE_DEFINITION); numpy only.  drive: {'labels' and / or 'hold': {'ssim', 'psnr', 'mse': [S, T]}};
    model: the model's own {'ssim', 'psnr', 'mse': [S, N, T]}, or None when it was not rolled out (--drive-only)."""
    if not drive or set(drive) - {'labels', 'hold'}:
        raise ValueError('summarise_drive: scores of labels and / or hold (got %s)' % sorted(drive or ()))
    out = {'definition': DRIVE_DEFINITION, 'modes': [m for m in DRIVE_MODES if m in drive]}
    shape = None
    for mode in out['modes']:
        if set(drive[mode]) != set(DRIVE_METRICS):
            raise ValueError('summarise_drive: %s holds ssim, psnr and mse (got %s)' % (mode, sorted(drive[mode])))
        out[mode] = {}
        for name in DRIVE_METRICS:
            x = np.asarray(drive[mode][name], np.float64)
            shape = x.shape if shape is None else shape
            if x.ndim != 2 or x.shape != shape:
                raise ValueError('summarise_drive: every array is [S, T] of one shape (got %s and %s)' % (shape, x.shape))
            with np.errstate(invalid='ignore', over='ignore'):
                out[mode][name] = {'mean': _json_num(x.mean()) if x.size else None,
                                   'per_frame': [_json_num(v) for v in x.mean(axis=0)] if x.shape[0] else [None] * x.shape[1]}
    if model is not None and 'labels' in drive and 'hold' in drive:
        out['skill'] = {}
        for name in DRIVE_METRICS:
            own = np.asarray(model[name], np.float64)
            with np.errstate(invalid='ignore', over='ignore'):
                m = own.mean() if own.size else np.nan
                top, floor = out['labels'][name]['mean'], out['hold'][name]['mean']
                ok = top is not None and floor is not None and np.isfinite(m) and top != floor
                out['skill'][name] = _json_num((m - floor) / (top - floor)) if ok else None
    return out


def _parse_index_list(text, what, limit):
    """'i,j,k' -> [i, j, k], distinct and in [0, limit); a ValueError names what is wrong"""
    try:
        idx = [int(v) for v in text.split(',')] if text.strip() else []
    except ValueError:
        raise ValueError('%s takes integers separated by commas (got %r)' % (what, text))
    if not idx:
        raise ValueError('%s lists nothing' % what)
    if len(set(idx)) != len(idx):
        raise ValueError('%s lists an index twice (got %r)' % (what, text))
    if min(idx) < 0 or max(idx) >= limit:
        raise ValueError('%s takes indices in [0, %d) (got %r)' % (what, limit, text))
    return idx


_PINNED = {}


def _sheet_to_host(canvas):
    """The one copy of a sheet's bytes to the host, into page-locked memory kept per shape (DESIGN.md section 4.4 has the rates)."""
    key = tuple(canvas.shape)
    if key not in _PINNED:
        _PINNED[key] = torch.empty(key, dtype=torch.uint8, pin_memory=True)
    _PINNED[key].copy_(canvas)               # synchronous: the bytes are there when it returns
    return _PINNED[key].numpy()


class _ClassSweep:
    """--actions for one batch: the further rollouts of each draw, their sheets (draw 0) and their scores."""

    def __init__(self, kpx_amd, model, actions, n_action, sheet_frames, image, real_im_seq, save, samples, kp_real, dev):
        self.ops, self.model, self.actions, self.sheet_frames, self.save = kpx_amd.ops, model, actions, sheet_frames, save
        self.image = image.contiguous()
        self.bsz = bsz = image.shape[0]
        self.codes = torch.eye(n_action, dtype=torch.float32, device=dev)[actions]                    # [A, n_action] one-hot rows
        self.real_row = 1 if real_im_seq is not None else 0
        self.classes = self.points = None
        self.on_class = None                 # --action-accuracy: called with (draw, class position, fut_pt_raw) for every rollout of the sweep
        if save:
            h, w = image.shape[1:3]
            cols = 1 + len(sheet_frames)
            self.classes = torch.empty((bsz, (self.real_row + len(actions)) * h, cols * w, 3), dtype=torch.uint8, device=dev)
            self.points = torch.empty((bsz, len(actions) * h, cols * w, 3), dtype=torch.uint8, device=dev)
            if real_im_seq is not None:
                self.ops.sheet_paste(self.classes, self.image.unsqueeze(1), [0], 0, 0, 'unit')
                self.ops.sheet_paste(self.classes, real_im_seq.contiguous(), sheet_frames, 0, 1, 'unit')
        self.kp_real = kp_real
        if kp_real is not None:              # the key points of every sweep run [D, A, B, 32, K, 2]: [d] is contiguous, the whole a [D * A, ...] view
            self.kp = torch.empty((samples, len(actions)) + tuple(kp_real.shape), dtype=torch.float32, device=dev)
            self.kp_div, self.div_mse, self.moments = [], [], None

    def run(self, draw, z):
        """One rollout per listed class at z; -> the frames predicted"""
        ops, n_cls = self.ops, len(self.actions)
        for a in range(n_cls):
            out = self.model.run(None, {'image': self.image, 'action_code': self.codes[a:a + 1].expand(self.bsz, -1).contiguous()}, z=z)
            pred = out['pred_im_seq'].contiguous()      # consumed before the next run() overwrites the graph's output buffers
            if self.save and draw == 0:
                ops.sheet_paste(self.classes, self.image.unsqueeze(1), [0], self.real_row + a, 0, 'unit')
                ops.sheet_paste(self.classes, pred, self.sheet_frames, self.real_row + a, 1, 'unit')
                ops.sheet_paste(self.points, out['current_points'].contiguous().unsqueeze(1), [0], a, 0, 'raw')
                ops.sheet_paste(self.points, out['future_points'].contiguous(), self.sheet_frames, a, 1, 'raw')
            if self.on_class is not None:
                self.on_class(draw, a, out['fut_pt_raw'])
            if self.kp_real is not None:
                ops.flat_copy_tensor(out['fut_pt_raw'].contiguous(), self.kp[draw, a].data_ptr())
                if n_cls >= 2:
                    if a == 0:               # this draw's own pair of accumulators (not those of --motion-metrics)
                        if self.moments is None:
                            self.moments = torch.empty((2, pred.numel()), dtype=torch.int32, device=pred.device)
                        ops.fill_raw_(self.moments, 0.0)
                    ops.draw_moments_add(pred.reshape(-1, *pred.shape[2:]), self.moments[0], self.moments[1])
        if self.kp_real is not None and n_cls >= 2:
            self.kp_div.append(ops.keypoint_draw_metrics(self.kp[draw], self.kp_real)[1])
            self.div_mse.append(ops.draw_diversity(self.moments[0], self.moments[1], n_cls, tuple(pred.shape[2:])))
        return self.bsz * N_FUTURE_FRAMES * n_cls

    def write_sheets(self, save_dir, first_sample):
        from PIL import Image
        for name, canvas in (('classes.png', self.classes), ('classes_points.png', self.points)):
            host = _sheet_to_host(canvas)    # one copy per canvas: the bytes of the PNGs
            for batch_idx in range(self.bsz):
                d = osp.join(save_dir, '%04d' % (first_sample + batch_idx))
                os.makedirs(d, exist_ok=True)
                Image.fromarray(host[batch_idx]).save(osp.join(d, name))

    def scores(self, action_scores):
        """after the last draw: this batch's class scores, as device tensors"""
        d, a = self.kp.shape[:2]
        l2, _ = self.ops.keypoint_draw_metrics(self.kp.view((d * a,) + tuple(self.kp.shape[2:])), self.kp_real, diversity=False)
        action_scores['kp_l2'].append(l2.view(d, a, self.bsz, -1))
        if a >= 2:
            action_scores['kp_div'].append(torch.stack(self.kp_div))                                   # [D, B, T]
            action_scores['div_mse'].append(torch.stack(self.div_mse).view(d, self.bsz, -1))          # [D, B, T]


def _write_actions_json(save_dir, actions, sheet_frames, real_row, cell):
    os.makedirs(save_dir, exist_ok=True)
    with open(osp.join(save_dir, 'actions.json'), 'w') as f:
        json.dump({'actions': actions, 'sheet_frames': sheet_frames, 'rows': (['real'] if real_row else []) + actions, 'points_rows': actions,
                   'cell': list(cell)}, f, indent=1)


def _drive_rows(modes, real, own):
    """the rows of drive.png, in order: ``real`` (there are real frames), ``own`` (the model's own rollout ran)"""
    return ([r for r in ('real',) if real] + [r for r in ('labels',) if 'labels' in modes] + [r for r in ('model',) if own]
            + [r for r in ('hold',) if 'hold' in modes] + [r for r in ('driver', 'transfer') if 'transfer' in modes])


class _Drive:
    """--drive for one batch: the driven rollouts, their PNGs, the sheet and the scores of labels and hold."""

    def __init__(self, kpx_amd, model, modes, scaled, sheet_frames, batch, own, save, dev):
        self.ops, self.model, self.modes, self.scaled, self.sheet_frames, self.save = kpx_amd.ops, model, modes, scaled, sheet_frames, save
        self.batch = batch
        self.image = batch['image'].contiguous()
        self.bsz = bsz = self.image.shape[0]
        self.shift = 1 % bsz                         # transfer: sample b is driven by sample b + 1 of its batch; a batch of one by itself
        real = batch.get('real_im_seq')
        self.rows = _drive_rows(modes, real is not None, own)
        self.sheet = None
        if save:
            h, w = self.image.shape[1:3]
            self.sheet = torch.empty((bsz, len(self.rows) * h, (1 + len(sheet_frames)) * w, 3), dtype=torch.uint8, device=dev)
            if real is not None:
                self.paste('real', self.image, real.contiguous())
            if 'transfer' in modes:                  # the driving sample's input image and real frames
                self.paste('driver', torch.roll(self.image, -self.shift, 0), torch.roll(real, -self.shift, 0).contiguous())

    def paste(self, row, image, seq):
        r = self.rows.index(row)
        self.ops.sheet_paste(self.sheet, image.unsqueeze(1), [0], r, 0, 'unit')
        self.ops.sheet_paste(self.sheet, seq, self.sheet_frames, r, 1, 'unit')

    def drive_of(self, mode):
        if mode == 'hold':
            return {'mode': 'hold', 'shift': 0, 'scaled': False}
        driver = {'first': self.batch['keypoints'].contiguous(), 'seq': self.batch['real_seq'].contiguous()}
        if mode == 'labels':
            return dict(driver, mode='absolute', shift=0, scaled=False)
        return dict(driver, mode='relative', shift=self.shift, scaled=self.scaled)

    def run(self, save_dir, first_sample, real_flat, drive_scores):
        """One driven rollout per listed mode; -> the frames predicted"""
        for mode in self.modes:
            out = self.model.run(None, {'image': self.image, 'action_code': self.batch['action_code']}, drive=self.drive_of(mode))
            if mode == self.modes[0]:
                self.first_out = out                 # --gif --drive-only: every mode replays a graph of its own, so these stay
            pred = out['pred_im_seq'].contiguous()   # consumed before the next run() of this mode overwrites the graph's output buffers
            if drive_scores is not None and mode in drive_scores:
                drive_scores[mode].append(self.ops.frame_metrics(pred.reshape(-1, *pred.shape[2:]), real_flat, png8=True))
            if self.save:
                self.paste(mode, self.image, pred)
                frames, points = pred.cpu().numpy(), out['future_points'].cpu().numpy() if mode == 'transfer' else None
                for batch_idx in range(self.bsz):
                    d = osp.join(save_dir, '%04d' % (first_sample + batch_idx))
                    _save_img_sequence(osp.join(d, 'drive_' + mode), frames[batch_idx], rescale=True)
                    if points is not None:
                        _save_img_sequence(osp.join(d, 'drive_transfer_points'), points[batch_idx], rescale=False)
        return self.bsz * N_FUTURE_FRAMES * len(self.modes)

    def write_sheet(self, save_dir, first_sample):
        from PIL import Image
        host = _sheet_to_host(self.sheet)            # the one copy: the bytes of the PNGs
        for batch_idx in range(self.bsz):
            d = osp.join(save_dir, '%04d' % (first_sample + batch_idx))
            os.makedirs(d, exist_ok=True)
            Image.fromarray(host[batch_idx]).save(osp.join(d, 'drive.png'))


def _write_drive_json(save_dir, rows, sheet_frames, cell, modes, scaled, n_self_driven):
    os.makedirs(save_dir, exist_ok=True)
    with open(osp.join(save_dir, 'drive.json'), 'w') as f:
        json.dump({'rows': rows, 'sheet_frames': sheet_frames, 'cell': list(cell), 'modes': modes, 'scaled': scaled,
                   'n_self_driven': n_self_driven}, f, indent=1)


def _write_drive_only_metrics(save_dir, drive_scores, n_frames):
    """--drive-only --metrics: the model's own rollout did not run, so metrics.npz holds the drive_* arrays and metrics.json the drive block"""
    arrays, blocks = _drive_arrays(drive_scores, n_frames)
    os.makedirs(save_dir, exist_ok=True)
    np.savez(osp.join(save_dir, 'metrics.npz'), **arrays)
    res = {'drive': summarise_drive(blocks)}
    with open(osp.join(save_dir, 'metrics.json'), 'w') as f:
        json.dump(res, f, indent=1, allow_nan=False)
    print(_drive_line(res['drive']))


def _drive_arrays(drive_scores, n_frames):
    """drive_scores: {mode: per batch a device tensor [B * T, 3] = (ssim, mse, psnr)} -> (the drive_* arrays of metrics.npz, each [S, T],
    summarise_drive's first argument)"""
    arrays, blocks = {}, {}
    for mode, ts in drive_scores.items():
        host = torch.cat(ts, dim=0).cpu().numpy() if ts else np.zeros((0, 3), np.float32)
        host = host.reshape(-1, n_frames, 3)
        blocks[mode] = {name: np.ascontiguousarray(host[..., i]) for i, name in enumerate(('ssim', 'mse', 'psnr'))}
        for name in DRIVE_METRICS:
            arrays['drive_%s_%s' % (mode, name)] = blocks[mode][name]
    return arrays, blocks


def _drive_line(blk):
    fmt = lambda v, spec: 'n/a' if v is None else spec % v
    parts = ['%s SSIM %s, PSNR %s dB' % (m, fmt(blk[m]['ssim']['mean'], '%.4f'), fmt(blk[m]['psnr']['mean'], '%.2f')) for m in blk['modes']]
    if 'skill' in blk:
        parts.append('skill SSIM %s, PSNR %s' % (fmt(blk['skill']['ssim'], '%.3f'), fmt(blk['skill']['psnr'], '%.3f')))
    return 'drive: ' + '; '.join(parts)


def _write_metrics(save_dir, scores, n_draws, n_frames, vgg_scores=None, motion_scores=None, action_scores=None, drive_scores=None,
                   frechet=None, accuracy=None, novelty=None, prdc=None, posterior=None):
    """scores: per batch a device tensor [draws, B * T, 3] = (ssim, mse, psnr); one copy to the host for all of them.
    vgg_scores (--vgg-metrics): per batch a device tensor [draws, B * T, 5, 2] = per layer (cos_layer, l1_layer).
    motion_scores (--motion-metrics): {'kp_l2': per batch [draws, B, T]} and for two or more draws {'kp_div': per batch [B, T], 'div_mse':
    per batch [B * T]}.
    action_scores (--actions): {'actions': [A], 'own': per batch the action codes [B, n_action], 'kp_l2': per batch [draws, A, B, T]} and for
    two or more classes {'kp_div', 'div_mse': per batch [draws, B, T]}.
    drive_scores (--drive labels / hold): {mode: per batch [B * T, 3] = (ssim, mse, psnr)}.
    frechet (--frechet): the accumulators {'real_even', 'real_odd', 'pred', 'pred_draw0'}; also writes frechet.npz.
    accuracy (--action-accuracy): the _ActionAccuracy of the run.  novelty (--novelty): the _Novelty of the run.  prdc (--prdc): the _Prdc
    of the run; also writes prdc.npz.  posterior (--posterior): the _Posterior of the run; also writes posterior.npz."""
    host = torch.cat(scores, dim=1).cpu().numpy() if scores else np.zeros((n_draws, 0, 3), np.float32)
    arr = host.reshape(n_draws, -1, n_frames, 3).transpose(1, 0, 2, 3)                  # [S, N, T, 3]
    ssim, mse, psnr = (np.ascontiguousarray(arr[..., i]) for i in range(3))
    arrays, extras = {'ssim': ssim, 'psnr': psnr, 'mse': mse}, None
    if vgg_scores is not None:
        nl = len(VGG_FEATURE_LAYERS)
        host = torch.cat(vgg_scores, dim=1).cpu().numpy() if vgg_scores else np.zeros((n_draws, 0, nl, 2), np.float32)
        layers = host.reshape(n_draws, -1, n_frames, nl, 2).transpose(1, 0, 2, 3, 4)    # [S, N, T, 5, 2]
        arrays['vgg_cos_layers'] = np.ascontiguousarray(layers[..., 0])
        arrays['vgg_l1_layers'] = np.ascontiguousarray(layers[..., 1])
        # the mean over the five layers, in fp64, stored as the fp32 the other metrics are
        extras = {'vgg_cos': arrays['vgg_cos_layers'].astype(np.float64).mean(axis=-1).astype(np.float32),
                  'vgg_l1': arrays['vgg_l1_layers'].astype(np.float64).mean(axis=-1).astype(np.float32)}
        arrays.update(extras)
    motion = None
    if motion_scores is not None:
        n_samples = ssim.shape[0]
        host = lambda ts, shape, dim: torch.cat(ts, dim=dim).cpu().numpy() if ts else np.zeros(shape, np.float32)
        motion = {'kp_l2': np.ascontiguousarray(host(motion_scores['kp_l2'], (n_draws, 0, n_frames), 1).transpose(1, 0, 2))}
        for name in ('kp_div', 'div_mse'):
            if name in motion_scores:
                motion[name] = host(motion_scores[name], (0,), 0).reshape(n_samples, n_frames)
        arrays.update(motion)
    act = None
    if action_scores is not None:
        actions = action_scores['actions']
        host = lambda ts, shape, dim: torch.cat(ts, dim=dim).cpu().numpy() if ts else np.zeros(shape, np.float32)
        own = host(action_scores['own'], (0, 1), 0)
        act = {'actions': np.asarray(actions, np.int32), 'act_own': own.argmax(axis=1).astype(np.int32),
               'act_kp_l2': np.ascontiguousarray(host(action_scores['kp_l2'], (n_draws, len(actions), 0, n_frames), 2).transpose(2, 1, 0, 3))}
        for name in ('kp_div', 'div_mse'):
            if name in action_scores:
                act['act_' + name] = np.ascontiguousarray(host(action_scores[name], (n_draws, 0, n_frames), 1).transpose(1, 0, 2))
        act['act_rank'] = action_ranks(actions, act['act_own'], act['act_kp_l2'])[1]
        arrays.update(act)
    drive = None
    if drive_scores:
        drive_arrays, drive = _drive_arrays(drive_scores, n_frames)
        arrays.update(drive_arrays)
    frechet_block = None
    if frechet is not None:
        from kpx_amd import frechet as F
        stats = {name: acc.stats() for name, acc in frechet.items()}
        stats['real'] = F.FrechetAccumulator(frechet['real_even'].dims, 'cpu').merge(frechet['real_even']).merge(frechet['real_odd']).stats()
        frechet_arrays, frechet_block = summarise_frechet(stats)
        arrays.update(frechet_arrays)
        stored = {'layers': np.array(VGG_FEATURE_LAYERS)}
        for name in ('real', 'pred', 'pred_draw0', 'real_even', 'real_odd'):
            stored.update(F.stats_arrays(name, stats[name], VGG_FEATURE_LAYERS))
        os.makedirs(save_dir, exist_ok=True)
        np.savez(osp.join(save_dir, 'frechet.npz'), **stored)
    if accuracy is not None:
        arrays.update(accuracy.arrays())
    if novelty is not None:
        if act is None and novelty.actions:
            arrays['actions'] = np.asarray(novelty.actions, np.int32)
        arrays.update(novelty.arrays())
    if prdc is not None:
        arrays.update(prdc.arrays(save_dir))
    posterior_block = None
    if posterior is not None:
        posterior_arrays, posterior_block = posterior.finish(save_dir, n_frames, {'ssim': ssim, 'psnr': psnr, 'mse': mse},
                                                             drive.get('hold') if drive is not None else None)
        arrays.update(posterior_arrays)
    os.makedirs(save_dir, exist_ok=True)
    np.savez(osp.join(save_dir, 'metrics.npz'), **arrays)
    res = summarise_metrics(ssim, psnr, mse, extras=extras, motion=motion)
    if frechet_block is not None:
        res['definition'] += ' ' + FRECHET_DEFINITION
        res['frechet'] = frechet_block
    if act is not None:
        res['actions'] = summarise_actions(actions, act['act_own'], act['act_kp_l2'], act.get('act_kp_div'), act.get('act_div_mse'))
    if drive is not None:
        res['drive'] = summarise_drive(drive, model={'ssim': ssim, 'psnr': psnr, 'mse': mse})
    if accuracy is not None:
        res['action_accuracy'] = summarise_action_accuracy(arrays)
    if novelty is not None:
        res['definition'] += ' ' + NOVELTY_DEFINITION
        res['novelty'] = summarise_novelty(arrays, mirror=novelty.mirror)
    if prdc is not None:
        res['prdc'] = prdc.P.summarise(arrays)
    if posterior_block is not None:
        res['posterior'] = posterior_block
    with open(osp.join(save_dir, 'metrics.json'), 'w') as f:
        json.dump(res, f, indent=1, allow_nan=False)
    fmt = lambda v, spec: 'n/a' if v is None else spec % v
    line = ('metrics: %d samples x %d draws: SSIM %s (best of draws %s), PSNR %s dB (best of draws %s), MSE %s'
            % (res['n_samples'], res['n_draws'], fmt(res['ssim']['mean'], '%.4f'), fmt(res['ssim']['best_of_draws'], '%.4f'),
               fmt(res['psnr']['mean'], '%.2f'), fmt(res['psnr']['best_of_draws'], '%.2f'), fmt(res['mse']['mean'], '%.3e')))
    if extras is not None:
        line += (', VGG cos %s (best of draws %s), VGG L1 %s (best of draws %s)'
                 % (fmt(res['vgg_cos']['mean'], '%.4f'), fmt(res['vgg_cos']['best_of_draws'], '%.4f'),
                    fmt(res['vgg_l1']['mean'], '%.4f'), fmt(res['vgg_l1']['best_of_draws'], '%.4f')))
    if frechet_block is not None:
        line += (', VGG Frechet (not FID/FVD) frames %s (floor %s), videos %s (floor %s)'
                 % (fmt(frechet_block['vgg_fd'], '%.4g'), fmt(frechet_block['vgg_fd_floor_layers'][-1], '%.4g'),
                    fmt(frechet_block['vgg_fvd'], '%.4g'), fmt(frechet_block['vgg_fvd_floor_layers'][-1], '%.4g')))
    if motion is not None:
        line += ', key-point L2 %s (best of draws %s)' % (fmt(res['kp_l2']['mean'], '%.4f'), fmt(res['kp_l2']['best_of_draws'], '%.4f'))
        if 'kp_div' in res:
            line += ', key-point diversity %s, draw diversity MSE %s' % (fmt(res['kp_div']['mean'], '%.4f'), fmt(res['div_mse']['mean'], '%.3e'))
    if act is not None:
        blk = res['actions']
        line += ', class top-1 %s (chance %.4f), class diversity %s' % (fmt(blk['top1'], '%.4f'), blk['chance'],
                                                                        fmt(blk['kp_div']['mean'], '%.4f') if 'kp_div' in blk else 'n/a')
    if accuracy is not None:
        blk = res['action_accuracy']
        line += (', key-point recogniser (own quantity, not comparable with published figures) top-1 real %s, predicted %s%s (chance %.4f), '
                 'key-point Frechet %s (floor %s)'
                 % (fmt(blk['real']['top1'], '%.4f'), fmt(blk['pred']['top1'], '%.4f'),
                    ', commanded %s' % fmt(blk['commanded']['top1'], '%.4f') if 'commanded' in blk else '', blk['real']['chance'],
                    fmt(blk['kp_fd']['kp_fd'], '%.4g'), fmt(blk['kp_fd']['kp_fd_floor'], '%.4g')))
    if novelty is not None:
        blk = res['novelty']
        line += (', nearest training motion (own quantity, not comparable with published figures) median pred %s, real %s, ratio %s, '
                 'copied %s, nn top-1 real %s, predicted %s'
                 % (fmt(blk['pred']['median'], '%.4f'), fmt(blk['real']['median'], '%.4f'), fmt(blk['ratio'], '%.3f'), fmt(blk['copied'], '%.3f'),
                    fmt(blk['nn_top1']['real'], '%.4f'), fmt(blk['nn_top1']['pred'], '%.4f')))
    if prdc is not None and 'draw0' in res['prdc'].get('kp', {}):
        blk = res['prdc']['kp']['draw0']
        line += (', key-point-space manifold scores at k = %d (own quantity, not comparable with published figures) precision %s, recall %s, '
                 'density %s, coverage %s' % (res['prdc']['k'], fmt(blk['precision'], '%.4f'), fmt(blk['recall'], '%.4f'),
                                              fmt(blk['density'], '%.4f'), fmt(blk['coverage'], '%.4f')))
    print('%s; %d non-finite frames' % (line, res['n_nonfinite']))
    if drive is not None:
        print(_drive_line(res['drive']))
    if posterior_block is not None:
        print(_Posterior.line(posterior_block))


POSTERIOR_ROWS = ('real', 'recon', 'model', 'driver', 'transfer')                  # the rows of posterior.png, in order


def summarise_recon(post, model=None, hold=None):
    """The ``recon`` (and ``z_skill``) entries of the ``posterior`` block; numpy only.  post: {'ssim', 'psnr', 'mse'[, 'kp_l2']: [S, T]}, the
    scores of the rollout at z = mu; model: the model's own {'ssim', 'psnr', 'mse': [S, N, T]}; hold: --drive hold's {'ssim', 'psnr',
    'mse': [S, T]}, or None when it did not run.  z_skill = (model - hold) / (posterior - hold) on the means, null as summarise_drive's
    skill is."""
    out = {'recon': {}}
    for name, x in post.items():
        x = np.asarray(x, np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            out['recon'][name] = {'mean': _json_num(x.mean()) if x.size else None,
                                  'per_frame': [_json_num(v) for v in x.mean(axis=0)] if x.shape[0] else [None] * x.shape[1]}
    if model is not None and hold is not None:
        out['z_skill'] = {}
        for name in DRIVE_METRICS:
            own, floor = np.asarray(model[name], np.float64), np.asarray(hold[name], np.float64)
            with np.errstate(invalid='ignore', over='ignore'):
                m, f = (own.mean() if own.size else np.nan), (floor.mean() if floor.size else np.nan)
                top = out['recon'][name]['mean']
                ok = top is not None and np.isfinite(m) and np.isfinite(f) and top != f
                out['z_skill'][name] = _json_num((m - f) / (top - f)) if ok else None
    return out


class _Posterior:
    """--posterior: per batch one encode, one latent_stats_add with the sample's class as its group and one more rollout at z = mu (with
    --posterior-transfer a second one at the mu of the next sample of the batch); the logit rows stay on the device until the last batch.
    Nothing here draws a random number, and everything runs after the batch's other rollouts have been consumed."""

    def __init__(self, kpx_amd, model, n_action, transfer, au, sheet_frames, save, metrics, motion, dev):
        self.P, self.ops, self.model, self.n_action, self.transfer, self.au = kpx_amd.posterior, kpx_amd.ops, model, n_action, transfer, au
        self.sheet_frames, self.save, self.metrics, self.motion, self.dev = sheet_frames, save, metrics, motion, dev
        self.state, self.counts = self.P.new_state(n_action, model.vae_dim, dev)
        self.rows, self.classes, self.kl_rows, self.scores, self.kp_l2 = [], [], [], [], []
        self.sheet = None

    def _paste(self, row, image, seq):
        r = POSTERIOR_ROWS.index(row)
        self.ops.sheet_paste(self.sheet, image.unsqueeze(1), [0], r, 0, 'unit')
        self.ops.sheet_paste(self.sheet, seq, self.sheet_frames, r, 1, 'unit')

    def begin_batch(self, batch):
        """before the batch's own rollout: the canvas of posterior.png with the rows that need no rollout"""
        if not (self.transfer and self.save):
            return
        image, real = batch['image'].contiguous(), batch['real_im_seq'].contiguous()
        bsz, (h, w) = image.shape[0], image.shape[1:3]
        shift = 1 % bsz
        self.sheet = torch.empty((bsz, len(POSTERIOR_ROWS) * h, (1 + len(self.sheet_frames)) * w, 3), dtype=torch.uint8, device=self.dev)
        self._paste('real', image, real)
        self._paste('driver', torch.roll(image, -shift, 0), torch.roll(real, -shift, 0).contiguous())

    def own_draw0(self, outputs):
        """draw 0 of the batch's own rollout, before anything replays its graph"""
        if self.sheet is not None:
            self._paste('model', outputs['im'].contiguous(), outputs['pred_im_seq'].contiguous())

    def end_batch(self, save_dir, first_sample, batch, real_flat):
        """after everything else of the batch; -> the frames predicted"""
        ops, bsz = self.ops, batch['image'].shape[0]
        logit = self.model.encode(batch['keypoints'].contiguous(), batch['real_seq'].contiguous(), batch['action_code'].contiguous())
        group = batch['action_code'].argmax(dim=1).to(torch.int32)
        self.kl_rows.append(ops.latent_stats_add(logit, self.state, self.counts, group))
        self.rows.append(logit.clone())              # a copy: the encoder's buffer is overwritten by the next replay
        self.classes.append(group)
        mu = ops.latent_sample(logit, None, 0.0)
        feed = {'image': batch['image'], 'action_code': batch['action_code']}
        runs = [('post', mu)] + ([('post_transfer', torch.roll(mu, -(1 % bsz), 0).contiguous())] if self.transfer else [])
        for name, z in runs:
            out = self.model.run(None, feed, z=z)
            pred = out['pred_im_seq'].contiguous()   # consumed before the next run() overwrites the graph's output buffers
            if name == 'post' and self.metrics:
                self.scores.append(ops.frame_metrics(pred.reshape(-1, *pred.shape[2:]), real_flat, png8=True))
                if self.motion:
                    self.kp_l2.append(ops.keypoint_draw_metrics(out['fut_pt_raw'].contiguous().unsqueeze(0), batch['real_seq'].contiguous(),
                                                                diversity=False)[0][0])
            if self.sheet is not None:
                self._paste('recon' if name == 'post' else 'transfer', batch['image'].contiguous(), pred)
            if self.save:
                frames = pred.cpu().numpy()
                points = out['future_points'].cpu().numpy() if name == 'post' else None
                for batch_idx in range(bsz):
                    d = osp.join(save_dir, '%04d' % (first_sample + batch_idx))
                    _save_img_sequence(osp.join(d, 'post_seq' if name == 'post' else name), frames[batch_idx], rescale=True)
                    if points is not None:
                        _save_img_sequence(osp.join(d, 'post_points'), points[batch_idx], rescale=False)
        if self.sheet is not None:
            from PIL import Image
            host = _sheet_to_host(self.sheet)
            for batch_idx in range(bsz):
                Image.fromarray(host[batch_idx]).save(osp.join(save_dir, '%04d' % (first_sample + batch_idx), 'posterior.png'))
            self.sheet = None
        return bsz * N_FUTURE_FRAMES * len(runs)

    def finish(self, save_dir, n_frames, model_scores=None, hold=None):
        """after the last batch -> (the post_* arrays of metrics.npz, the ``posterior`` block); writes <save_dir>/posterior.npz"""
        v = self.model.vae_dim
        cat = lambda ts, shape, dtype: torch.cat(ts, dim=0).cpu().numpy() if ts else np.zeros(shape, dtype)
        state, counts = self.state.cpu().numpy(), self.counts.cpu().numpy()
        os.makedirs(save_dir, exist_ok=True)
        np.savez(osp.join(save_dir, 'posterior.npz'), logit=cat(self.rows, (0, 2 * v), np.float32), classes=cat(self.classes, (0,), np.int32),
                 kl_rows=cat(self.kl_rows, (0,), np.float64), state=state, counts=counts, au_threshold=np.float64(self.au))
        block = self.P.summarise_posterior(state, counts, self.au)
        arrays = {}
        if self.metrics:
            host = cat(self.scores, (0, 3), np.float32).reshape(-1, n_frames, 3)
            for i, name in enumerate(('ssim', 'mse', 'psnr')):
                arrays['post_' + name] = np.ascontiguousarray(host[..., i])
            if self.motion:
                arrays['post_kp_l2'] = cat(self.kp_l2, (0, n_frames), np.float32).reshape(-1, n_frames)
            block.update(summarise_recon({key[5:]: x for key, x in arrays.items()}, model_scores, hold))
        return arrays, block

    @staticmethod
    def line(block):
        fmt = lambda x, spec: 'n/a' if x is None else spec % x
        if not block.get('n'):
            return 'posterior (own quantity, not comparable with published figures): no rows'
        text = ('posterior (own quantity, not comparable with published figures): %d rows, KL %s nats, active units %d of %d, dead sigma share %s, '
                'aggregate KL to the prior %s' % (block['n'], fmt(block['kl_total'], '%.4f'), block['active_units'], block['vae_dim'],
                                                  fmt(float(np.mean(block['dead_sigma_share'])), '%.3f'),
                                                  fmt(block['agg_kl_total'], '%.4f')))
        if 'recon' in block:
            text += ', recon SSIM %s, PSNR %s dB' % (fmt(block['recon']['ssim']['mean'], '%.4f'), fmt(block['recon']['psnr']['mean'], '%.2f'))
        if 'z_skill' in block:
            text += ', z skill SSIM %s, PSNR %s' % (fmt(block['z_skill']['ssim'], '%.3f'), fmt(block['z_skill']['psnr'], '%.3f'))
        return text


class _LongRollout:
    """--frames / --rate: after a batch's ordinary rollout a second one, chained to ``frames`` predicted frames and resampled by ``rate``
    (FinalModel.run(frames=, rate=, resample=)), at the same z for segment 0 and seeded z for the later segments.  Per sample long.gif
    (with --gif) and long.avi (with --video), both pred | points, and long_points.npy [T',K,2]; per run long.json: the mean speed curve and the seam ratio (kpx_amd.resample)."""

    def __init__(self, kpx_amd, model, frames, rate, resample, fps, dither, dev, video=None):
        self.kpx, self.model, self.frames, self.rate, self.resample, self.dev = kpx_amd, model, frames, rate, resample, dev
        self.gifs = kpx_amd.gif.RolloutGifs(fps * rate, dither) if fps is not None else None       # F times the frames in the same time
        self.videos = kpx_amd.mjpeg.RolloutVideos(video[0] * rate, video[1]) if video is not None else None
        self.compose = (self.gifs or self.videos)._canvas
        self.bytes = []
        self.speed_sum, self.n, self.sizes = np.zeros(frames * rate, np.float64), 0, []

    def run(self, save_dir, first_sample, image, action_code, z):
        """z: the [B,V] of the batch's ordinary rollout -> the number of frames predicted"""
        ops, bsz, segments = self.kpx.ops, image.shape[0], self.frames // N_FUTURE_FRAMES
        more = np.random.RandomState(first_sample).randn(segments - 1, bsz, self.model.vae_dim).astype(np.float32)
        z_all = torch.cat([z.reshape(1, bsz, -1), torch.from_numpy(more).to(self.dev)])
        out = self.model.run(None, {'image': image, 'action_code': action_code}, z=z_all, frames=self.frames, rate=self.rate, resample=self.resample)
        pts = out['fut_pt_raw'].contiguous()
        speed = ops.points_speed(out['first_pt'].reshape(bsz, -1, 2).contiguous(), pts, float(self.rate))
        canvas = self.compose([(out['im'], out['pred_im_seq'], 'unit'), (out['current_points'], out['future_points'], 'raw')])
        pts_host = pts.cpu().numpy()
        if self.gifs is not None:
            idx, palettes, sizes = ops.gif_indices(canvas, self.gifs.dither)
            host = self.gifs._host(idx)
        if self.videos is not None:
            self.videos.write_canvas(save_dir, first_sample, 'long', canvas, self.bytes)
        for i in range(bsz):
            d = osp.join(save_dir, '%04d' % (first_sample + i))
            os.makedirs(d, exist_ok=True)
            if self.gifs is not None:
                self.kpx.gif.write_gif(osp.join(d, 'long.gif'), host[i], palettes[i, :sizes[i]], self.gifs.delay)
                self.sizes.append(int(sizes[i]))
            np.save(osp.join(d, 'long_points.npy'), pts_host[i])
        self.speed_sum += speed.cpu().numpy().sum(0)
        self.n += bsz
        return bsz * self.frames * self.rate

    def write_json(self, save_dir):
        from kpx_amd.resample import seam_ratio
        speed = self.speed_sum / max(self.n, 1)
        os.makedirs(save_dir, exist_ok=True)
        doc = {'frames': self.frames, 'rate': self.rate, 'resample': self.resample, 'n_frames': self.frames * self.rate,
               'columns': ['pred', 'points']}
        if self.gifs is not None:
            doc.update({'fps': self.gifs.fps, 'delay_cs': self.gifs.delay})
        doc.update({'n_samples': self.n, 'speed_unit': 'mean key-point displacement per source frame, in the [-1, 1] coordinates',
                    'speed': [_json_num(v) for v in speed], 'seam_ratio': seam_ratio(speed, self.frames, self.rate)})
        if self.gifs is not None:
            doc['palette_sizes'] = self.sizes
        if self.videos is not None:
            doc.update({'video_fps': self.videos.fps, 'video_quality': self.videos.quality, 'video_bytes': self.bytes})
        with open(osp.join(save_dir, 'long.json'), 'w') as f:
            json.dump(doc, f, indent=1)


def _save_img_sequence(output_dir, img_seq, rescale=False, raw=False):
    """reference :151-156"""
    os.makedirs(output_dir, exist_ok=True)
    for i in range(img_seq.shape[0]):
        _save_img(osp.join(output_dir, '%06d.png' % i), img_seq[i], rescale=rescale, raw=raw)


def main(argv=None):
    from train import IMAGE_SIZE_HELP, config_image_size, load_config
    parser = ArgumentParser()
    parser.add_argument('--config', type=str, required=True, help='path of the configuration file')
    parser.add_argument('--checkpoint_stage1', type=str, required=True, help='path of the stage1 checkpoint')
    parser.add_argument('--checkpoint_stage2', type=str, required=False, default=None,
                        help='path of the stage2 checkpoint (required unless --drive-only)')
    parser.add_argument('--save_dir', type=str, required=False, help='root dir to save results', default='results/eval')
    parser.add_argument('--synthetic', type=int, default=0)
    parser.add_argument('--batch', type=int, default=8)             # reference :27
    parser.add_argument('--colors_seed', type=int, default=0, help='seed of the key-point palette (the reference draws it unseeded)')
    parser.add_argument('--image-size', type=int, default=None, metavar='S', help=IMAGE_SIZE_HELP)
    parser.add_argument('--no-save', action='store_true')
    parser.add_argument('--metrics', action='store_true', help='score the predictions: <save_dir>/metrics.npz and metrics.json')
    parser.add_argument('--samples', type=int, default=1, help='rollouts per batch with fresh z (PNGs from the first)')
    parser.add_argument('--vgg-metrics', action='store_true',
                        help='with --metrics: VGG19 feature-space cosine similarity and perceptual L1 per predicted frame (paths.vggnet)')
    parser.add_argument('--synthetic-vgg', action='store_true', help='He-normal VGG19 weights when paths.vggnet is absent')
    parser.add_argument('--frechet', action='store_true',
                        help='with --metrics --vgg-metrics: the Frechet distance between the real and the predicted frames (and rollouts) '
                             'in the feature space of the same VGG19, with its even / odd noise floor, and <save_dir>/frechet.npz.  This '
                             "project's own quantity: not FID/FVD, not comparable with published figures.  The rollouts of --actions and "
                             '--drive are not accumulated')
    parser.add_argument('--motion-metrics', action='store_true',
                        help='with --metrics: key-point error against the pseudo labels and, for --samples >= 2, the diversity of the draws')
    parser.add_argument('--actions', type=str, default=None,
                        help="'all' or i,j,k: also roll every image out under these action classes at the same z: classes.png, "
                             'classes_points.png, actions.json and, with --metrics, the class scores')
    parser.add_argument('--sheet-frames', type=str, default=None,
                        help='with --actions or --drive: the predicted frames of a sheet (default 3,7,...,31)')
    parser.add_argument('--drive', type=str, default=None,
                        help='comma list of labels, hold, transfer: also roll the translator out on given key points: drive_*/, drive.png, '
                             'drive.json and, with --metrics, the scores of labels and hold')
    parser.add_argument('--drive-scaled', action='store_true',
                        help='with --drive transfer: scale the driving motion by the ratio of the two constellations\' spreads')
    parser.add_argument('--drive-only', action='store_true',
                        help="with --drive: skip the model's own rollout; --checkpoint_stage2 may then be omitted")
    parser.add_argument('--action-accuracy', type=str, default=None, metavar='CKPT',
                        help='with --metrics: a checkpoint of train.py --mode action_classifier; its recogniser classifies the real and the '
                             'predicted key points (with --actions: every class rollout against the commanded class) and gives a Frechet '
                             "distance in its feature space.  This project's own key-point-space quantity: not comparable with published "
                             'action-recognition or FVD figures')
    parser.add_argument('--action-accuracy-ema', action='store_true',
                        help='with --action-accuracy: read the recogniser under its averaged weights (it was trained with train.py --ema)')
    parser.add_argument('--ema', action='store_true',
                        help="read every checkpoint given under its averaged weights (train.py --ema: the <name>/ExponentialMovingAverage entries take their variables' places); a checkpoint without them is refused")
    parser.add_argument('--gif', action='store_true',
                        help='per sample pred.gif (the input image, then the predicted frames of draw 0) and compare.gif (real | pred | '
                             'points side by side), quantised to one palette per GIF on the device; <save_dir>/gif.json')
    parser.add_argument('--gif-fps', type=int, default=None, help='with --gif: frames per second, 1..50 (default 10)')
    parser.add_argument('--gif-dither', type=int, default=None, help='with --gif: amplitude of the 4x4 ordered dither, 0..64 (default 0: none)')
    parser.add_argument('--video', action='store_true',
                        help='per sample pred.avi and compare.avi, the frames and columns of the GIFs in true colour: Motion-JPEG in an AVI, '
                             'every frame JPEG-coded on the device; <save_dir>/video.json')
    parser.add_argument('--video-fps', type=int, default=None, help='with --video: frames per second, 1..240 (default 10)')
    parser.add_argument('--video-quality', type=int, default=None, help='with --video: the JPEG quality, 1..100 (default 90)')
    parser.add_argument('--novelty', action='store_true',
                        help='with --metrics: search every rollout and the real future in the training motions of train_set.txt (the nearest '
                             "window per action class, in HIP) and report how far they lie.  This project's own key-point-space quantity: "
                             'not comparable with published figures')
    parser.add_argument('--novelty-sheets', action='store_true',
                        help='with --novelty: per sample nearest.png, every rollout above its nearest training window (--sheet-frames picks the frames)')
    parser.add_argument('--novelty-no-mirror', action='store_true', help='with --novelty: do not search the mirror images of the training motions')
    parser.add_argument('--prdc', action='store_true',
                        help='with --metrics: precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of the '
                             'rollouts against the real motions, from exact fp64 nearest-neighbour searches in HIP, in key-point space and with '
                             "--action-accuracy in the recogniser's feature space; <save_dir>/prdc.npz keeps the rows.  This project's own "
                             'quantities: not comparable with published figures')
    parser.add_argument('--prdc-k', type=int, default=None, metavar='K', help='with --prdc: the neighbour that sets a ball\'s radius, 1..8 (default 5)')
    parser.add_argument('--frames', type=int, default=None,
                        help='with --gif or --video: a second rollout per batch chained to this many predicted frames (a multiple of 32, default 32): '
                             'per sample long.gif / long.avi and long_points.npy, <save_dir>/long.json with the speed curve and the seam ratio')
    parser.add_argument('--rate', type=int, default=None, help='with --gif or --video: resample the second rollout to F = 1..64 times the frames (default 1); long.gif plays at F x --gif-fps, long.avi at F x --video-fps')
    parser.add_argument('--resample', type=str, default=None, help='with --rate: linear or cubic (default)')
    parser.add_argument('--posterior', action='store_true',
                        help='encode the real motion of every sample with the stage-2 encoder (needs a checkpoint with vae_encoder/*): one more '
                             'rollout at z = mu (post_seq/, post_points/; with --metrics post_ssim ... in metrics.npz), the KL per latent '
                             'dimension, active units and the distance of the aggregate posterior from the prior (a posterior block in '
                             "metrics.json), <save_dir>/posterior.npz keeps the rows.  This project's own quantities: not comparable with "
                             'published figures')
    parser.add_argument('--posterior-transfer', action='store_true',
                        help="with --posterior: also decode the mu of the batch's next sample from each sample's image, first pose and class: "
                             'post_transfer/ and the sheet posterior.png (--sheet-frames picks the frames)')
    parser.add_argument('--posterior-au', type=float, default=None, metavar='T',
                        help='with --posterior: a latent unit is active when the variance of its mu over the samples exceeds T (default 0.01)')
    args = parser.parse_args(argv)
    if (args.posterior_transfer or args.posterior_au is not None) and not args.posterior:
        parser.error('--posterior-transfer and --posterior-au shape the outputs of --posterior and need it')
    if args.posterior and args.synthetic:
        parser.error('--posterior encodes the pseudo labels of real videos, and --synthetic inputs have none')
    if args.posterior and args.drive_only:
        parser.error("--drive-only skips the model's own rollout and needs no stage-2 checkpoint, which --posterior reads the encoder from")
    if args.posterior_transfer and args.no_save:
        parser.error('--posterior-transfer writes files, and --no-save writes none')
    posterior_au = 0.01 if args.posterior_au is None else args.posterior_au
    if not (np.isfinite(posterior_au) and posterior_au >= 0):
        parser.error('--posterior-au takes a finite threshold >= 0 (got %r)' % args.posterior_au)
    long_frames, long_rate = 32 if args.frames is None else args.frames, 1 if args.rate is None else args.rate
    want_long = args.frames is not None or args.rate is not None
    if args.resample is not None and args.rate is None:
        parser.error('--resample chooses how --rate places the frames in between and needs it')
    if want_long and not (args.gif or args.video):
        parser.error('--frames and --rate write long.gif beside the files of --gif and need it')
    if want_long and args.drive_only:
        parser.error("--drive-only skips the model's own rollout, which --frames and --rate lengthen")
    if long_frames < 32 or long_frames % 32:
        parser.error('--frames takes a positive multiple of 32 (got %d)' % long_frames)
    if not 1 <= long_rate <= 64:
        parser.error('--rate takes 1..64 (got %d)' % long_rate)
    if (args.resample or 'cubic') not in ('linear', 'cubic'):
        parser.error('--resample takes linear or cubic (got %r)' % args.resample)
    def check_long_gif(side):
        if args.gif and 2 * (1 + long_frames * long_rate) * side * side > 1 << 24:
            parser.error('--frames x --rate: long.gif would hold %d frames of two %d x %d cells, and the colour histogram of one GIF counts '
                         'at most 2^24 pixels (%d frames)' % (1 + long_frames * long_rate, side, side, (1 << 24) // (2 * side * side)))
    check_long_gif(128)
    if (args.novelty_sheets or args.novelty_no_mirror) and not args.novelty:
        parser.error('--novelty-sheets and --novelty-no-mirror shape the search of --novelty and need it')
    if args.novelty and args.synthetic:
        parser.error('--novelty searches the training motions for the rollouts of real videos and their pseudo labels, and --synthetic '
                     'inputs have neither')
    if args.novelty and not args.metrics:
        parser.error('--novelty adds to the scores of --metrics and needs it')
    if args.novelty and args.drive_only:
        parser.error("--drive-only skips the model's own rollout, which --novelty is about")
    if args.novelty_sheets and args.no_save:
        parser.error('--novelty-sheets writes files, and --no-save writes none')
    if args.novelty_sheets and args.samples > 31:
        parser.error('--novelty-sheets draws two rows per draw and holds at most 31 --samples (got %d)' % args.samples)
    if args.prdc_k is not None and not args.prdc:
        parser.error('--prdc-k sets the neighbour count of --prdc and needs it')
    if args.prdc and args.synthetic:
        parser.error('--prdc compares the rollouts of real videos with their pseudo labels, and --synthetic inputs have neither')
    if args.prdc and not args.metrics:
        parser.error('--prdc adds to the scores of --metrics and needs it')
    if args.prdc and args.drive_only:
        parser.error("--drive-only skips the model's own rollout, which --prdc is about")
    prdc_k = 5 if args.prdc_k is None else args.prdc_k
    if not 1 <= prdc_k <= 8:
        parser.error('--prdc-k takes 1..8 neighbours (got %d)' % prdc_k)
    if (args.gif_fps is not None or args.gif_dither is not None) and not args.gif:
        parser.error('--gif-fps and --gif-dither shape the files of --gif and need it')
    if args.gif and args.no_save:
        parser.error('--gif writes files, and --no-save writes none')
    gif_fps = 10 if args.gif_fps is None else args.gif_fps
    gif_dither = 0 if args.gif_dither is None else args.gif_dither
    if not 1 <= gif_fps <= 50:
        parser.error('--gif-fps takes 1..50 frames per second (got %d)' % gif_fps)
    if not 0 <= gif_dither <= 64:
        parser.error('--gif-dither takes an amplitude in 0..64 (got %d)' % gif_dither)
    if want_long and args.gif and gif_fps * long_rate > 50:
        parser.error('--gif-fps %d x --rate %d = %d frames per second, and a GIF plays at most 50: lower --gif-fps'
                     % (gif_fps, long_rate, gif_fps * long_rate))
    if (args.video_fps is not None or args.video_quality is not None) and not args.video:
        parser.error('--video-fps and --video-quality shape the files of --video and need it')
    if args.video and args.no_save:
        parser.error('--video writes files, and --no-save writes none')
    video_fps = 10 if args.video_fps is None else args.video_fps
    video_quality = 90 if args.video_quality is None else args.video_quality
    if not 1 <= video_fps <= 240:
        parser.error('--video-fps takes 1..240 frames per second (got %d)' % video_fps)
    if not 1 <= video_quality <= 100:
        parser.error('--video-quality takes 1..100 (got %d)' % video_quality)
    if want_long and args.video and video_fps * long_rate > 240:
        parser.error('--video-fps %d x --rate %d = %d frames per second, and long.avi plays at most 240: lower --video-fps'
                     % (video_fps, long_rate, video_fps * long_rate))
    if args.sheet_frames is not None and args.actions is None and args.drive is None and not args.novelty_sheets and not args.posterior_transfer:
        parser.error('--sheet-frames picks the frames of the sheets of --actions / --drive / --novelty-sheets and needs it')
    drive_modes = None
    if args.drive is not None:
        listed = [m.strip() for m in args.drive.split(',')] if args.drive.strip() else []
        if not listed:
            parser.error('--drive lists nothing (modes: %s)' % ', '.join(DRIVE_MODES))
        for m in listed:
            if m not in DRIVE_MODES:
                parser.error('--drive takes a comma list of %s (got %r)' % (', '.join(DRIVE_MODES), m))
        if len(set(listed)) != len(listed):
            parser.error('--drive lists a mode twice (got %r)' % args.drive)
        drive_modes = [m for m in DRIVE_MODES if m in listed]          # run and shown in the one order of DRIVE_MODES
        if args.synthetic and set(drive_modes) - {'hold'}:
            parser.error('--drive labels and transfer take their key points from the pseudo labels, and --synthetic inputs have none '
                         '(hold is allowed)')
    if args.drive_scaled and 'transfer' not in (drive_modes or ()):
        parser.error('--drive-scaled scales the motion of --drive transfer and needs it')
    if args.drive_only:
        if drive_modes is None:
            parser.error('--drive-only keeps the rollouts of --drive alone and needs it')
        for flag, on in (('--samples > 1', args.samples > 1), ('--actions', args.actions is not None), ('--vgg-metrics', args.vgg_metrics),
                         ('--frechet', args.frechet), ('--motion-metrics', args.motion_metrics),
                         ('--action-accuracy', args.action_accuracy is not None)):
            if on:
                parser.error("--drive-only skips the model's own rollout, which %s is about" % flag)
        if args.metrics and not set(drive_modes) & {'labels', 'hold'}:
            parser.error('--drive-only --metrics scores labels and hold, and --drive lists neither (transfer has no ground truth)')
    elif args.checkpoint_stage2 is None:
        parser.error('the following arguments are required: --checkpoint_stage2 (unless --drive-only)')
    if args.vgg_metrics and not args.metrics:
        parser.error('--vgg-metrics adds to the scores of --metrics and needs it')
    if args.frechet and not (args.metrics and args.vgg_metrics):
        parser.error('--frechet adds to the features of --metrics --vgg-metrics and needs both')
    if args.motion_metrics and not args.metrics:
        parser.error('--motion-metrics adds to the scores of --metrics and needs it')
    if args.motion_metrics and args.samples > MAX_MOTION_DRAWS:
        parser.error('--motion-metrics holds at most %d --samples in its exact accumulators (got %d)' % (MAX_MOTION_DRAWS, args.samples))
    if args.action_accuracy is not None and args.synthetic:
        parser.error('--action-accuracy classifies the pseudo labels of the real frames and the rollouts of their classes, and --synthetic '
                     'inputs have neither')
    if args.action_accuracy_ema and args.action_accuracy is None:
        parser.error('--action-accuracy-ema reads the checkpoint of --action-accuracy and needs it')
    if args.action_accuracy is not None and not args.metrics:
        parser.error('--action-accuracy adds to the scores of --metrics and needs it')
    if args.metrics and args.synthetic:
        parser.error('--metrics scores predictions against the real future frames, and --synthetic inputs have no ground truth')
    if args.samples < 1:
        parser.error('--samples must be >= 1 (got %d)' % args.samples)
    config = load_config(args.config)
    size = config_image_size(config, args.image_size)
    if want_long:
        check_long_gif(size)
    actions = sheet_frames = None
    if args.actions is not None or drive_modes is not None or args.novelty_sheets or args.posterior_transfer:
        n_cls_all = config['model'].get('n_action', 9)
        try:
            if args.actions is not None:
                actions = list(range(n_cls_all)) if args.actions.strip() == 'all' else _parse_index_list(args.actions, '--actions', n_cls_all)
            sheet_frames = list(SHEET_FRAMES_DEFAULT)
            if args.sheet_frames is not None:
                sheet_frames = _parse_index_list(args.sheet_frames, '--sheet-frames', N_FUTURE_FRAMES)
                if sheet_frames != sorted(sheet_frames) or len(sheet_frames) > 63:
                    raise ValueError('--sheet-frames takes at most 63 increasing frame indices (got %r)' % args.sheet_frames)
        except ValueError as e:
            parser.error(str(e))
        if actions is not None and len(actions) * args.samples > MAX_MOTION_DRAWS:
            parser.error('--actions scores classes x --samples as draws and holds at most %d of them (got %d x %d)'
                         % (MAX_MOTION_DRAWS, len(actions), args.samples))
    checkpoints = [args.checkpoint_stage1] + ([args.checkpoint_stage2] if args.checkpoint_stage2 is not None else [])
    for p in checkpoints + ([args.action_accuracy] if args.action_accuracy is not None else []):    # reference :34-38
        if not (osp.exists(p) or osp.exists(p + '.index')):                 # .npz file or TensorFlow bundle prefix
            raise Exception('checkpoint not found at %s' % p)
    vggnet = config.get('paths', {}).get('vggnet')
    if args.vgg_metrics and not args.synthetic_vgg and not os.path.exists(str(vggnet)):      # as train.py
        raise Exception('file of pretrained vgg19 does not exist at: %s (pass --synthetic-vgg for benchmarking)' % vggnet)
    import kpx_amd
    dev = torch.device('cuda', 0)
    vgg = None
    if args.vgg_metrics:
        vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(), device=dev) if args.synthetic_vgg else kpx_amd.Vgg19(vggnet, device=dev)
    model = kpx_amd.FinalModel(config, device=dev, image_size=size, point_maps=not args.no_save, colors_seed=args.colors_seed,
                               **({'posterior': True} if args.posterior else {}))
    print('model initialized')
    model.build(None)
    for p in checkpoints:                                            # reference :76-77: two partial restores by name
        model.restore(None, p, **({'ema': True} if args.ema else {}))
    n_action = config['model']['n_action']
    gifs = kpx_amd.gif.RolloutGifs(gif_fps, gif_dither) if args.gif else None
    videos = kpx_amd.mjpeg.RolloutVideos(video_fps, video_quality) if args.video else None
    animations = [a for a in (gifs, videos) if a is not None]     # the same canvases, written at the same places
    long_run = _LongRollout(kpx_amd, model, long_frames, long_rate, args.resample or 'cubic', gif_fps if args.gif else None, gif_dither, dev,
                            video=(video_fps, video_quality) if args.video else None) if want_long else None
    sample_idx, frames, t0 = 0, 0, time.time()
    if not args.synthetic:                       # reference :43-51, :84-130: the test subset through the sequence loader
        loader = kpx_amd.data.SequenceDataLoader(config['paths']['data_dir'], 'test', n_points=config['model']['n_pts'], n_action=n_action,
                                                 random_order=False, randomness=False, with_image_seq=True, image_size=size)
        scores, n_frames = [], 32
        vgg_scores = [] if args.vgg_metrics else None
        frechet = None
        if args.frechet:             # moments over the whole test set: the real samples by parity, every draw of the predictions, draw 0
            dims = [int(vgg.params[name][0].shape[3]) for name in VGG_FEATURE_LAYERS]
            frechet = {name: kpx_amd.frechet.FrechetAccumulator(dims, dev) for name in ('real_even', 'real_odd', 'pred', 'pred_draw0')}
        n_scored = 0                                                     # samples scored so far: the parity of a real sample
        motion_scores = action_scores = None
        if actions and args.metrics:
            action_scores = {'actions': actions, 'own': [], 'kp_l2': []}
            if len(actions) >= 2:
                action_scores.update(kp_div=[], div_mse=[])
        if args.motion_metrics:
            motion_scores = {'kp_l2': []} if args.samples < 2 else {'kp_l2': [], 'kp_div': [], 'div_mse': []}
        drive_scores = {m: [] for m in drive_modes if m != 'transfer'} if drive_modes and args.metrics else None
        n_self_driven = 0
        accuracy = _ActionAccuracy(kpx_amd, config, args.action_accuracy, dev, args.samples, actions, ema=args.action_accuracy_ema) if args.action_accuracy is not None else None
        novelty = None
        if args.novelty:
            novelty = _Novelty(kpx_amd, config, dev, args.samples, actions, not args.novelty_no_mirror,
                               sheet_frames if args.novelty_sheets else None, model.colors)
        prdc = _Prdc(kpx_amd, dev, args.samples, actions, prdc_k, accuracy) if args.prdc else None
        posterior = _Posterior(kpx_amd, model, n_action, args.posterior_transfer, posterior_au, sheet_frames, not args.no_save, args.metrics,
                               args.motion_metrics, dev) if args.posterior else None
        n_read = 0                                                       # samples read so far: the listing line of a batch's first sample
        for batch in loader.batches(args.batch, dev, repeat=False, num_preprocess_threads=12):
            bsz = batch['image'].shape[0]
            n_read += bsz
            if args.drive_only:              # the driven rollouts alone: no own rollout, so no draws and nothing of what they write
                real_flat = batch['real_im_seq'].reshape(bsz * n_frames, *batch['real_im_seq'].shape[2:]) if args.metrics else None
                if not args.no_save:
                    image, real = batch['image'].cpu().numpy(), batch['real_im_seq'].cpu().numpy()
                    for batch_idx in range(bsz):
                        d = osp.join(args.save_dir, '%04d' % (sample_idx + batch_idx))
                        os.makedirs(d, exist_ok=True)
                        _save_img(osp.join(d, 'input_im.png'), image[batch_idx], rescale=True)
                        _save_img_sequence(osp.join(d, 'real_seq'), real[batch_idx], rescale=True)
                driven = _Drive(kpx_amd, model, drive_modes, args.drive_scaled, sheet_frames, batch, False, not args.no_save, dev)
                frames += driven.run(args.save_dir, sample_idx, real_flat, drive_scores)
                if not args.no_save:
                    driven.write_sheet(args.save_dir, sample_idx)
                for anim in animations:
                    o = driven.first_out
                    anim.write(args.save_dir, sample_idx, [('real', batch['image'], batch['real_im_seq'], 'unit'),
                                                           ('pred', batch['image'], o['pred_im_seq'], 'unit'),
                                                           ('points', o['current_points'], o['future_points'], 'raw')])
                n_self_driven += bsz if 'transfer' in drive_modes and bsz == 1 else 0
                sample_idx += bsz
                continue
            if args.metrics:
                real_seq = batch['real_im_seq']
                n_frames = real_seq.shape[1]
                real_flat = real_seq.reshape(bsz * n_frames, *real_seq.shape[2:])
                score = torch.empty((args.samples, bsz * n_frames, 3), dtype=torch.float32, device=dev)
                scores.append(score)
                if args.vgg_metrics:         # the real frames' features once per batch, reused by every draw
                    if frechet is not None:
                        split = kpx_amd.frechet.FrechetSplit([frechet['real_even'], frechet['real_odd']], n_scored)
                        scorer = kpx_amd.FeatureScorer(vgg, real_flat, frechet=split, frames_per_video=n_frames)
                    else:
                        scorer = kpx_amd.FeatureScorer(vgg, real_flat)
                    n_scored += bsz
                    vgg_score = torch.empty((args.samples, bsz * n_frames, len(VGG_FEATURE_LAYERS), 2), dtype=torch.float32, device=dev)
                    vgg_scores.append(vgg_score)
                if args.motion_metrics:      # every draw's key points, and two integer accumulators per value of the predicted frames
                    kp_real = batch['real_seq'].contiguous()
                    kp_pred = torch.empty((args.samples,) + tuple(kp_real.shape), dtype=torch.float32, device=dev)
                    if args.samples >= 2:
                        moments = torch.empty((2, real_flat.numel()), dtype=torch.int32, device=dev)
                        kpx_amd.ops.fill_raw_(moments, 0.0)
                if accuracy is not None:
                    accuracy.begin_batch(batch)
                if novelty is not None:
                    novelty.begin_batch([line.split()[0] for line in loader._images[n_read - bsz:n_read]], batch)
                if prdc is not None:
                    prdc.begin_batch(batch)
            if posterior is not None:
                posterior.begin_batch(batch)
            sweep = None
            if actions:
                sweep = _ClassSweep(kpx_amd, model, actions, n_action, sheet_frames, batch['image'], batch['real_im_seq'], not args.no_save,
                                    args.samples, batch['real_seq'].contiguous() if args.metrics else None, dev)
                if args.metrics:
                    action_scores['own'].append(batch['action_code'].clone())
                hooks = [h.class_rollout for h in (accuracy, novelty, prdc) if h is not None]
                if hooks:
                    sweep.on_class = hooks[0] if len(hooks) == 1 else lambda *a: [h(*a) for h in hooks]
            for draw in range(args.samples):
                # --actions: one z per batch and draw, drawn here, for the batch's own rollout and for every class of the sweep
                # --frames / --rate: drawn here too -- the draw run() would make itself, so the ordinary rollout keeps its bits
                z = torch.randn((bsz, model.vae_dim), device=dev) if actions or long_run is not None else None
                if draw == 0:
                    z_first = z
                outputs = model.run(None, {'image': batch['image'], 'action_code': batch['action_code']}, z=z)
                frames += bsz * 32
                if args.metrics:             # enqueued before the next run() overwrites the graph's output buffers
                    pred = outputs['pred_im_seq']
                    pred_flat = pred.reshape(bsz * n_frames, *pred.shape[2:])
                    kpx_amd.ops.frame_metrics(pred_flat, real_flat, png8=True, out=score[draw])
                    if frechet is not None:
                        scorer(pred_flat, out=vgg_score[draw], frechet=[frechet['pred'], frechet['pred_draw0']] if draw == 0 else frechet['pred'])
                    elif args.vgg_metrics:
                        scorer(pred_flat, out=vgg_score[draw])
                    if accuracy is not None:
                        accuracy.own_draw(draw, outputs['fut_pt_raw'])
                    if novelty is not None:
                        novelty.own_draw(draw, outputs['fut_pt_raw'])
                    if prdc is not None:
                        prdc.own_draw(draw, outputs['fut_pt_raw'])
                    if args.motion_metrics:
                        kpx_amd.ops.flat_copy_tensor(outputs['fut_pt_raw'].contiguous(), kp_pred[draw].data_ptr())
                        if args.samples >= 2:
                            kpx_amd.ops.draw_moments_add(pred_flat, moments[0], moments[1])
                        if draw == args.samples - 1:
                            kp_l2, kp_div = kpx_amd.ops.keypoint_draw_metrics(kp_pred, kp_real, diversity=args.samples >= 2)
                            motion_scores['kp_l2'].append(kp_l2)
                            if args.samples >= 2:
                                res = kpx_amd.ops.draw_diversity(moments[0], moments[1], args.samples, pred.shape[2:], std_map=not args.no_save)
                                div_mse, std_map = res if not args.no_save else (res, None)
                                motion_scores['kp_div'].append(kp_div)
                                motion_scores['div_mse'].append(div_mse)
                                if std_map is not None:      # the directories of this batch exist since draw 0
                                    spread = std_map.cpu().numpy().reshape(bsz, n_frames, *std_map.shape[1:], 1)
                                    for batch_idx in range(bsz):
                                        _save_img_sequence(osp.join(args.save_dir, '%04d' % (sample_idx - bsz + batch_idx), 'pred_std'),
                                                           spread[batch_idx], raw=True)
                if draw == 0 and not args.no_save:
                    o = {k: v.cpu().numpy() for k, v in outputs.items() if isinstance(v, torch.Tensor)}
                    real = batch['real_im_seq'].cpu().numpy()
                    for batch_idx in range(bsz):
                        d = osp.join(args.save_dir, '%04d' % sample_idx)
                        os.makedirs(d, exist_ok=True)
                        _save_img(osp.join(d, 'input_im.png'), o['im'][batch_idx], rescale=True)
                        _save_img(osp.join(d, 'current_points.png'), o['current_points'][batch_idx], rescale=False)
                        _save_img_sequence(osp.join(d, 'real_seq'), real[batch_idx], rescale=True)
                        _save_img_sequence(osp.join(d, 'pred_seq'), o['pred_im_seq'][batch_idx], rescale=True)
                        _save_img_sequence(osp.join(d, 'mask'), o['mask'][batch_idx], rescale=False)
                        _save_img_sequence(osp.join(d, 'crude'), o['pred_im_crude'][batch_idx], rescale=True)
                        _save_img_sequence(osp.join(d, 'pred_points'), o['future_points'][batch_idx], rescale=False)
                        sample_idx += 1
                    for anim in animations:     # before the driven rollouts and the sweep below replay the graph over these outputs
                        anim.write(args.save_dir, sample_idx - bsz, [('real', batch['image'], batch['real_im_seq'], 'unit'),
                                                                     ('pred', outputs['im'], outputs['pred_im_seq'], 'unit'),
                                                                     ('points', outputs['current_points'], outputs['future_points'], 'raw')])
                if posterior is not None and draw == 0:
                    posterior.own_draw0(outputs)
                if drive_modes and draw == 0:    # once per batch: the driven rollouts do not depend on z (their graphs are their own:
                    # this draw's own outputs stay), before the sweep replays the own rollout's graph
                    first = sample_idx - bsz if not args.no_save else 0
                    driven = _Drive(kpx_amd, model, drive_modes, args.drive_scaled, sheet_frames, batch, True, not args.no_save, dev)
                    if not args.no_save:
                        driven.paste('model', driven.image, outputs['pred_im_seq'].contiguous())
                    frames += driven.run(args.save_dir, first, real_flat if args.metrics else None, drive_scores)
                    if not args.no_save:
                        driven.write_sheet(args.save_dir, first)
                    n_self_driven += bsz if 'transfer' in drive_modes and bsz == 1 else 0
                if sweep is not None:        # after everything that reads this draw's own rollout: the sweep replays the same graph
                    frames += sweep.run(draw, z)
                    if draw == 0 and not args.no_save:
                        sweep.write_sheets(args.save_dir, sample_idx - bsz)
                    if draw == args.samples - 1 and args.metrics:
                        sweep.scores(action_scores)
            if novelty is not None:
                novelty.end_batch(args.save_dir, n_read - bsz)
            if long_run is not None:         # after everything of the ordinary rollout: its own graph, its own files
                frames += long_run.run(args.save_dir, sample_idx - bsz, batch['image'], batch['action_code'], z_first)
            if posterior is not None:        # last: its rollouts replay the ordinary rollout's graph, whose outputs are all consumed by now
                frames += posterior.end_batch(args.save_dir, sample_idx - bsz if not args.no_save else 0, batch, real_flat if args.metrics else None)
        torch.cuda.synchronize()
        print('iteration through test set finished: %d predicted frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))
        if actions and not args.no_save:
            _write_actions_json(args.save_dir, actions, sheet_frames, True, (model.image_size, model.image_size))
        if drive_modes and not args.no_save:
            _write_drive_json(args.save_dir, _drive_rows(drive_modes, True, not args.drive_only), sheet_frames,
                              (model.image_size, model.image_size), drive_modes, args.drive_scaled, n_self_driven)
        for anim in animations:
            anim.write_json(args.save_dir)
        if long_run is not None:
            long_run.write_json(args.save_dir)
        if args.metrics and args.drive_only:
            _write_drive_only_metrics(args.save_dir, drive_scores, n_frames)
        elif args.metrics:
            _write_metrics(args.save_dir, scores, args.samples, n_frames, vgg_scores, motion_scores, action_scores, drive_scores, frechet,
                           accuracy, novelty, prdc, posterior)
        elif posterior is not None:          # without --metrics: posterior.npz and the printed line; the block is python -m kpx_amd.posterior's
            print(_Posterior.line(posterior.finish(args.save_dir, n_frames)[1]))
        return
    for start in range(0, args.synthetic, args.batch):
        bsz = min(args.batch, args.synthetic - start)
        rs = np.random.RandomState(start)
        im = (rs.randint(0, 256, size=(bsz, size, size, 3)).astype(np.float32) / 255.0 * 2.0 - 1.0)
        act = np.eye(n_action, dtype=np.float32)[rs.randint(0, n_action, size=bsz)]
        image = torch.from_numpy(im).to(dev)
        if args.drive_only:                  # hold alone, without the model's own rollout
            if not args.no_save:
                for batch_idx in range(bsz):
                    d = osp.join(args.save_dir, '%04d' % (sample_idx + batch_idx))
                    os.makedirs(d, exist_ok=True)
                    _save_img(osp.join(d, 'input_im.png'), im[batch_idx], rescale=True)
            driven = _Drive(kpx_amd, model, drive_modes, False, sheet_frames, {'image': image, 'action_code': torch.from_numpy(act).to(dev)},
                            False, not args.no_save, dev)
            frames += driven.run(args.save_dir, sample_idx, None, None)
            if not args.no_save:
                driven.write_sheet(args.save_dir, sample_idx)
            for anim in animations:
                o = driven.first_out
                anim.write(args.save_dir, sample_idx, [('pred', image, o['pred_im_seq'], 'unit'),
                                                       ('points', o['current_points'], o['future_points'], 'raw')])
            sample_idx += bsz
            continue
        z = torch.randn((bsz, model.vae_dim), device=dev) if actions or long_run is not None else None   # --actions: shared with the sweep below
        outputs = model.run(None, {'image': image, 'action_code': torch.from_numpy(act).to(dev)}, z=z)
        frames += bsz * 32
        if not args.no_save:
            o = {k: v.cpu().numpy() for k, v in outputs.items() if isinstance(v, torch.Tensor)}
            for batch_idx in range(bsz):
                d = osp.join(args.save_dir, '%04d' % sample_idx)
                os.makedirs(d, exist_ok=True)
                _save_img(osp.join(d, 'input_im.png'), o['im'][batch_idx], rescale=True)
                _save_img(osp.join(d, 'current_points.png'), o['current_points'][batch_idx], rescale=False)
                _save_img_sequence(osp.join(d, 'pred_seq'), o['pred_im_seq'][batch_idx], rescale=True)
                _save_img_sequence(osp.join(d, 'mask'), o['mask'][batch_idx], rescale=False)
                _save_img_sequence(osp.join(d, 'crude'), o['pred_im_crude'][batch_idx], rescale=True)
                _save_img_sequence(osp.join(d, 'pred_points'), o['future_points'][batch_idx], rescale=False)
                sample_idx += 1
            for anim in animations:
                anim.write(args.save_dir, sample_idx - bsz, [('pred', outputs['im'], outputs['pred_im_seq'], 'unit'),
                                                             ('points', outputs['current_points'], outputs['future_points'], 'raw')])
        if drive_modes:
            first = sample_idx - bsz if not args.no_save else 0
            driven = _Drive(kpx_amd, model, drive_modes, False, sheet_frames, {'image': image, 'action_code': torch.from_numpy(act).to(dev)},
                            True, not args.no_save, dev)
            if not args.no_save:
                driven.paste('model', driven.image, outputs['pred_im_seq'].contiguous())
            frames += driven.run(args.save_dir, first, None, None)
            if not args.no_save:
                driven.write_sheet(args.save_dir, first)
        if actions:
            sweep = _ClassSweep(kpx_amd, model, actions, n_action, sheet_frames, image, None, not args.no_save, 1, None, dev)
            frames += sweep.run(0, z)
            if not args.no_save:
                sweep.write_sheets(args.save_dir, sample_idx - bsz)
        if long_run is not None:
            frames += long_run.run(args.save_dir, sample_idx - bsz, image, torch.from_numpy(act).to(dev), z)
    if actions and not args.no_save:
        _write_actions_json(args.save_dir, actions, sheet_frames, False, (model.image_size, model.image_size))
    if drive_modes and not args.no_save:
        _write_drive_json(args.save_dir, _drive_rows(drive_modes, False, not args.drive_only), sheet_frames,
                          (model.image_size, model.image_size), drive_modes, False, 0)
    for anim in animations:
        anim.write_json(args.save_dir)
    if long_run is not None:
        long_run.write_json(args.save_dir)
    torch.cuda.synchronize()
    print('iteration through synthetic set finished: %d predicted frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))


if __name__ == '__main__':
    main()
