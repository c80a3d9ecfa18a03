#!/usr/bin/env python3
"""Evaluation entry point with the reference's CLI (reference: evaluate.py:13-163):

    python evaluate.py --config configs/penn.yaml --checkpoint_stage1 S1.npz --checkpoint_stage2 S2.npz [--save_dir results/eval]
                       [--synthetic N] [--colors_seed S] [--no-save]
                       [--metrics [--samples N] [--vgg-metrics [--synthetic-vgg]] [--motion-metrics]]

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

``--motion-metrics`` (with ``--metrics``; at most 4096 ``--samples``) adds what needs no network: ``kp_l2`` [samples, draws, 32], the mean
distance of each draw's predicted key points to the pseudo labels of the real frames (``kpx_amd.ops.keypoint_draw_metrics``), and with
``--samples`` >= 2 how far the draws lie apart: ``kp_div`` [samples, 32] in key-point space and ``div_mse`` [samples, 32], the mean over
pairs of draws of the MSE between their 8-bit frames (``draw_moments_add`` per draw, ``draw_diversity`` per batch: exact integers), plus
per sample ``pred_std/``, the per-pixel spread of the draws as 8-bit grey PNGs.  Blocks of the same names in metrics.json.
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


def _write_metrics(save_dir, scores, n_draws, n_frames, vgg_scores=None, motion_scores=None):
    """scores: per batch a device tensor [draws, B * T, 3] = (ssim, mse, psnr); one copy to the host for all of them.
    vgg_scores (--vgg-metrics): per batch a device tensor [draws, B * T, 5, 2] = per layer (cos_layer, l1_layer).
    motion_scores (--motion-metrics): {'kp_l2': per batch [draws, B, T]} and for two or more draws {'kp_div': per batch [B, T], 'div_mse':
    per batch [B * T]}."""
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
    os.makedirs(save_dir, exist_ok=True)
    np.savez(osp.join(save_dir, 'metrics.npz'), **arrays)
    res = summarise_metrics(ssim, psnr, mse, extras=extras, motion=motion)
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
    if motion is not None:
        line += ', key-point L2 %s (best of draws %s)' % (fmt(res['kp_l2']['mean'], '%.4f'), fmt(res['kp_l2']['best_of_draws'], '%.4f'))
        if 'kp_div' in res:
            line += ', key-point diversity %s, draw diversity MSE %s' % (fmt(res['kp_div']['mean'], '%.4f'), fmt(res['div_mse']['mean'], '%.3e'))
    print('%s; %d non-finite frames' % (line, res['n_nonfinite']))


def _save_img_sequence(output_dir, img_seq, rescale=False, raw=False):
    """reference :151-156"""
    os.makedirs(output_dir, exist_ok=True)
    for i in range(img_seq.shape[0]):
        _save_img(osp.join(output_dir, '%06d.png' % i), img_seq[i], rescale=rescale, raw=raw)


def main(argv=None):
    from train import load_config
    parser = ArgumentParser()
    parser.add_argument('--config', type=str, required=True, help='path of the configuration file')
    parser.add_argument('--checkpoint_stage1', type=str, required=True, help='path of the stage1 checkpoint')
    parser.add_argument('--checkpoint_stage2', type=str, required=True, help='path of the stage2 checkpoint')
    parser.add_argument('--save_dir', type=str, required=False, help='root dir to save results', default='results/eval')
    parser.add_argument('--synthetic', type=int, default=0)
    parser.add_argument('--batch', type=int, default=8)             # reference :27
    parser.add_argument('--colors_seed', type=int, default=0, help='seed of the key-point palette (the reference draws it unseeded)')
    parser.add_argument('--no-save', action='store_true')
    parser.add_argument('--metrics', action='store_true', help='score the predictions: <save_dir>/metrics.npz and metrics.json')
    parser.add_argument('--samples', type=int, default=1, help='rollouts per batch with fresh z (PNGs from the first)')
    parser.add_argument('--vgg-metrics', action='store_true',
                        help='with --metrics: VGG19 feature-space cosine similarity and perceptual L1 per predicted frame (paths.vggnet)')
    parser.add_argument('--synthetic-vgg', action='store_true', help='He-normal VGG19 weights when paths.vggnet is absent')
    parser.add_argument('--motion-metrics', action='store_true',
                        help='with --metrics: key-point error against the pseudo labels and, for --samples >= 2, the diversity of the draws')
    args = parser.parse_args(argv)
    if args.vgg_metrics and not args.metrics:
        parser.error('--vgg-metrics adds to the scores of --metrics and needs it')
    if args.motion_metrics and not args.metrics:
        parser.error('--motion-metrics adds to the scores of --metrics and needs it')
    if args.motion_metrics and args.samples > MAX_MOTION_DRAWS:
        parser.error('--motion-metrics holds at most %d --samples in its exact accumulators (got %d)' % (MAX_MOTION_DRAWS, args.samples))
    if args.metrics and args.synthetic:
        parser.error('--metrics scores predictions against the real future frames, and --synthetic inputs have no ground truth')
    if args.samples < 1:
        parser.error('--samples must be >= 1 (got %d)' % args.samples)
    config = load_config(args.config)
    for p in (args.checkpoint_stage1, args.checkpoint_stage2):       # reference :34-38
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
    model = kpx_amd.FinalModel(config, device=dev, point_maps=not args.no_save, colors_seed=args.colors_seed)
    print('model initialized')
    model.build(None)
    model.restore(None, args.checkpoint_stage1)                      # reference :76-77: two partial restores by name
    model.restore(None, args.checkpoint_stage2)
    n_action = config['model']['n_action']
    sample_idx, frames, t0 = 0, 0, time.time()
    if not args.synthetic:                       # reference :43-51, :84-130: the test subset through the sequence loader
        loader = kpx_amd.data.SequenceDataLoader(config['paths']['data_dir'], 'test', n_points=config['model']['n_pts'], n_action=n_action,
                                                 random_order=False, randomness=False, with_image_seq=True)
        scores, n_frames = [], 32
        vgg_scores = [] if args.vgg_metrics else None
        motion_scores = None
        if args.motion_metrics:
            motion_scores = {'kp_l2': []} if args.samples < 2 else {'kp_l2': [], 'kp_div': [], 'div_mse': []}
        for batch in loader.batches(args.batch, dev, repeat=False, num_preprocess_threads=12):
            bsz = batch['image'].shape[0]
            if args.metrics:
                real_seq = batch['real_im_seq']
                n_frames = real_seq.shape[1]
                real_flat = real_seq.reshape(bsz * n_frames, *real_seq.shape[2:])
                score = torch.empty((args.samples, bsz * n_frames, 3), dtype=torch.float32, device=dev)
                scores.append(score)
                if args.vgg_metrics:         # the real frames' features once per batch, reused by every draw
                    scorer = kpx_amd.FeatureScorer(vgg, real_flat)
                    vgg_score = torch.empty((args.samples, bsz * n_frames, len(VGG_FEATURE_LAYERS), 2), dtype=torch.float32, device=dev)
                    vgg_scores.append(vgg_score)
                if args.motion_metrics:      # every draw's key points, and two integer accumulators per value of the predicted frames
                    kp_real = batch['real_seq'].contiguous()
                    kp_pred = torch.empty((args.samples,) + tuple(kp_real.shape), dtype=torch.float32, device=dev)
                    if args.samples >= 2:
                        moments = torch.empty((2, real_flat.numel()), dtype=torch.int32, device=dev)
                        kpx_amd.ops.fill_raw_(moments, 0.0)
            for draw in range(args.samples):
                outputs = model.run(None, {'image': batch['image'], 'action_code': batch['action_code']})
                frames += bsz * 32
                if args.metrics:             # enqueued before the next run() overwrites the graph's output buffers
                    pred = outputs['pred_im_seq']
                    pred_flat = pred.reshape(bsz * n_frames, *pred.shape[2:])
                    kpx_amd.ops.frame_metrics(pred_flat, real_flat, png8=True, out=score[draw])
                    if args.vgg_metrics:
                        scorer(pred_flat, out=vgg_score[draw])
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
                if draw > 0 or args.no_save:
                    continue
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
        torch.cuda.synchronize()
        print('iteration through test set finished: %d predicted frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))
        if args.metrics:
            _write_metrics(args.save_dir, scores, args.samples, n_frames, vgg_scores, motion_scores)
        return
    for start in range(0, args.synthetic, args.batch):
        bsz = min(args.batch, args.synthetic - start)
        rs = np.random.RandomState(start)
        im = (rs.randint(0, 256, size=(bsz, 128, 128, 3)).astype(np.float32) / 255.0 * 2.0 - 1.0)
        act = np.eye(n_action, dtype=np.float32)[rs.randint(0, n_action, size=bsz)]
        outputs = model.run(None, {'image': torch.from_numpy(im).to(dev), 'action_code': torch.from_numpy(act).to(dev)})
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
    torch.cuda.synchronize()
    print('iteration through synthetic set finished: %d predicted frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))


if __name__ == '__main__':
    main()
