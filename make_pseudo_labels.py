#!/usr/bin/env python3
"""Pseudo-label writer with the reference's CLI (reference: make_pseudo_labels.py:12-105):

    python make_pseudo_labels.py --config configs/penn.yaml --checkpoint results/detector_translator/model.ckpt-N.npz [--synthetic V]
                                 [--stability [--stability-warps W] [--stability-seed S] [--stability-sheets] [--colors_seed C]]

For every video writes ``<data_dir>/pseudo_labels/NNNN.npy`` = float32 [len, K, 2] key-points (reference :98-101).  Videos come
from the train and test subsets of ``paths.data_dir`` through kpx_amd.data.KeypointDataLoader (the reference's
data/keypoint_dataloader.py); ``--synthetic V`` feeds V random videos padded to 663 frames with the loader's output contract
({'image': [1,663,128,128,3] in [-1,1], 'idx', 'len'}) instead.

``--stability`` (not in the reference) also scores the detector that writes the labels, without annotations: every
frame of a video is moved by W random similarity maps (``kpx_amd.stability.draw_warps``, seeded by S, the subset and the video number),
detected again, and the detected points are compared with the mapped originals (``KeypointModel.stability``: the warp and the score are HIP
kernels, the cost is the W extra detector passes).  The labels written are the same bytes with and without the flag.  The report goes to
``<paths.log_dir>/stability/`` -- not into pseudo_labels/, which the loaders enumerate: ``stability.json`` (``summarise_stability``: the
mean error ``equiv``, the mean distance the maps moved the points, their ``ratio`` -- 0: the points follow the map, 1: the detector ignores
the image --, per key point, per subset and overall; this project's own quantity, not comparable with published figures) and
``stability.npz`` (per video: subset, idx, err, moved, n_valid, n_total).  ``--stability-sheets`` adds ``sheets/NNNN.png`` per video for its
first frame: one row per map of frame | warped frame | point map of the detector on the warped frame | point map of the expected points,
in the palette of ``random.Random(--colors_seed)``.
"""
import json
import os
import random
import sys
import time
from argparse import ArgumentParser
from os import path as osp

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
MAX_FRAMES = 663                       # reference data/keypoint_dataloader.py:13


def _save_output(keypoints_root_dir, outputs):
    """reference :98-101"""
    idx, n = int(outputs['idx'][0]), int(outputs['len'][0])
    np.save(osp.join(keypoints_root_dir, '{:04d}.npy'.format(idx)), outputs['pts'][0, :n].cpu().numpy())


class _Stability:
    """--stability: scores every video after its labels are written and writes the report (module docstring)."""

    def __init__(self, model, config, args, dev):
        from kpx_amd import model_utils, ops, stability
        self.model, self.ops, self.lib, self.dev = model, ops, stability, dev
        self.warps, self.seed, self.sheets = args.stability_warps, args.stability_seed, args.stability_sheets
        self.dir = osp.join(config['paths']['log_dir'], 'stability')
        os.makedirs(osp.join(self.dir, 'sheets') if self.sheets else self.dir, exist_ok=True)
        self.colors = torch.tensor(model_utils.get_n_colors(model.n_points, rng=random.Random(args.colors_seed)), dtype=torch.float32, device=dev)
        self.subsets, self.records = [], []

    def video(self, subset, frames, pts, idx, n):
        """frames [>= n, R, R, 3] and pts [>= n, K, 2] of video ``idx``; its first n frames are scored."""
        if subset not in self.subsets:
            self.subsets.append(subset)
        coef, fwd = self.lib.draw_warps(n, self.warps, seed=[self.seed, self.subsets.index(subset), idx], res=self.model.image_size)
        out = self.model.stability(frames[:n], coef, fwd, pts=pts[:n])
        self.records.append(self.lib.video_record(subset, idx, *(out[key].cpu().numpy() for key in ('scores', 'valid', 'frame_mean', 'n_valid'))))
        if self.sheets:
            self._sheet(frames[:1].contiguous(), coef[0], fwd[0], out, idx)

    def _sheet(self, frame, coef, fwd, out, idx):
        from PIL import Image
        ops, r, w = self.ops, self.model.image_size, self.warps
        warped = ops.affine_warp(frame, torch.zeros(w, dtype=torch.int32, device=self.dev), torch.from_numpy(coef).to(self.dev))
        p = out['pts'][0].cpu().numpy().astype(np.float64)                                  # [K,2]; the expected points in float64, rounded once
        target = np.stack([(fwd[:, None, 0] * p[None, :, 0] + fwd[:, None, 1] * p[None, :, 1]) + fwd[:, None, 2],
                           (fwd[:, None, 3] * p[None, :, 0] + fwd[:, None, 4] * p[None, :, 1]) + fwd[:, None, 5]], axis=-1).astype(np.float32)
        cells = ((frame, 'unit'), (warped, 'unit'), (ops.point_maps_rgb(out['pts_w'][0].contiguous(), r, r, self.colors), 'raw'),
                 (ops.point_maps_rgb(torch.from_numpy(target).to(self.dev), r, r, self.colors), 'raw'))
        canvas = torch.zeros((1, w * r, len(cells) * r, 3), dtype=torch.uint8, device=self.dev)
        for j in range(w):
            for col, (src, premap) in enumerate(cells):
                ops.sheet_paste(canvas, src.unsqueeze(0), [j if col else 0], j, col, premap)
        Image.fromarray(canvas[0].cpu().numpy()).save(osp.join(self.dir, 'sheets', '{:04d}.png'.format(idx)))

    def finish(self):
        S = self.lib
        draw = {'warps': self.warps, 'seed': self.seed, 'rot_deg': S.DEFAULT_ROT_DEG, 'log_scale': S.DEFAULT_LOG_SCALE, 'shift': S.DEFAULT_SHIFT}
        summary = S.summarise_stability(self.records, self.model.image_size, draw)
        with open(osp.join(self.dir, 'stability.json'), 'w') as f:
            json.dump(S.jsonable(summary), f, indent=1, allow_nan=False)
        np.savez(osp.join(self.dir, 'stability.npz'), **S.per_video_arrays(self.records))
        o = summary['overall']
        print('stability (own quantity, not comparable with published figures): equiv %.5f (%.3f px), moved %.5f, ratio %.4f, valid %.3f '
              'over %d videos -> %s' % (o['equiv'], o['equiv_px'], o['moved'], o['ratio'], o['valid_fraction'], o['videos'], self.dir))


def main(argv=None):
    from train import load_config
    parser = ArgumentParser()
    parser.add_argument('--config', type=str, required=True, help='path of the configuration file')
    parser.add_argument('--checkpoint', type=str, required=True, help='path of the pretrained keypoints detector')
    parser.add_argument('--synthetic', type=int, default=0, help='number of synthetic videos instead of paths.data_dir')
    parser.add_argument('--frames', type=int, default=MAX_FRAMES)
    parser.add_argument('--stability', action='store_true',
                        help="also score the detector's equivariance under random similarity maps into <paths.log_dir>/stability/ (this "
                             "project's own quantity, not comparable with published figures)")
    parser.add_argument('--stability-warps', type=int, default=None, help='maps drawn per frame (default 2)')
    parser.add_argument('--stability-seed', type=int, default=None, help='seed of the maps (default 0)')
    parser.add_argument('--stability-sheets', action='store_true', help='one contact sheet per video for its first frame')
    parser.add_argument('--colors_seed', type=int, default=0, help="seed of the sheets' key-point palette")
    args = parser.parse_args(argv)
    if not args.stability and (args.stability_warps is not None or args.stability_seed is not None or args.stability_sheets):
        parser.error('--stability-warps, --stability-seed and --stability-sheets belong to --stability')
    if args.stability_warps is not None and args.stability_warps < 1:
        parser.error('--stability-warps must be >= 1 (got %d)' % args.stability_warps)
    if args.stability_seed is not None and not 0 <= args.stability_seed < 2 ** 32:
        parser.error('--stability-seed must lie in [0, 2^32) (got %d)' % args.stability_seed)
    if args.stability_sheets and args.stability_warps is not None and args.stability_warps > 64:
        parser.error('--stability-sheets draws one row per map: at most 64 (got --stability-warps %d)' % args.stability_warps)
    config = load_config(args.config)
    keypoints_root_dir = osp.join(config['paths']['data_dir'], 'pseudo_labels')
    os.makedirs(keypoints_root_dir, exist_ok=True)
    if not (osp.exists(args.checkpoint) or osp.exists(args.checkpoint + '.index')):      # .npz file or TensorFlow bundle prefix
        raise Exception('checkpoint not found at %s' % args.checkpoint)          # reference :31-32
    import kpx_amd
    dev = torch.device('cuda', 0)
    model = kpx_amd.KeypointModel(config, device=dev)
    print('model initialized')
    model.build(None)
    restored = model.restore(None, args.checkpoint)
    print('restored %d arrays' % len(restored))
    stab = None
    if args.stability:
        args.stability_warps = 2 if args.stability_warps is None else args.stability_warps      # = kpx_amd.stability.DEFAULT_WARPS
        args.stability_seed = args.stability_seed or 0
        stab = _Stability(model, config, args, dev)
    t0, frames = time.time(), 0
    if not args.synthetic:                       # reference :36-37, :79-95: every video of the train and the test subset
        data_dir = config['paths']['data_dir']
        for subset in ('train', 'test'):
            for v in kpx_amd.data.KeypointDataLoader(data_dir, subset).videos(dev):
                outputs = model.run(None, {'image': v['image'][None], 'idx': np.array([v['idx']]), 'len': np.array([v['len']])})
                _save_output(keypoints_root_dir, outputs)
                if stab:
                    stab.video(subset, v['image'], outputs['pts'][0], int(v['idx']), int(v['len']))
                frames += v['len']
            print('iteration through %s set finished' % subset)
        torch.cuda.synchronize()
        print('%d frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))
        if stab:
            stab.finish()
        return
    for v in range(args.synthetic):
        rs = np.random.RandomState(v)
        n = int(rs.randint(args.frames // 4, args.frames + 1))
        im = np.zeros((1, args.frames, 128, 128, 3), np.float32)
        im[0, :n] = (rs.randint(0, 256, size=(n, 128, 128, 3)).astype(np.float32) / 255.0 * 2.0 - 1.0)
        outputs = model.run(None, {'image': torch.from_numpy(im).to(dev), 'idx': np.array([v]), 'len': np.array([n])})
        _save_output(keypoints_root_dir, outputs)
        if stab:
            stab.video('synthetic', outputs['im'][0], outputs['pts'][0], v, n)
        frames += args.frames
    torch.cuda.synchronize()
    print('iteration through synthetic set finished: %d frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))
    if stab:
        stab.finish()


if __name__ == '__main__':
    main()
