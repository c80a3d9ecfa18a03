#!/usr/bin/env python3
"""Pseudo-label writer with the reference's CLI (reference: make_pseudo_labels.py:12-105):

    python make_pseudo_labels.py --config configs/penn.yaml --checkpoint results/detector_translator/model.ckpt-N.npz [--synthetic V]
                                 [--stability [--stability-warps W] [--stability-seed S] [--stability-sheets] [--colors_seed C]]
                                 [--joints [--joints-dir DIR] [--joints-ridge L] [--joints-pck 0.05,0.1,0.2] [--joints-norm bbox|image]
                                  [--joints-sheets]]

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

``--joints`` (not in the reference) asks whether the K points carry the body's pose: landmark regression, the usual
measure of an unsupervised key-point detector.  Penn Action's annotations (``<data_dir>/labels/NNNN.mat``, or ``--joints-dir``: 13 joints,
a visibility flag and a box per frame) are taken into the crop's coordinates (``kpx_amd.joints.crop_map``), a linear map from the detected
points to the joints is fitted per joint on the train subset (ridge ``--joints-ridge``, default 1e-6, the bias not penalised) and both
subsets are scored by it: the mean error and PCK at the ``--joints-pck`` thresholds (default 0.05,0.1,0.2; at most 8, each in (0, 1]) of
the normaliser ``--joints-norm``: ``bbox`` (default) the longer side of the frame's annotated box, ``image`` the side of the crop.
The points of every video stay on the device until the end, so there is no second detector pass (``kpx_amd.joints.JointRegression``: three
HIP launches per video).  The labels written are the same bytes with and without the flag.  A video without a label file is counted and
listed under ``missing``; no label file at all is an error before the first video.  The report goes to ``<paths.log_dir>/joints/``:
``joints.json`` (``kpx_amd.joints.summarise``: overall, per subset and per joint; the note says what the figures are comparable with),
``joints.npz`` (W, G, Bm, n, K, J, alphas, norm, ridge and per video subset, idx, frames, err, count, pck_count: the file a later
evaluate.py flag can load to reach annotated pose space) and with ``--joints-sheets`` ``sheets/NNNN.png`` per video for its first frame:
frame | point map of the annotated joints | point map of the regressed joints (joints that are not scored are not drawn), in a J-colour
palette of ``random.Random(--colors_seed)``.  With ``--synthetic V`` the annotations are planted (``kpx_amd.joints.planted_labels`` from
``RandomState([0, v])``, even videos train, odd videos test) and the report is marked ``"synthetic": true``: it exercises the path, its
scores mean nothing.
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


JOINTS_DEFAULT_PCK, JOINTS_DEFAULT_RIDGE = '0.05,0.1,0.2', 1e-6      # = kpx_amd.joints.DEFAULT_ALPHAS, DEFAULT_RIDGE (tests/test_joints_cpu.py holds them equal)
SYNTHETIC_JOINTS, SYNTHETIC_JOINTS_SEED = 13, 0      # --synthetic with --joints: Penn Action's joint count, planted from [seed, v]


class _Joints:
    """--joints: collects every video after its labels are written, fits and scores at the end and writes the report (module docstring)."""

    def __init__(self, model, config, args, dev, labels_dir):
        from kpx_amd import joints, model_utils, ops
        self.model, self.ops, self.lib, self.dev, self.args, self.labels_dir = model, ops, joints, dev, args, labels_dir
        self.model_utils = model_utils
        self.dir = osp.join(config['paths']['log_dir'], 'joints')
        os.makedirs(osp.join(self.dir, 'sheets') if args.joints_sheets else self.dir, exist_ok=True)
        self.reg, self.missing, self.frames = None, [], []

    def _regression(self, n_joints):
        if self.reg is None:
            a = self.args
            self.reg = self.lib.JointRegression(self.model.n_points, n_joints, alphas=a.joints_pck, norm=a.joints_norm, ridge=a.joints_ridge,
                                                device=self.dev, res=self.model.image_size)
        return self.reg

    def require_labels(self, video_ids):
        """No label file for any of the videos is an error, before the first video is read."""
        if not any(self.lib.find_label_file(self.labels_dir, v) for v in video_ids):
            raise Exception('--joints: no label file (NNNN.mat or NNNN.npz) for any of the %d videos under %s' % (len(video_ids), self.labels_dir))

    def video(self, subset, frames, pts, idx, n, frame_size, labels=None):
        """pts [>= n, K, 2] of video ``idx``, frames [>= n, R, R, 3] (the first is kept for the sheet), the original frames' (w, h)."""
        if labels is None:
            path = self.lib.find_label_file(self.labels_dir, idx)
            if path is None:
                self.missing.append(int(idx))
                return
            labels = self.lib.read_labels(path, n_frames=n)
        self._regression(labels['x'].shape[1]).add(subset, idx, pts[:n], labels, frame_size)
        self.frames.append(frames[:1].clone() if self.args.joints_sheets else None)

    def _sheet(self, frame, first, idx, colors):
        from PIL import Image
        ops, r = self.ops, self.model.image_size
        target, mask, pred = first
        shown = np.where(mask[:, None] != 0, 1.0, np.nan)
        cells = [(frame, 'unit')]
        for p in (target, pred):                     # a joint that is not scored sits far outside the frame: its Gaussian is 0 everywhere
            mu = np.where(np.isfinite(p * shown), p, -4.0).astype(np.float32)
            cells.append((ops.point_maps_rgb(torch.from_numpy(mu[None]).to(self.dev), r, r, colors), 'raw'))
        canvas = torch.zeros((1, r, len(cells) * r, 3), dtype=torch.uint8, device=self.dev)
        for col, (src, premap) in enumerate(cells):
            ops.sheet_paste(canvas, src.unsqueeze(0).contiguous(), [0], 0, col, premap)
        Image.fromarray(canvas[0].cpu().numpy()).save(osp.join(self.dir, 'sheets', '{:04d}.png'.format(idx)))

    def finish(self, synthetic):
        L, a = self.lib, self.args
        if self.reg is None:
            raise Exception('--joints: none of the videos had a label file under %s' % self.labels_dir)
        out = self.reg.finish()
        summary = dict(out['summary'], missing=sorted(set(self.missing)), synthetic=bool(synthetic))
        with open(osp.join(self.dir, 'joints.json'), 'w') as f:
            json.dump(L.jsonable(summary), f, indent=1, allow_nan=False)
        np.savez(osp.join(self.dir, 'joints.npz'), W=out['W'], G=out['G'], Bm=out['Bm'], n=out['n'], K=np.int64(self.reg.k), J=np.int64(self.reg.j),
                 alphas=np.array(self.reg.alphas, np.float64), norm=np.array(a.joints_norm), ridge=np.float64(a.joints_ridge),
                 **L.per_video_arrays(out['records']))
        if a.joints_sheets:
            colors = torch.tensor(self.model_utils.get_n_colors(self.reg.j, rng=random.Random(a.colors_seed)), dtype=torch.float32, device=self.dev)
            for rec, frame, first in zip(out['records'], self.frames, out['first']):
                self._sheet(frame, first, rec['idx'], colors)
        subsets = summary['subsets']
        name = 'test' if 'test' in subsets else next(iter(subsets))
        s = subsets[name]
        print('joints (landmark regression; %s): %s err %.5f (%.3f px), PCK %s, valid %.3f over %d videos, %d without labels -> %s'
              % ('synthetic annotations, the scores mean nothing' if synthetic else "this project's crop, normaliser and joint set", name,
                 s['err'], s['err_px'], ' '.join('@%g %.4f' % (al, v) for al, v in zip(summary['alphas'], s['pck'])), s['valid_fraction'],
                 summary['overall']['videos'], len(summary['missing']), self.dir))


def main(argv=None):
    from train import IMAGE_SIZE_HELP, config_image_size, load_config
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
    parser.add_argument('--image-size', type=int, default=None, metavar='S', help=IMAGE_SIZE_HELP)
    parser.add_argument('--joints', action='store_true',
                        help='also regress the annotated joints from the key points (fit on train, error and PCK per subset) into '
                             "<paths.log_dir>/joints/ (comparable across this project's checkpoints)")
    parser.add_argument('--joints-dir', type=str, default=None, help='directory of the NNNN.mat label files (default <data_dir>/labels)')
    parser.add_argument('--joints-ridge', type=float, default=None, help='ridge of the regression (default 1e-6)')
    parser.add_argument('--joints-pck', type=str, default=None, help='PCK thresholds, comma separated, at most 8 in (0, 1] (default 0.05,0.1,0.2)')
    parser.add_argument('--joints-norm', type=str, default=None, choices=('bbox', 'image'), help='PCK normaliser (default bbox)')
    parser.add_argument('--joints-sheets', action='store_true', help='one contact sheet per video for its first frame')
    parser.add_argument('--ema', action='store_true',
                        help="read the checkpoint under its averaged weights (train.py --ema: the <name>/ExponentialMovingAverage entries take their variables' places); a checkpoint without them is refused")
    args = parser.parse_args(argv)
    if not args.joints and (args.joints_dir is not None or args.joints_ridge is not None or args.joints_pck is not None
                            or args.joints_norm is not None or args.joints_sheets):
        parser.error('--joints-dir, --joints-ridge, --joints-pck, --joints-norm and --joints-sheets belong to --joints')
    if args.joints:
        if args.joints_ridge is not None and not args.joints_ridge >= 0:
            parser.error('--joints-ridge must be >= 0 (got %r)' % args.joints_ridge)
        try:
            alphas = [float(v) for v in (args.joints_pck if args.joints_pck is not None else JOINTS_DEFAULT_PCK).split(',')]
        except ValueError:
            parser.error('--joints-pck must be comma-separated numbers (got %r)' % args.joints_pck)
        if len(alphas) > 8:
            parser.error('--joints-pck takes at most 8 thresholds (got %d)' % len(alphas))
        if any(not 0.0 < v <= 1.0 for v in alphas):
            parser.error('--joints-pck: every threshold must lie in (0, 1] (got %r)' % args.joints_pck)
        args.joints_pck = alphas
        args.joints_ridge = JOINTS_DEFAULT_RIDGE if args.joints_ridge is None else args.joints_ridge
        args.joints_norm = args.joints_norm or 'bbox'
    if not args.stability and (args.stability_warps is not None or args.stability_seed is not None or args.stability_sheets):
        parser.error('--stability-warps, --stability-seed and --stability-sheets belong to --stability')
    if args.stability_warps is not None and args.stability_warps < 1:
        parser.error('--stability-warps must be >= 1 (got %d)' % args.stability_warps)
    if args.stability_seed is not None and not 0 <= args.stability_seed < 2 ** 32:
        parser.error('--stability-seed must lie in [0, 2^32) (got %d)' % args.stability_seed)
    if args.stability_sheets and args.stability_warps is not None and args.stability_warps > 64:
        parser.error('--stability-sheets draws one row per map: at most 64 (got --stability-warps %d)' % args.stability_warps)
    config = load_config(args.config)
    size = config_image_size(config, args.image_size)
    keypoints_root_dir = osp.join(config['paths']['data_dir'], 'pseudo_labels')
    os.makedirs(keypoints_root_dir, exist_ok=True)
    if not (osp.exists(args.checkpoint) or osp.exists(args.checkpoint + '.index')):      # .npz file or TensorFlow bundle prefix
        raise Exception('checkpoint not found at %s' % args.checkpoint)          # reference :31-32
    import kpx_amd
    dev = torch.device('cuda', 0)
    model = kpx_amd.KeypointModel(config, device=dev, image_size=size)
    print('model initialized')
    model.build(None)
    restored = model.restore(None, args.checkpoint, **({'ema': True} if args.ema else {}))
    print('restored %d arrays' % len(restored))
    stab = None
    if args.stability:
        args.stability_warps = 2 if args.stability_warps is None else args.stability_warps      # = kpx_amd.stability.DEFAULT_WARPS
        args.stability_seed = args.stability_seed or 0
        stab = _Stability(model, config, args, dev)
    joints = None
    if args.joints:
        joints = _Joints(model, config, args, dev, args.joints_dir or osp.join(config['paths']['data_dir'], 'labels'))
    t0, frames = time.time(), 0
    if not args.synthetic:                       # reference :36-37, :79-95: every video of the train and the test subset
        data_dir = config['paths']['data_dir']
        if joints:                               # both listings are read up front only here: no label file at all ends the run before the first video
            joints.require_labels([v for subset in ('train', 'test') for v in kpx_amd.data.KeypointDataLoader(data_dir, subset, image_size=size).video_ids()])
        for subset in ('train', 'test'):
            loader = kpx_amd.data.KeypointDataLoader(data_dir, subset, image_size=size)
            for pos, v in enumerate(loader.videos(dev)):
                outputs = model.run(None, {'image': v['image'][None], 'idx': np.array([v['idx']]), 'len': np.array([v['len']])})
                _save_output(keypoints_root_dir, outputs)
                if stab:
                    stab.video(subset, v['image'], outputs['pts'][0], int(v['idx']), int(v['len']))
                if joints:
                    joints.video(subset, v['image'], outputs['pts'][0], int(v['idx']), int(v['len']), loader.frame_size(pos))
                frames += v['len']
            print('iteration through %s set finished' % subset)
        torch.cuda.synchronize()
        print('%d frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))
        if stab:
            stab.finish()
        if joints:
            joints.finish(False)
        return
    for v in range(args.synthetic):
        rs = np.random.RandomState(v)
        n = int(rs.randint(args.frames // 4, args.frames + 1))
        im = np.zeros((1, args.frames, size, size, 3), np.float32)
        im[0, :n] = (rs.randint(0, 256, size=(n, size, size, 3)).astype(np.float32) / 255.0 * 2.0 - 1.0)
        outputs = model.run(None, {'image': torch.from_numpy(im).to(dev), 'idx': np.array([v]), 'len': np.array([n])})
        _save_output(keypoints_root_dir, outputs)
        if stab:
            stab.video('synthetic', outputs['im'][0], outputs['pts'][0], v, n)
        if joints:
            planted = joints.lib.planted_labels([SYNTHETIC_JOINTS_SEED, v], n, SYNTHETIC_JOINTS, (size, size))
            joints.video('test' if v % 2 else 'train', outputs['im'][0], outputs['pts'][0], v, n, (size, size), labels=planted)
        frames += args.frames
    torch.cuda.synchronize()
    print('iteration through synthetic set finished: %d frames, %.1f frames/sec' % (frames, frames / (time.time() - t0)))
    if stab:
        stab.finish()
    if joints:
        joints.finish(True)


if __name__ == '__main__':
    main()
