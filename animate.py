"""Animate your own stills: every image rolled out under each action class, or along the motion of your own video, as animated GIFs.

    python animate.py --config C --checkpoint_stage1 S1 [--checkpoint_stage2 S2] --images PATH [PATH ...]
                      [--box x0,y0,x1,y1] [--actions all|i,j,k] [--samples S] [--seed N] [--overlay R] [--sheet-frames i,j,k]
                      [--driver DIR [--driver-mode relative|absolute] [--driver-scaled] [--driver-box x0,y0,x1,y1]]
                      [--frames N] [--rate F] [--resample linear|cubic]
                      [--gif-fps N] [--gif-dither A] [--video [--video-fps N] [--video-quality Q]] [--png] [--batch B] [--colors_seed S] [--save_dir D]

Inputs (``kpx_amd.stills``): each PATH is an image file, a directory (its .jpg .jpeg .png .bmp files in sorted name order) or a .txt manifest
(one ``path [x0,y0,x1,y1]`` per line, relative to the manifest).  Decoding is PIL's on the host: EXIF orientation applied, then
``convert('RGB')`` -- an alpha channel is dropped, not composited.  ``--box`` crops in pixels of the upright image (a manifest's box wins);
the fit to S x S (``model.image_size`` / ``--image-size``, default 128) is the sequence loader's start-frame arithmetic, so a still reaches the networks as a Penn frame of the same pixels.

Rollouts (``--checkpoint_stage2``): every still under each class of ``--actions`` (default all) for each of ``--samples`` draws; draw s
uses row s of ``numpy.random.RandomState(seed).randn(S, vae_dim).astype(float32)``, shared by all stills and all classes.
Driver (``--driver DIR``, stage 2 not needed): DIR holds N >= 33 frames of a video; frames i * (N // 33) are fitted like stills, the stage-1
detector finds their key points, and every still is rolled out on them (``FinalModel.run(drive=...)``, default mode ``relative``).

Longer and smoother (``FinalModel.run(frames=, rate=, resample=)``): ``--frames N`` (a multiple of 32) chains N / 32
calls of the motion generator, each started from the last pose of the one before; segment i >= 1 of draw s uses row s of the i-th further
``randn(S, vae_dim)`` of the same RandomState.  ``--rate F`` puts F - 1 frames between every two (``--resample``, default cubic) and plays
the GIFs at F times ``--gif-fps``, so they last as long as before and only move more smoothly; set ``--gif-fps`` for slow motion.  The GIFs then
hold 1 + N F frames and ``--sheet-frames`` indexes those.  With ``--driver`` only ``--rate`` applies: the driver's cell repeats each of its
frames F times.

Files, under <save_dir>/%04d/ per still in input order: input_im.png and current_points.png as evaluate.py writes them; classes.gif, the
animated grid (row = draw, column = class, 33 frames, frame 0 = the still) with ONE palette over all cells and frames; with ``--overlay R``
classes_overlay.gif, the same grid with the key points marked on the frames (a disc of radius R - 1 with a one-pixel outline,
``kpx_amd.ops.cell_frames``), and overlay.png, its first cell at frame 0; classes.png and classes_points.png, the contact sheets of
evaluate.py --actions for draw 0; with ``--driver`` driven.gif (driver | pred) and driven_overlay.gif; with ``--png`` the frames of every
rollout as evaluate.py writes them; with ``--video`` every GIF also as a true-colour Motion-JPEG AVI beside it (classes.avi, classes_overlay.avi,
driven.avi, driven_overlay.avi: the same canvases JPEG-coded on the device, ``kpx_amd.ops.jpeg_encode``; ``--video-fps`` 1..240, default 10,
times ``--rate``; ``--video-quality`` 1..100, default 90).  <save_dir>/animate.json records the inputs and the settings.  No quality claim is made for images
outside the training distribution: the overlay is there to judge that.
"""
import json
import os
import os.path as osp
import sys
from argparse import ArgumentParser

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_FRAMES = 33                          # the still, then the 32 predicted frames
PNG_FOLDERS = (('pred_seq', 'pred_im_seq', True), ('mask', 'mask', False), ('crude', 'pred_im_crude', True), ('pred_points', 'future_points', False))


class _Tap:
    """a FinalModel whose run() hands every output to ``consume`` before the caller (evaluate._ClassSweep) sees it: the outputs live in graph
    buffers that the next run() overwrites"""

    def __init__(self, model, consume, rollout=None):
        self.model, self.consume, self.rollout = model, consume, dict(rollout or {})       # rollout: frames / rate / resample of every run()

    def __getattr__(self, name):
        return getattr(self.model, name)

    def run(self, sess, feed_dict, z=None, drive=None):
        out = self.model.run(sess, feed_dict, z=z, drive=drive, **self.rollout)
        self.consume(out)
        return out


def _write_rollout_pngs(evaluate, folder, out, batch_idx):
    for name, key, rescale in PNG_FOLDERS:
        evaluate._save_img_sequence(osp.join(folder, name), out[key][batch_idx], rescale=rescale)


def main(argv=None):
    parser = ArgumentParser(description='animate stills by action class or by a driving video')
    parser.add_argument('--config', type=str, required=True, help='path of the configuration file')
    parser.add_argument('--checkpoint_stage1', type=str, required=True, help='path of the stage1 checkpoint')
    parser.add_argument('--checkpoint_stage2', type=str, default=None, help='path of the stage2 checkpoint (class rollouts need it)')
    parser.add_argument('--images', type=str, nargs='+', required=True, help='image files, directories or .txt manifests')
    parser.add_argument('--box', type=str, default=None, help='x0,y0,x1,y1: crop every still, in pixels of the upright image')
    parser.add_argument('--actions', type=str, default=None, help="'all' (default) or i,j,k: the classes, one column each")
    parser.add_argument('--samples', type=int, default=None, help='draws of z, one row each (default 1)')
    parser.add_argument('--seed', type=int, default=None, help='seed of the draws (default 0)')
    parser.add_argument('--overlay', type=int, default=0, help='radius 1..16 of the key-point markers of the *_overlay files (default 0: none)')
    parser.add_argument('--sheet-frames', type=str, default=None, help='the predicted frames of classes.png (default 3,7,...,31)')
    parser.add_argument('--driver', type=str, default=None, help='a directory of >= 33 frames of a video whose motion drives every still')
    parser.add_argument('--driver-mode', type=str, default=None, help='relative (default) or absolute')
    parser.add_argument('--driver-scaled', action='store_true', help="with --driver-mode relative: scale the motion by the constellations' spreads")
    parser.add_argument('--driver-box', type=str, default=None, help='x0,y0,x1,y1: crop every driver frame')
    parser.add_argument('--frames', type=int, default=None, help='predicted frames before resampling, a multiple of 32 (default 32): N / 32 chained motion-generator calls')
    parser.add_argument('--rate', type=int, default=None, help='1..64 (default 1): F - 1 frames between every two predicted ones; the GIFs play at F x --gif-fps')
    parser.add_argument('--resample', type=str, default=None, help='linear or cubic (default): how --rate places the key points in between')
    parser.add_argument('--gif-fps', type=int, default=10, help='frames per second, 1..50 (default 10); with --rate F the GIFs play at F times this')
    parser.add_argument('--gif-dither', type=int, default=0, help='amplitude of the 4x4 ordered dither, 0..64 (default 0: none)')
    parser.add_argument('--video', action='store_true',
                        help='also every GIF as a true-colour Motion-JPEG AVI beside it (classes.avi, ...), JPEG-coded on the device')
    parser.add_argument('--video-fps', type=int, default=None, help='with --video: frames per second, 1..240 (default 10); with --rate F the AVIs play at F times this')
    parser.add_argument('--video-quality', type=int, default=None, help='with --video: the JPEG quality, 1..100 (default 90)')
    parser.add_argument('--png', action='store_true', help='also the frames of every rollout as PNGs')
    parser.add_argument('--batch', type=int, default=8)
    parser.add_argument('--colors_seed', type=int, default=0, help='seed of the key-point palette')
    parser.add_argument('--image-size', type=int, default=None, metavar='S',
                        help='side S of the stills the networks see and of every cell written, a multiple of 16 in [32, 256]; overrides '
                             'model.image_size of the configuration (default 128)')
    parser.add_argument('--ema', action='store_true',
                        help="read every checkpoint given under its averaged weights (train.py --ema: the <name>/ExponentialMovingAverage entries take their variables' places); a checkpoint without them is refused")
    parser.add_argument('--save_dir', type=str, default='results/animate')
    args = parser.parse_args(argv)

    import evaluate
    from train import config_image_size, load_config
    from kpx_amd import stills
    from kpx_amd.gif import DITHER_RANGE, FPS_RANGE, delay_of_fps
    from kpx_amd.mjpeg import FPS_RANGE as VIDEO_FPS_RANGE, QUALITY_RANGE

    # ---- everything that can be refused is refused here, before the device is touched
    if args.checkpoint_stage2 is None and args.driver is None:
        parser.error('at least one of --checkpoint_stage2 (class rollouts) and --driver (driven rollouts) must be given')
    if args.driver is None:
        for flag, given in (('--driver-mode', args.driver_mode is not None), ('--driver-scaled', args.driver_scaled),
                            ('--driver-box', args.driver_box is not None)):
            if given:
                parser.error('%s shapes the rollout of --driver and needs it' % flag)
    driver_mode = args.driver_mode or 'relative'
    if driver_mode not in ('relative', 'absolute'):
        parser.error('--driver-mode takes relative or absolute (got %r)' % args.driver_mode)
    if args.driver_scaled and driver_mode != 'relative':
        parser.error('--driver-scaled goes with --driver-mode relative alone')
    if not FPS_RANGE[0] <= args.gif_fps <= FPS_RANGE[1]:
        parser.error('--gif-fps takes %d..%d frames per second (got %d)' % (FPS_RANGE + (args.gif_fps,)))
    n_pred, rate, resample = 32 if args.frames is None else args.frames, 1 if args.rate is None else args.rate, args.resample or 'cubic'
    if n_pred < 32 or n_pred % 32:
        parser.error('--frames takes a positive multiple of 32 (got %d)' % n_pred)
    if not 1 <= rate <= 64:
        parser.error('--rate takes 1..64 (got %d)' % rate)
    if resample not in ('linear', 'cubic'):
        parser.error('--resample takes linear or cubic (got %r)' % args.resample)
    if args.resample is not None and rate == 1:
        parser.error('--resample chooses how --rate places the frames in between and needs --rate >= 2')
    if args.driver is not None and args.frames is not None:
        parser.error('--frames chains the motion generator; with --driver the motion is the 33 frames of the driver (only --rate applies)')
    if args.gif_fps * rate > FPS_RANGE[1]:
        parser.error('--gif-fps %d x --rate %d = %d frames per second, and a GIF plays at most %d: lower --gif-fps'
                     % (args.gif_fps, rate, args.gif_fps * rate, FPS_RANGE[1]))
    if (args.video_fps is not None or args.video_quality is not None) and not args.video:
        parser.error('--video-fps and --video-quality shape the files of --video and need it')
    video_fps, video_quality = 10 if args.video_fps is None else args.video_fps, 90 if args.video_quality is None else args.video_quality
    if not VIDEO_FPS_RANGE[0] <= video_fps <= VIDEO_FPS_RANGE[1]:
        parser.error('--video-fps takes %d..%d frames per second (got %d)' % (VIDEO_FPS_RANGE + (video_fps,)))
    if not QUALITY_RANGE[0] <= video_quality <= QUALITY_RANGE[1]:
        parser.error('--video-quality takes %d..%d (got %d)' % (QUALITY_RANGE + (video_quality,)))
    if args.video and video_fps * rate > VIDEO_FPS_RANGE[1]:
        parser.error('--video-fps %d x --rate %d = %d frames per second, and the AVIs play at most %d: lower --video-fps'
                     % (video_fps, rate, video_fps * rate, VIDEO_FPS_RANGE[1]))
    n_frames = 1 + n_pred * rate                           # the still, then T' = frames x rate predicted frames
    if not DITHER_RANGE[0] <= args.gif_dither <= DITHER_RANGE[1]:
        parser.error('--gif-dither takes an amplitude in %d..%d (got %d)' % (DITHER_RANGE + (args.gif_dither,)))
    if not 0 <= args.overlay <= stills.MAX_RADIUS:
        parser.error('--overlay takes a marker radius in 1..%d, or 0 for none (got %d)' % (stills.MAX_RADIUS, args.overlay))
    if args.batch < 1:
        parser.error('--batch must be >= 1 (got %d)' % args.batch)
    samples = 1 if args.samples is None else args.samples
    seed = 0 if args.seed is None else args.seed
    if not 0 <= seed < 2 ** 32:
        parser.error('--seed takes a numpy RandomState seed in [0, 2^32) (got %d)' % seed)
    config = load_config(args.config)
    n_action, size = config['model'].get('n_action', 9), config_image_size(config, args.image_size)      # the model's size, and the stills'
    actions = sheet_frames = None
    try:
        if args.checkpoint_stage2 is not None:
            text = 'all' if args.actions is None else args.actions.strip()
            actions = list(range(n_action)) if text == 'all' else evaluate._parse_index_list(text, '--actions', n_action)
            stills.check_grid(samples, len(actions), size, size, frames=n_frames)
            sheet_frames = list(evaluate.SHEET_FRAMES_DEFAULT)
            if args.sheet_frames is not None:
                sheet_frames = evaluate._parse_index_list(args.sheet_frames, '--sheet-frames', n_frames - 1)
                if sheet_frames != sorted(sheet_frames) or len(sheet_frames) > 63:
                    raise ValueError('--sheet-frames takes at most 63 increasing frame indices (got %r)' % args.sheet_frames)
        box = stills.parse_box(args.box, '--box') if args.box is not None else None
        listed = stills.list_images(args.images, box)
        fitted, records = [], []
        for path, own in listed:                         # decoded on the host, once: the decode is what a still costs
            u8, info = stills.fit(path, own, what='--box' if own is box else 'the manifest box', image_size=size)
            fitted.append(u8)
            records.append(info)
        driver = None
        if args.driver is not None:
            driver_box = stills.parse_box(args.driver_box, '--driver-box') if args.driver_box is not None else None
            paths, idx, n_found = stills.driver_frames(args.driver)
            driver = {'paths': paths, 'frames': idx, 'n_found': n_found,
                      'u8': np.stack([stills.fit(p, driver_box, what='--driver-box', image_size=size)[0] for p in paths])}
    except ValueError as e:                              # (StillsError is one)
        parser.error(str(e))
    checkpoints = [args.checkpoint_stage1] + ([args.checkpoint_stage2] if args.checkpoint_stage2 is not None else [])
    for p in checkpoints:
        if not (osp.exists(p) or osp.exists(p + '.index')):
            raise Exception('checkpoint not found at %s' % p)

    # ---- the device
    import torch
    import kpx_amd
    from kpx_amd.data import _to_device_unit
    ops = kpx_amd.ops
    dev = torch.device('cuda', 0)
    model = kpx_amd.FinalModel(config, device=dev, image_size=size, point_maps=True, colors_seed=args.colors_seed)
    model.build(None)
    for p in checkpoints:
        model.restore(None, p, **({'ema': True} if args.ema else {}))
    k, radius = model.n_points, args.overlay
    if radius and k > ops.CELL_MAX_POINTS:
        raise Exception('--overlay marks at most %d key points (the model has %d)' % (ops.CELL_MAX_POINTS, k))
    colors = torch.from_numpy(stills.marker_colors(model.colors)).to(dev) if radius else None
    gifs = kpx_amd.gif.RolloutGifs(args.gif_fps * rate, args.gif_dither)
    if args.video and actions and max(samples, len(actions)) * size > ops.JPEG_MAX_SIDE:
        raise Exception('--video: the grid of %d draws x %d classes of %d x %d cells is larger than the %d pixels a side a JPEG frame of '
                        'classes.avi holds' % (samples, len(actions), size, size, ops.JPEG_MAX_SIDE))
    video_bytes = {}

    def write_videos(name, canvas):                        # beside <name>.gif, from the same canvas
        if args.video:
            video_bytes.setdefault(name, []).extend(
                stills.write_grid_videos(canvas, [osp.join(d, name + '.avi') for d in dirs], video_fps * rate, video_quality))

    rollout = {} if (n_pred, rate) == (32, 1) else {'frames': n_pred, 'rate': rate, 'resample': resample}
    n_cls = len(actions) if actions else 0
    layers = 2 if radius else 1
    per_still = n_frames * size * size * 3 * layers * ((samples * n_cls if actions else 0) + (2 if driver else 0))
    batch = stills.batch_under(args.batch, per_still)
    zs = None
    if actions:
        rs = np.random.RandomState(seed)                   # segment 0 first: a longer rollout begins as the 32-frame one of the same seed
        zs = torch.from_numpy(np.stack([rs.randn(samples, model.vae_dim).astype(np.float32) for _ in range(n_pred // 32)], 1)).to(dev)   # [S, segments, V]
    drv = None
    if driver is not None:
        frames = _to_device_unit(driver['u8'], dev)                                        # [33,R,R,3]
        pts = model.detect(frames)                                                         # [33,K,2]
        drv = {'image': frames[:1], 'seq': frames[1:].unsqueeze(0), 'first_pt': pts[:1].contiguous(), 'seq_pt': pts[1:].unsqueeze(0).contiguous()}
    palette_sizes = {name: [] for name in (['classes'] if actions else []) + (['classes_overlay'] if actions and radius else [])
                     + (['driven'] if driver else []) + (['driven_overlay'] if driver and radius else [])}
    from PIL import Image

    for start in range(0, len(fitted), batch):
        bsz = min(batch, len(fitted) - start)
        image = _to_device_unit(np.stack(fitted[start:start + bsz]), dev)
        dirs = [osp.join(args.save_dir, '%04d' % (start + i)) for i in range(bsz)]
        for d in dirs:
            os.makedirs(d, exist_ok=True)
        state = {'inputs': False}

        def write_inputs(out):
            if not state['inputs']:
                state['inputs'] = True
                im, cur = out['im'].cpu().numpy(), out['current_points'].cpu().numpy()
                for i, d in enumerate(dirs):
                    evaluate._save_img(osp.join(d, 'input_im.png'), im[i], rescale=True)
                    evaluate._save_img(osp.join(d, 'current_points.png'), cur[i], rescale=False)

        def marks(out):
            return out['first_pt'].reshape(bsz, k, 2).contiguous(), out['fut_pt_raw'].reshape(bsz, n_frames - 1, k, 2).contiguous()

        if actions:
            grid = torch.empty((bsz, n_frames, samples * size, n_cls * size, 3), dtype=torch.uint8, device=dev)
            over = torch.empty_like(grid) if radius else None

            def consume(out):                            # one rollout: its cell of the grids, before the next run() replays the graph
                s, a = state['draw'], state['a']
                pred = out['pred_im_seq'].contiguous()
                ops.cell_frames(grid, image, pred, s, a, 'unit')
                if over is not None:
                    ops.cell_frames(over, image, pred, s, a, 'unit', *marks(out), colors=colors, radius=radius)
                write_inputs(out)
                if args.png:
                    host = {key: out[key].cpu().numpy() for _, key, _ in PNG_FOLDERS}
                    for i, d in enumerate(dirs):
                        _write_rollout_pngs(evaluate, osp.join(d, 'draw_%02d' % s, 'class_%02d' % actions[a]), host, i)
                state['a'] = a + 1

            sweep = evaluate._ClassSweep(kpx_amd, _Tap(model, consume, rollout), actions, n_action, sheet_frames, image, None, True, samples, None, dev)
            for s in range(samples):
                state.update(draw=s, a=0)
                z = zs[s].unsqueeze(1).expand(-1, bsz, -1).contiguous()           # [segments, B, V]
                sweep.run(s, z[0] if n_pred == 32 else z)
            sweep.write_sheets(args.save_dir, start)
            palette_sizes['classes'] += stills.write_grid_gifs(gifs, grid, [osp.join(d, 'classes.gif') for d in dirs])
            write_videos('classes', grid)
            if over is not None:
                palette_sizes['classes_overlay'] += stills.write_grid_gifs(gifs, over, [osp.join(d, 'classes_overlay.gif') for d in dirs])
                write_videos('classes_overlay', over)
                first = over[:, 0, :size, :size].contiguous().cpu().numpy()
                for i, d in enumerate(dirs):
                    Image.fromarray(first[i]).save(osp.join(d, 'overlay.png'))
        if drv is not None:
            tile = lambda t: t.expand((bsz,) + tuple(t.shape[1:])).contiguous()
            out = model.run(None, {'image': image}, drive={'mode': driver_mode, 'first': tile(drv['first_pt']), 'seq': tile(drv['seq_pt']),
                                                           'shift': 0, 'scaled': bool(args.driver_scaled)}, **rollout)
            pred = out['pred_im_seq'].contiguous()
            d_first, d_seq, d_pts = tile(drv['image']), tile(drv['seq']), tile(drv['seq_pt'])
            if rate > 1:                                 # the driver has the frames it has: each one stands for `rate` frames of the rollout
                d_seq, d_pts = d_seq.repeat_interleave(rate, dim=1), d_pts.repeat_interleave(rate, dim=1)
            pair = torch.empty((bsz, n_frames, size, 2 * size, 3), dtype=torch.uint8, device=dev)
            ops.cell_frames(pair, d_first, d_seq, 0, 0, 'unit')
            ops.cell_frames(pair, image, pred, 0, 1, 'unit')
            palette_sizes['driven'] += stills.write_grid_gifs(gifs, pair, [osp.join(d, 'driven.gif') for d in dirs])
            write_videos('driven', pair)
            if radius:                                   # the driver's own key points on its cell, the retargeted ones on the rollout
                ops.cell_frames(pair, d_first, d_seq, 0, 0, 'unit', tile(drv['first_pt']), d_pts, colors=colors, radius=radius)
                ops.cell_frames(pair, image, pred, 0, 1, 'unit', *marks(out), colors=colors, radius=radius)
                palette_sizes['driven_overlay'] += stills.write_grid_gifs(gifs, pair, [osp.join(d, 'driven_overlay.gif') for d in dirs])
                write_videos('driven_overlay', pair)
            write_inputs(out)
            if args.png:
                host = {key: out[key].cpu().numpy() for _, key, _ in PNG_FOLDERS}
                for i, d in enumerate(dirs):
                    _write_rollout_pngs(evaluate, osp.join(d, 'driven'), host, i)
    torch.cuda.synchronize()
    meta = {'stills': records, 'cell': [size, size], 'frames': n_frames, 'fps': gifs.fps, 'delay_cs': delay_of_fps(gifs.fps), 'dither': gifs.dither,
            'overlay': radius, 'batch': batch, 'palette_sizes': palette_sizes}
    if rollout:
        meta['rollout'] = dict(rollout, gif_fps=args.gif_fps)
    if args.video:
        meta['video'] = {'fps': video_fps * rate, 'quality': video_quality, 'bytes': video_bytes}
    if actions:
        meta.update({'actions': actions, 'draws': samples, 'seed': seed, 'grid': [samples, n_cls], 'sheet_frames': sheet_frames})
    if driver is not None:
        meta['driver'] = {'dir': args.driver, 'n_found': driver['n_found'], 'frames': driver['frames'], 'files': driver['paths'],
                          'mode': driver_mode, 'scaled': bool(args.driver_scaled),
                          'box': None if args.driver_box is None else list(stills.parse_box(args.driver_box, '--driver-box'))}
    os.makedirs(args.save_dir, exist_ok=True)
    with open(osp.join(args.save_dir, 'animate.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('animated %d stills: %s' % (len(fitted), ', '.join('%s.gif' % name for name in palette_sizes)))


if __name__ == '__main__':
    main()
