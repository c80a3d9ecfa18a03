"""Animate your own stills: every image rolled out under each action class, or along the motion of your own video, as animated GIFs.

    python animate.py --config C --checkpoint_stage1 S1 [--checkpoint_stage2 S2] --images PATH [PATH ...]
                      [--box x0,y0,x1,y1] [--actions all|i,j,k] [--samples S] [--seed N] [--overlay R] [--sheet-frames i,j,k]
                      [--driver DIR [--driver-mode relative|absolute] [--driver-scaled] [--driver-box x0,y0,x1,y1]]
                      [--frames N] [--rate F] [--resample linear|cubic]
                      [--interpolate S [--interp-mode lerp|slerp]] [--motion-from DIR --motion-class C]
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

Latent space (stage 2; 32-frame rollouts only, so not with ``--frames`` / ``--rate``): ``--interpolate S`` (2..64, ``--samples`` >= 2) joins the
seeded draws 0 and 1 by ``kpx_amd.ops.latent_path`` (``--interp-mode``, default slerp: the great circle; lerp: the straight line) and rolls every
still out at each of the S steps under each class: interp.gif, one row per step and one column per class, and interp.png, the same grid at
the last predicted frame -- its first and last rows are the cells of draws 0 and 1.  ``--motion-from DIR --motion-class C`` (not with
``--driver``; the checkpoint must hold the stage-2 encoder) reads and detects 33 frames of DIR exactly as ``--driver`` does, encodes their
key points as a motion of class C (``FinalModel.encode``) and rolls every still out at z = mu under each class of ``--actions``: latent.gif
and latent.png, one column per class.  This replays the motion through the generator's latent space, from the still's own pose; ``--driver``
copies key points.

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
    parser.add_argument('--interpolate', type=int, default=None, metavar='S',
                        help='2..64: also roll every still out at S steps of z between the seeded draws 0 and 1 (needs --samples >= 2): interp.gif, interp.png')
    parser.add_argument('--interp-mode', type=str, default=None, help='with --interpolate: slerp (default) or lerp')
    parser.add_argument('--motion-from', type=str, default=None, metavar='DIR',
                        help='a directory of >= 33 frames of a video whose motion is encoded by the stage-2 encoder and replayed from every still at z = mu: latent.gif, latent.png')
    parser.add_argument('--motion-class', type=int, default=None, metavar='C', help='with --motion-from: the action class of that motion')
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
    if args.interp_mode is not None and args.interpolate is None:
        parser.error('--interp-mode chooses the path of --interpolate and needs it')
    interp_mode = args.interp_mode or 'slerp'
    if interp_mode not in ('lerp', 'slerp'):
        parser.error('--interp-mode takes lerp or slerp (got %r)' % args.interp_mode)
    if args.interpolate is not None:
        if not 2 <= args.interpolate <= 64:
            parser.error('--interpolate takes 2..64 steps (got %d)' % args.interpolate)
        if args.checkpoint_stage2 is None:
            parser.error('--interpolate walks the latent space of the motion generator and needs --checkpoint_stage2')
        if (1 if args.samples is None else args.samples) < 2:
            parser.error('--interpolate joins the seeded draws 0 and 1 and needs --samples >= 2')
    if (args.motion_from is None) != (args.motion_class is None):
        parser.error('--motion-from and --motion-class go together: the encoder reads a motion and its class')
    if args.motion_from is not None:
        if args.driver is not None:
            parser.error('--motion-from replays a motion through the latent space and --driver copies its key points: give one of them')
        if args.checkpoint_stage2 is None:
            parser.error('--motion-from encodes the motion with the stage-2 encoder and needs --checkpoint_stage2')
    if (args.interpolate is not None or args.motion_from is not None) and (n_pred, rate) != (32, 1):
        parser.error('--interpolate and --motion-from roll one 32-frame segment out at a given z: not with --frames or --rate')
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
        if args.motion_class is not None and not 0 <= args.motion_class < n_action:
            raise ValueError('--motion-class takes a class in [0, %d) (got %d)' % (n_action, args.motion_class))
        if args.interpolate is not None:
            stills.check_grid(args.interpolate, len(actions), size, size, frames=n_frames)
        motion = None
        if args.motion_from is not None:                 # read as --driver reads its frames
            paths, idx, n_found = stills.driver_frames(args.motion_from, '--motion-from')
            motion = {'paths': paths, 'frames': idx, 'n_found': n_found,
                      'u8': np.stack([stills.fit(p, None, what='--motion-from', image_size=size)[0] for p in paths])}
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
    model = kpx_amd.FinalModel(config, device=dev, image_size=size, point_maps=True, colors_seed=args.colors_seed,
                               **({'posterior': True} if motion is not None else {}))
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
    if args.video and args.interpolate is not None and max(args.interpolate, len(actions)) * size > ops.JPEG_MAX_SIDE:
        raise Exception('--video: the grid of %d steps x %d classes of %d x %d cells is larger than the %d pixels a side a JPEG frame of '
                        'interp.avi holds' % (args.interpolate, len(actions), size, size, ops.JPEG_MAX_SIDE))
    video_bytes = {}

    def write_videos(name, canvas):                        # beside <name>.gif, from the same canvas
        if args.video:
            video_bytes.setdefault(name, []).extend(
                stills.write_grid_videos(canvas, [osp.join(d, name + '.avi') for d in dirs], video_fps * rate, video_quality))

    rollout = {} if (n_pred, rate) == (32, 1) else {'frames': n_pred, 'rate': rate, 'resample': resample}
    n_cls = len(actions) if actions else 0
    layers = 2 if radius else 1
    per_still = n_frames * size * size * 3 * layers * ((samples * n_cls if actions else 0) + (2 if driver else 0))
    per_still += n_frames * size * size * 3 * n_cls * ((args.interpolate or 0) + (1 if motion else 0))
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
    z_path = z_motion = None
    if args.interpolate is not None:                   # [S, 1, V]: the steps between the seeded draws 0 and 1 of segment 0
        z_path = ops.latent_path(zs[0, :1].contiguous(), zs[1, :1].contiguous(), args.interpolate, interp_mode)
    if motion is not None:
        frames = _to_device_unit(motion['u8'], dev)                                        # [33,R,R,3]
        pts = model.detect(frames)                                                         # [33,K,2]
        code = torch.eye(n_action, dtype=torch.float32, device=dev)[args.motion_class:args.motion_class + 1].contiguous()
        logit = model.encode(pts[:1].contiguous(), pts[1:].unsqueeze(0).contiguous(), code)
        z_motion = ops.latent_sample(logit, None, 0.0)                                     # [1, V]: mu
    palette_sizes = {name: [] for name in (['classes'] if actions else []) + (['classes_overlay'] if actions and radius else [])
                     + (['driven'] if driver else []) + (['driven_overlay'] if driver and radius else [])
                     + (['interp'] if z_path is not None else []) + (['latent'] if z_motion is not None else [])}
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
        for name, z_rows in (('interp', z_path), ('latent', z_motion)):
            if z_rows is None:
                continue
            z_rows = z_rows.reshape(-1, model.vae_dim)                                     # one row of cells per z
            codes = torch.eye(n_action, dtype=torch.float32, device=dev)[actions]
            canvas = torch.empty((bsz, n_frames, z_rows.shape[0] * size, n_cls * size, 3), dtype=torch.uint8, device=dev)
            for r in range(z_rows.shape[0]):
                z = z_rows[r:r + 1].expand(bsz, -1).contiguous()
                for a in range(n_cls):
                    out = model.run(None, {'image': image, 'action_code': codes[a:a + 1].expand(bsz, -1).contiguous()}, z=z)
                    ops.cell_frames(canvas, image, out['pred_im_seq'].contiguous(), r, a, 'unit')     # before the next run() replays the graph
                    write_inputs(out)
            palette_sizes[name] += stills.write_grid_gifs(gifs, canvas, [osp.join(d, name + '.gif') for d in dirs])
            write_videos(name, canvas)
            last = canvas[:, n_frames - 1].contiguous().cpu().numpy()                      # the grid at the last predicted frame
            for i, d in enumerate(dirs):
                Image.fromarray(last[i]).save(osp.join(d, name + '.png'))
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
    if z_path is not None:
        meta['interpolate'] = {'steps': args.interpolate, 'mode': interp_mode, 'draws': [0, 1], 'grid': [args.interpolate, n_cls]}
    if motion is not None:
        meta['motion_from'] = {'dir': args.motion_from, 'n_found': motion['n_found'], 'frames': motion['frames'], 'files': motion['paths'],
                               'class': args.motion_class, 'z': 'mu', 'grid': [1, n_cls]}
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
