#!/usr/bin/env python3
"""Training entry point with the reference's CLI (reference: train.py:12-114):

    python train.py --mode detector_translator --config configs/penn.yaml [--synthetic] [--steps N]
    python train.py --mode detector_translator --config configs/penn256.yaml --resident-data      (256 x 256; or --image-size S on any config)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py --mode ... (data parallel)

    python train.py --mode action_classifier --config configs/penn.yaml [--synthetic] [--resident-labels] [--steps N]

Three modes are built: ``detector_translator`` (stage 1, the BASELINE.json hot path), ``motion_generator`` (stage 2, the
sequence VAE-GAN over the pseudo labels written by make_pseudo_labels.py) and ``action_classifier`` (this project's own recogniser
over the same key-point sequences and classes, the network evaluate.py --action-accuracy scores rollouts with; it has no
counterpart in the reference).  Without ``--synthetic`` the frames come from ``paths.data_dir`` through kpx_amd.data.ImagePairDataLoader (the
reference's data/image_pair_dataloader.py + tf.data pipeline: threaded PIL augmentation, uint8 batches in pinned memory, async
copy + on-device conversion); ``--synthetic`` feeds Penn-shaped random pairs with the same output contract (float32 NHWC in
[-1,1], keys image / future_image).  ``--resident-data`` (detector_translator) decodes every frame of both subsets once into HBM and augments on the
GPU (kpx_amd.resident): the same batches bit for bit, without the per-step JPEG decoding.  ``--resident-labels`` (motion_generator) keeps
every video's pseudo labels in HBM and builds each key-point batch with one HIP launch: the same batches bit for bit, with no file read,
PIL call or numpy work per step; the start frames, which only the image summary shows, are rendered for its two samples alone.
``action_classifier`` reads the batches ``motion_generator`` reads (``--resident-labels`` included) and uses their ``real_seq`` and
``action_code``; its ``--synthetic`` feeds a planted problem in which the class decides the direction the points drift in
(kpx_amd.synthetic.planted_action_batch).

Long runs, all three modes: ``--resume latest|PATH`` continues from a checkpoint (variables, Adam slots, beta powers, global_step; stage 2 also
its noise generator's state from the side file model.ckpt-N.rng-RANK.npz; ``latest`` = the newest complete checkpoint of the log directory,
or a start from scratch when there is none), ``--keep N`` prunes older checkpoints after each save, and ``--guard`` skips the update of a
bucket whose gradient holds a NaN or an Inf, decided on the device inside the step (``--guard-max-skips N`` stops a run that only skips).
``--ema DECAY`` keeps an exponential moving average of the generator's weights (the 'G' bucket) inside the step, one HIP launch behind the
generator's Adam update; checkpoints carry the averages as ``<name>/ExponentialMovingAverage``, ``--resume`` continues them, ``--ema-test``
runs each test pass a second time under them (``<log_dir>/<mode>/test_ema``), and evaluate.py / animate.py / make_pseudo_labels.py ``--ema``
read a checkpoint under them (``python -m kpx_amd.ema IN OUT`` writes them out as a plain inference checkpoint).
``--clip-norm C`` is tf.clip_by_global_norm per optimiser: a bucket whose exchanged gradient has a norm above C is scaled down to norm C inside
the Adam launch, from the fp64 sum of squares the guard's health pass already leaves on the device (so it turns ``--guard`` on).
``--grad-stats [N]`` prints, at each log point, the N variables of largest gradient norm per bucket (one segmented reduction in HIP, run
between steps) and names every variable that holds a non-finite gradient value when the guard counted one; at summary steps the scalars
``clip/*``, ``grad_norm/<variable>`` and ``update_ratio/<variable>`` are written.  Neither is written into checkpoints: the clip counters
restart on ``--resume``.
Checkpoints are written under temporary names and renamed into place.  Real data loaders are reseeded on a resume, not continued sample
for sample.
"""
import logging
import os
import sys
from argparse import ArgumentParser

import torch
import yaml

log = logging.getLogger('kpx')

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_config(config_path):
    """reference utils/__init__.py:8-10"""
    with open(config_path, 'r') as f:
        return yaml.load(f, Loader=yaml.FullLoader)


def config_image_size(config, override=None):
    """The side S of the frames the networks see: ``--image-size`` where the command line gives one, else the optional YAML key
    model.image_size, else 128; checked by the package's one rule (kpx_amd.data.check_image_size: a multiple of 16 in [32, 256], a
    ``KpxError`` naming the key and the value otherwise).  train.py, evaluate.py, make_pseudo_labels.py and animate.py all come here."""
    from kpx_amd.data import IMAGE_SIZE, check_image_size
    if override is not None:
        return check_image_size(override, '--image-size')
    return check_image_size((config.get('model') or {}).get('image_size', IMAGE_SIZE))


IMAGE_SIZE_HELP = ('side S of the frames the networks see, a multiple of 16 in [32, 256]; overrides model.image_size of the configuration '
                   '(default 128).  Checkpoints carry no size: one trained at another S loads, with no claim about its quality')


def _get_model_by_mode(mode, config, global_step, **kw):
    """reference train.py:117-123"""
    if mode == 'detector_translator':
        from kpx_amd import DetectorTranslatorModel
        return DetectorTranslatorModel(config, global_step, is_training=True, **kw)
    if mode == 'motion_generator':
        from kpx_amd import MotionGeneratorModel
        kw.pop('vgg', None)
        return MotionGeneratorModel(config, global_step, is_training=True, **kw)
    if mode == 'action_classifier':
        from kpx_amd import ActionClassifierModel
        kw.pop('vgg', None)
        kw.pop('colors_seed', None)
        return ActionClassifierModel(config, global_step, is_training=True, **kw)
    raise Exception('unknown model %s' % mode)


def _guard_kw(args):
    """guard=True only under --guard: without the flag the constructors are called exactly as before."""
    return {'guard': True} if args.guard else {}


def _clip_kw(args):
    """clip_norm=C only under --clip-norm and grad_stats=True only under --grad-stats, as _guard_kw."""
    kw = {'clip_norm': args.clip_norm} if args.clip_norm is not None else {}
    if args.grad_stats is not None:
        kw['grad_stats'] = True
    return kw


def _ema_kw(args):
    """ema=DECAY (and ema_warmup=False) only under --ema (--ema-no-warmup), as _guard_kw."""
    kw = {'ema': args.ema} if args.ema is not None else {}
    if args.ema is not None and args.ema_no_warmup:
        kw['ema_warmup'] = False
    return kw


def _test_under_ema(model, test_pass, step):
    """--ema-test: the test pass once more inside ema_weights(), its summaries and collect_test_results through the third writer."""
    with model.ema_weights():
        writer, model.test_writer = model.test_writer, model.test_ema_writer
        try:
            log.info('test under the averaged weights (step %d):', step)
            return model.collect_test_results(test_pass(), step)
        finally:
            model.test_writer = writer


def _resume_seed(rank, step):
    """One integer per (data-parallel rank, step resumed at): what the streams that are not continued sample for sample are reseeded from."""
    return ((1000 + rank) << 32) | int(step)


def _resume(args, model, log_dir, rank, world, dev):
    """--resume latest|PATH, after build() and before initialize_loggers and the first step: restore the checkpoint strictly (model.resume),
    continue this rank's torch generators from the checkpoint's side file where the model draws on the device, and hold the ranks to one
    global_step.  -> True when a checkpoint was restored (False: --resume latest on a log directory without one)."""
    path = args.resume
    if path == 'latest':
        found = model.latest_checkpoint(log_dir)
        if found is None:
            log.info('--resume latest: no complete checkpoint under %s, starting from scratch', os.path.join(str(log_dir), model.name))
            return False
        path = found[0]
    step, n_vars, n_slots = model.resume(None, path)
    log.info('resumed from %s: global_step %d, %d variables and %d Adam slots restored', path, step, n_vars, n_slots)
    if getattr(model, 'draws_on_device', False):
        saved, beside = step - 1, os.path.dirname(os.path.abspath(path))     # the checkpoint written after step s holds global_step s + 1
        if not model.load_rng_state(saved, rank, beside):
            log.warning('no generator state %s (another world size?): rank %d reseeds its noise from (%d, %d)',
                        model.rng_state_path(saved, rank, beside), rank, 1000 + rank, step)
            torch.manual_seed(_resume_seed(rank, step))
    if world > 1:
        # every rank read the same file; one all-reduce (max of [step, -step]) holds them to it before the first step
        both = torch.tensor([step, -step], dtype=torch.int64, device=dev)
        torch.distributed.all_reduce(both, op=torch.distributed.ReduceOp.MAX)
        hi, lo = int(both[0]), -int(both[1])
        if hi != lo:
            raise Exception('--resume: the ranks restored different steps (global_step %d .. %d; this rank %d): every rank must read the '
                            'same checkpoint' % (lo, hi, step))
    return True


def _reseed_loaders(rank, step):
    """Real data loaders are not continued sample for sample (threads, prefetch, shuffle buffer): a run resumed at ``step`` draws from
    streams reseeded from (1000 + rank, step) -- a deterministic function of where it resumed."""
    import random
    import numpy as np
    random.seed(_resume_seed(rank, step)); np.random.seed([1000 + rank, int(step)])


class _GuardLog(object):
    """--guard at a log point (rank 0): one line when a count moved, the guard/* scalars with the summaries, and the end of a run in which a
    bucket has skipped --guard-max-skips updates in a row."""

    def __init__(self, max_skips):
        self.max_skips, self.seen = max_skips, None

    def __call__(self, model, step, should_write_summary):
        report = model.guard_report()
        counts = {b: (r['skipped_total'], r['skipped_run']) for b, r in report.items()}
        if counts != self.seen and (self.seen is not None or any(c != (0, 0) for c in counts.values())):
            log.info('guard: step %d: %s', step, ', '.join(
                '%s skipped %d of %d updates (%d in a row; %d non-finite gradient values in the last step, grad norm %.4g, max |g| %.4g)'
                % (b, r['skipped_total'], r['updates'], r['skipped_run'], r['nonfinite'], r['grad_norm'], r['max_abs']) for b, r in report.items()))
        self.seen = counts
        if should_write_summary and model.train_writer is not None:
            from kpx_amd import summary
            model.train_writer.add_summary([summary.scalar_value('guard/%s_%s' % (key, b), float(r[field])) for b, r in report.items()
                                            for key, field in (('skipped', 'skipped_total'), ('grad_norm', 'grad_norm'))], step)
        stuck = [b for b, r in report.items() if r['skipped_run'] >= self.max_skips]
        if stuck:
            raise Exception('--guard: bucket %s has skipped %d updates in a row at step %d (--guard-max-skips %d): every gradient is '
                            'non-finite, the run is not training' % (', '.join(stuck), max(report[b]['skipped_run'] for b in stuck), step, self.max_skips))


class _ClipLog(object):
    """--clip-norm / --grad-stats at a log point (rank 0): the clip line, the per-variable line of each bucket, the names of the variables
    that hold a non-finite gradient value when the last step's health record counts one, and the scalars with the summaries."""

    def __init__(self, top):
        self.top = top                      # --grad-stats N, or None without the flag

    def __call__(self, model, step, should_write_summary):
        from kpx_amd import summary
        values = []
        if model.clip_norm is not None:
            report = model.clip_report()
            log.info('clip: step %d: %s', step, ', '.join('%s norm %.4g scale %.4g (%d clipped so far, bound %.4g)'
                                                          % (b, r['norm'], r['scale'], r['clipped_total'], model.clip_norm)
                                                          for b, r in sorted(report.items())))
            for b, r in sorted(report.items()):
                values += [summary.scalar_value('clip/norm_%s' % b, r['norm']), summary.scalar_value('clip/scale_%s' % b, r['scale']),
                           summary.scalar_value('clip/clipped_%s' % b, float(r['clipped_total']))]
        if self.top is not None:
            stats = model.grad_stats()
            lr = float(model.current_lr())
            for b, per_var in sorted(stats.items()):
                first = sorted(per_var.items(), key=lambda kv: -kv[1]['grad_norm'])[:self.top]
                log.info('grad-stats: step %d: %s: %s', step, b, ', '.join('%s %.4g' % (name, r['grad_norm']) for name, r in first))
                bad = [(name, r['nonfinite']) for name, r in per_var.items() if r['nonfinite'] > 0]
                if bad:         # the same buffer the guard's health pass judged: its record counts what these add up to
                    log.info('grad-stats: step %d: %s: non-finite gradient values in %s', step, b, ', '.join('%s (%d)' % nb for nb in bad))
                for name, r in per_var.items():
                    values.append(summary.scalar_value('grad_norm/%s' % name, r['grad_norm']))
                    if r['param_norm'] > 0.0:
                        values.append(summary.scalar_value('update_ratio/%s' % name, lr * r['grad_norm'] / r['param_norm']))
        if should_write_summary and model.train_writer is not None and values:
            model.train_writer.add_summary(values, step)


def _save(args, model, step, rank):
    """The checkpoint of ``step``: rank 0 writes (and prunes under --keep); every rank of a model that draws on the device writes its
    generator states beside it."""
    if getattr(model, 'draws_on_device', False):
        model.save_rng_state(step, rank)
    if rank == 0:
        model.save_checkpoint(None, step, fmt=args.ckpt_format, **({'keep': args.keep} if args.keep is not None else {}))


def _train_motion_generator(args, config, dev, rank, world):
    """reference train.py:136-147 (SequenceDataLoader, is_train -> random_order + randomness) + the common loop (:84-113).  The
    action_classifier mode runs the same loop over the same loaders; it writes no image summary, so it asks for no start frames."""
    import numpy as np
    import kpx_amd
    paths_config, train_config, model_config = config['paths'], config['training'], config['model']
    classifier = args.mode == 'action_classifier'
    model = _get_model_by_mode(args.mode, config, 0, device=dev, colors_seed=args.colors_seed, **_guard_kw(args), **_ema_kw(args), **_clip_kw(args))
    print('model initialized')
    model.build(None)
    batch_size = train_config['batch_size']
    n_steps = args.steps if args.steps is not None else train_config['n_steps']
    k, a = model_config['n_pts'], model_config['n_action']
    train_it = test_batches = None
    resumed = args.resume is not None and _resume(args, model, paths_config['log_dir'], rank, world, dev)
    if not args.synthetic:
        import random
        random.seed(1000 + rank); np.random.seed(1000 + rank)
        if resumed:
            _reseed_loaders(rank, model.global_step)
        size = config_image_size(config, args.image_size)          # stage 2 trains on key points; the size shapes the start frames of its summaries
        mk = lambda subset, train: kpx_amd.SequenceDataLoader(paths_config['data_dir'], subset, n_points=k, n_action=a,
                                                              random_order=train, randomness=train, image_size=size)
        train_it = mk('train', True).batches(batch_size, dev, repeat=True, resident=args.resident_labels)
        if os.path.exists(os.path.join(str(paths_config['data_dir']), 'test_set.txt')):
            test_loader = mk('test', False)
            test_batches = lambda: test_loader.batches(batch_size, dev, repeat=False, resident=args.resident_labels)

    def test_feeds(it):
        """The batches of one test pass; the resident iterator has no 'image', so the batch the summary is written from gets its two."""
        for i, f in enumerate(it):
            if i == 0 and args.resident_labels and not classifier:
                f = dict(f, image=it.start_images(2))
            yield f

    def synthetic(seed):
        if classifier:
            from kpx_amd.synthetic import planted_action_batch
            return {n: torch.from_numpy(v).to(dev) for n, v in planted_action_batch(batch_size, k, a, seed=seed).items()}
        rs = np.random.RandomState(seed)
        d = {'keypoints': rs.rand(batch_size, k, 2) * 1.6 - 0.8, 'real_seq': rs.rand(batch_size, 32, k, 2) * 1.6 - 0.8,
             'action_code': np.eye(a)[rs.randint(0, a, size=batch_size)]}
        return {n: torch.from_numpy(v.astype(np.float32)).to(dev) for n, v in d.items()}
    model.initialize_loggers(paths_config['log_dir'], None)
    guard_log = _GuardLog(args.guard_max_skips) if args.guard else None
    clip_log = _ClipLog(args.grad_stats) if (args.clip_norm is not None or args.grad_stats is not None) else None
    print('training start')
    for step in range(model.global_step, n_steps):
        feed = next(train_it) if train_it is not None else synthetic(step * world + rank)
        should_write_summary = _should_write_summary(train_config, step, rank)
        if args.resident_labels and should_write_summary and not classifier:
            feed = dict(feed, image=train_it.start_images(2))
        model.train_step(None, feed, step, batch_size, should_write_log=step % train_config['log_interval'] == 0 and rank == 0,
                         should_write_summary=should_write_summary)
        if guard_log is not None and step % train_config['log_interval'] == 0 and rank == 0:
            guard_log(model, step, should_write_summary)
        if clip_log is not None and step % train_config['log_interval'] == 0 and rank == 0:
            clip_log(model, step, should_write_summary)
        if step % train_config['checkpoint_interval'] == 0:
            _save(args, model, step, rank)
        if step % train_config['test_interval'] == 0 and rank == 0:
            def test_pass():
                feeds = test_feeds(test_batches()) if test_batches is not None else [synthetic(10 ** 6)]
                return [model.test_step(None, f, step, i, f['keypoints'].shape[0]) for i, f in enumerate(feeds)]
            model.collect_test_results(test_pass(), step)
            if args.ema_test:
                _test_under_ema(model, test_pass, step)
    model.close_loggers()
    if world > 1:
        torch.distributed.destroy_process_group()


def _should_write_summary(train_config, step, rank):
    """reference train.py:88 (step % summary_interval == 0), rank 0 only; a config without summary_interval writes no summaries."""
    interval = train_config.get('summary_interval')
    return bool(interval) and step % int(interval) == 0 and rank == 0


def parse_args(argv=None):
    """The command line, checked: a bad value ends in parser.error (exit status 2) before anything is built."""
    parser = ArgumentParser()
    parser.add_argument('--mode', type=str, choices=['detector_translator', 'motion_generator', 'action_classifier'],
                        help='which mode to train: stage 1, stage 2, or the key-point action recogniser evaluate.py --action-accuracy reads')
    parser.add_argument('--config', type=str, help='path of the configuration file')
    parser.add_argument('--synthetic', action='store_true', help='synthetic Penn-shaped pairs instead of the JPEG pipeline (action_classifier: a planted problem, the class decides '
                             'the direction the points drift in)')
    parser.add_argument('--resident-data', action='store_true',
                        help='detector_translator: decode every frame once, keep the frames in HBM and augment with HIP kernels '
                             '(ImagePairDataLoader.batches(resident=True)); the same batches as without the flag')
    parser.add_argument('--resident-labels', action='store_true',
                        help='motion_generator / action_classifier: keep the pseudo labels of every listed video in HBM and build each key-point batch with '
                             'one HIP launch (SequenceDataLoader.batches(resident=True)); the same batches and summaries as without the flag')
    parser.add_argument('--synthetic-vgg', action='store_true', help='He-normal VGG19 weights when paths.vggnet is absent')
    parser.add_argument('--steps', type=int, default=None, help='override training.n_steps')
    parser.add_argument('--image-size', type=int, default=None, metavar='S', help=IMAGE_SIZE_HELP)
    parser.add_argument('--ckpt-format', choices=['npz', 'tf', 'bundle'], default=os.environ.get('KPX_CKPT_FORMAT', 'npz'),
                        help="checkpoint container: 'tf' = TensorFlow V2 bundle (model.ckpt-N.index / .data-00000-of-00001 + `checkpoint`, the "
                             "layout tf.train.Saver writes and the reference restores, models/base_model.py:74-91); 'npz' (default) = one "
                             "numpy archive with the same variable names -- readable by this repo only")
    parser.add_argument('--batch-per-run', action='store_true',
                        help="feed a NEW batch to the G update like the reference's two sess.run (train.py:46-50); default: one batch per "
                             'step with a shared generator forward')
    parser.add_argument('--colors_seed', type=int, default=0,
                        help='seed of the key-point palette of the image summaries (the reference draws it from the unseeded random module)')
    parser.add_argument('--resume', type=str, default=None, metavar='latest|PATH',
                        help="continue from a checkpoint (an .npz or a bundle prefix): variables, Adam slots, beta powers and global_step; 'latest' = "
                             'the complete checkpoint with the highest step under <log_dir>/<mode>/, or a start from scratch when there is none, so '
                             'that one command line serves the first start and every restart.  Every trainable variable must be in it')
    parser.add_argument('--keep', type=int, default=None, metavar='N',
                        help='after each save, delete this mode\'s checkpoints beyond the newest N (default: keep all)')
    parser.add_argument('--guard', action='store_true',
                        help='skip the update of a bucket whose gradient holds a NaN or an Inf (parameters, Adam slots and batch-norm moving '
                             'statistics keep their bits) instead of writing it into every parameter; decided on the device, inside the captured step')
    parser.add_argument('--guard-max-skips', type=int, default=100, metavar='N',
                        help='--guard: stop the run when a bucket has skipped N updates in a row at a log point (default 100)')
    parser.add_argument('--ema', type=float, default=None, metavar='DECAY',
                        help="keep an exponential moving average of the generator's weights (0 < DECAY < 1, e.g. 0.999), updated on the device "
                             'inside the step; checkpoints carry it as <name>/ExponentialMovingAverage and --resume continues it')
    parser.add_argument('--ema-no-warmup', action='store_true',
                        help='--ema: the rate is 1 - DECAY from the first step (default: 1 - min(DECAY, (1 + step) / (10 + step)))')
    parser.add_argument('--ema-test', action='store_true',
                        help='--ema: at each test interval run the test pass a second time under the averaged weights and write it to '
                             '<log_dir>/<mode>/test_ema')
    parser.add_argument('--clip-norm', type=float, default=None, metavar='C',
                        help='clip each optimiser\'s gradient to global norm C (tf.clip_by_global_norm per bucket, C > 0), inside the Adam launch; '
                             'turns --guard on: a norm over non-finite values has no meaning, and the guard costs +0.08 %% of a step '
                             '(profiles/guard.txt).  The counters are not checkpointed and restart on --resume')
    parser.add_argument('--grad-stats', type=int, nargs='?', const=5, default=None, metavar='N',
                        help='at each log point, print the N (default 5) variables of largest gradient norm per bucket and, when the guard '
                             'counted a non-finite value in the last step, the name of every variable that holds one; at summary steps write '
                             'grad_norm/<variable> and update_ratio/<variable> = lr * grad_norm / param_norm')
    args = parser.parse_args(argv)
    if args.clip_norm is not None:
        if not args.clip_norm > 0.0:
            parser.error('--clip-norm C: C must be a number greater than 0 (got %r)' % args.clip_norm)
        args.guard = True
    if args.grad_stats is not None and args.grad_stats < 1:
        parser.error('--grad-stats N: N must be at least 1')
    if args.ema is not None and not (0.0 < args.ema < 1.0):
        parser.error('--ema DECAY: DECAY must lie strictly between 0 and 1 (got %r)' % args.ema)
    if (args.ema_test or args.ema_no_warmup) and args.ema is None:
        parser.error('--ema-test and --ema-no-warmup need --ema DECAY')
    if args.keep is not None and args.keep < 1:
        parser.error('--keep N keeps the newest N checkpoints: N must be at least 1')
    if args.guard_max_skips < 1:
        parser.error('--guard-max-skips N: N must be at least 1')
    if args.resume is not None and args.resume != 'latest':
        if not (os.path.isfile(args.resume) or os.path.isfile(args.resume + '.index')):
            parser.error('--resume %s: no such checkpoint (an .npz file, the prefix of a bundle, or the word latest)' % args.resume)
    if args.resident_data and (args.mode != 'detector_translator' or args.synthetic):
        parser.error('--resident-data keeps JPEG frames in HBM: the motion_generator and action_classifier modes read key-point files and '
                     '--synthetic reads no frames')
    if args.resident_labels and (args.mode not in ('motion_generator', 'action_classifier') or args.synthetic):
        parser.error('--resident-labels keeps pseudo labels in HBM: the detector_translator mode reads frames (see --resident-data) and '
                     '--synthetic reads no label files')
    return args


def main(argv=None):
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format='%(message)s')

    config = load_config(args.config)
    paths_config, train_config = config['paths'], config['training']
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if world > 1:
        torch.distributed.init_process_group('nccl', device_id=dev)

    import kpx_amd
    from kpx_amd.synthetic import synthetic_pair
    vgg = None
    if args.mode in ('motion_generator', 'action_classifier'):
        return _train_motion_generator(args, config, dev, rank, world)
    if args.synthetic_vgg or not os.path.exists(str(paths_config.get('vggnet'))):
        if not args.synthetic_vgg:
            raise Exception('file of pretrained vgg19 does not exist at: %s (pass --synthetic-vgg for benchmarking)' % paths_config.get('vggnet'))
        vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(), device=dev)
    size = config_image_size(config, args.image_size)
    model = _get_model_by_mode(args.mode, config, 0, device=dev, vgg=vgg, colors_seed=args.colors_seed, image_size=size,
                               **_guard_kw(args), **_ema_kw(args), **_clip_kw(args))
    print('model initialized')
    model.build(None)
    batch_size = train_config['batch_size']          # per process, like the reference's single-device batch
    train_it = test_it = None
    resumed = args.resume is not None and _resume(args, model, paths_config['log_dir'], rank, world, dev)
    if not args.synthetic:                           # reference train.py:125-135, 60-70: is_train -> random_order + randomness
        data_dir = paths_config['data_dir']
        if not os.path.exists(os.path.join(str(data_dir), 'train_set.txt')):
            raise Exception('no train_set.txt under paths.data_dir = %s (pass --synthetic for benchmarking)' % data_dir)
        import random
        import numpy as np
        random.seed(1000 + rank); np.random.seed(1000 + rank)          # different sample streams per data-parallel rank
        if resumed:
            _reseed_loaders(rank, model.global_step)
        train_it = iter(kpx_amd.ImagePairDataLoader(data_dir, 'train', random_order=True, randomness=True, image_size=size)
                        .batches(batch_size, dev, repeat=True, shuffle=True, resident=args.resident_data))
        if os.path.exists(os.path.join(str(data_dir), 'test_set.txt')):
            test_loader = kpx_amd.ImagePairDataLoader(data_dir, 'test', random_order=False, randomness=False, image_size=size)
            test_it = lambda: iter(test_loader.batches(batch_size, dev, repeat=False, shuffle=False, resident=args.resident_data))
    n_steps = args.steps if args.steps is not None else train_config['n_steps']
    model.initialize_loggers(paths_config['log_dir'], None)
    guard_log = _GuardLog(args.guard_max_skips) if args.guard else None
    clip_log = _ClipLog(args.grad_stats) if (args.clip_norm is not None or args.grad_stats is not None) else None
    print('training start')
    for step in range(model.global_step, n_steps):   # reference train.py:84-113
        should_write_log = step % train_config['log_interval'] == 0
        if train_it is not None:
            feed_dict = next(train_it)
            if args.batch_per_run:                   # the reference's input node serves a new batch to each of the two sess.run (:46-50)
                feed_dict = dict(feed_dict, **{k + '_G': v for k, v in next(train_it).items() if k in ('image', 'future_image')})
        else:
            pair = synthetic_pair(batch_size, res=model.image_size, seed0=2 * (step * world + rank), seed1=2 * (step * world + rank) + 1)
            feed_dict = {k: torch.from_numpy(v).to(dev) for k, v in pair.items()}
            if args.batch_per_run:
                s2 = 10 ** 7 + 2 * (step * world + rank)
                pair = synthetic_pair(batch_size, res=model.image_size, seed0=s2, seed1=s2 + 1)
                feed_dict.update({k + '_G': torch.from_numpy(v).to(dev) for k, v in pair.items()})
        should_write_summary = _should_write_summary(train_config, step, rank)
        model.train_step(None, feed_dict, step, batch_size, should_write_log=should_write_log and rank == 0,
                         should_write_summary=should_write_summary)
        if guard_log is not None and should_write_log and rank == 0:
            guard_log(model, step, should_write_summary)
        if clip_log is not None and step % train_config['log_interval'] == 0 and rank == 0:
            clip_log(model, step, should_write_summary)
        if step % train_config['checkpoint_interval'] == 0:
            _save(args, model, step, rank)
        if step % train_config['test_interval'] == 0 and rank == 0:
            def test_pass():
                if test_it is not None:              # reference train.py:97-110: one pass over the test subset
                    return [model.test_step(None, fd, step, i, fd['image'].shape[0]) for i, fd in enumerate(test_it())]
                tp = synthetic_pair(batch_size, res=model.image_size, seed0=10 ** 6, seed1=10 ** 6 + 1)
                return [model.test_step(None, {k: torch.from_numpy(v).to(dev) for k, v in tp.items()}, step, 0, batch_size)]
            model.collect_test_results(test_pass(), step)
            if args.ema_test:
                _test_under_ema(model, test_pass, step)
    model.close_loggers()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
