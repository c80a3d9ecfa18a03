"""Abstract model API with the reference's method names (reference: models/base_model.py:7-92).

``sess`` arguments are kept for signature parity and ignored (there is no session: kernels are launched eagerly on the
current HIP stream).  Checkpoints keep the reference's location ``<log_dir>/<name>/model.ckpt-<step>`` and variable
names, in an ``.npz`` container (default) or as a TensorFlow V2 checkpoint bundle (``tf_bundle.py``, SURVEY 8f-2;
``KPX_CKPT_FORMAT=tf``).
"""
import contextlib
import logging
import os
import re
from abc import ABC, abstractmethod
from os import path as osp

import numpy as np
import torch

TMP_SUFFIX = '.tmp'                # a checkpoint file being written; renamed into place when it is whole (tf_bundle.TMP_SUFFIX)
_CKPT_FILE = re.compile(r'^model\.ckpt-(\d+)\.(npz|index)$')
_RNG_FILE = re.compile(r'^model\.ckpt-(\d+)\.rng-(\d+)\.npz$')
log = logging.getLogger('kpx')
_COUNTERS = ('global_step', 'beta1_power', 'beta2_power', 'beta1_power_1', 'beta2_power_1')


class BaseModel(ABC):
    name = 'base_model'
    trainable = True

    def __init__(self, is_training=True):
        super(BaseModel, self).__init__()
        self.is_training = is_training
        self.log_dir = None
        self.store = None
        self.train_writer = None
        self.test_writer = None
        self.test_ema_writer = None

    @abstractmethod
    def build(self, inputs):
        raise NotImplementedError

    @abstractmethod
    def train_step(self, sess, feed_dict, step, batch_size, should_write_log=False, should_write_summary=False):
        raise NotImplementedError

    @abstractmethod
    def test_step(self, sess, feed_dict, step, test_idx, batch_size):
        raise NotImplementedError

    @abstractmethod
    def collect_test_results(self, results, step):
        raise NotImplementedError

    def initialize_loggers(self, log_dir, sess=None):
        """reference :62-75: the checkpoint directory, and -- for a training model on rank 0 -- the TensorBoard event writers of
        ``<log_dir>/<name>/train`` and ``<log_dir>/<name>/test`` (summary.EventFileWriter).  The reference's train writer also records
        ``sess.graph``; there is no TF graph here, so that event is not written."""
        self.log_dir = log_dir
        name = self.__class__.name
        os.makedirs(osp.join(log_dir, name), exist_ok=True)
        rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
        if self.is_training and rank == 0:
            from .summary import EventFileWriter
            self.close_loggers()
            self.train_writer = EventFileWriter(osp.join(log_dir, name, 'train'))
            self.test_writer = EventFileWriter(osp.join(log_dir, name, 'test'))
            if self.ema is not None:       # train.py --ema-test: the test pass under the averages, <log_dir>/<name>/test_ema
                self.test_ema_writer = EventFileWriter(osp.join(log_dir, name, 'test_ema'))

    def close_loggers(self):
        for w in (self.train_writer, self.test_writer, self.test_ema_writer):
            if w is not None:
                w.close()
        self.train_writer = self.test_writer = self.test_ema_writer = None

    def _write_summaries(self, writer, step, summaries):
        """One add_summary per merged summary, in order (the reference's add_summary calls)."""
        if writer is not None:
            for values in summaries:
                writer.add_summary(values, step)

    # ---- the step guard (guard=True of the training models, train.py --guard) -------------------------------------------------------
    # A bucket whose exchanged gradient holds a NaN or an Inf skips its update: parameters, Adam slots and the batch-norm moving
    # statistics the bucket owns keep the bits they had before the step.  The verdict is one KpxGuardHealth record per bucket in device
    # memory, written by the health pass and read by the update and the restore themselves, so every launch is part of the captured step
    # and the host never learns of a skip: beta powers and global_step advance as on any other step (the bias correction then runs a few
    # steps ahead of the slots, which is harmless).  Only guard_report() reads the records back.
    guard = False
    draws_on_device = False            # a model whose train step draws from torch's device generator (stage 2): see save_rng_state

    def _guard_init(self, buckets):
        """After store.materialise(): the health record, the health pass's workspace and the device-side step size of every non-empty bucket."""
        self._guard_health, self._guard_work, self._guard_alpha, self._clip_state = {}, {}, {}, {}
        self._grad_stats_init(buckets)
        if not self.guard:
            return
        from . import ops
        for which in buckets:
            bucket = self.store.buckets[which]
            if bucket.size:
                self._guard_health[which] = ops.new_guard_health(self.device)
                self._guard_work[which] = ops.grad_health_workspace(bucket.grads.numel(), self.device)
                self._guard_alpha[which] = torch.zeros(1, dtype=torch.float32, device=self.device)
                if self.clip_norm is not None:
                    self._clip_state[which] = ops.new_clip_state(self.device)

    def _guard_shadow_moving(self):
        """Before the forward: the moving statistics as they stand, into their shadows (one copy per owner bucket; nothing without guard)."""
        if self.guard:
            from . import ops
            for which, live in self.store.moving.items():
                ops.flat_copy_raw(live.data_ptr(), self.store.moving_shadow[which].data_ptr(), live.numel())

    def _guarded_adam(self, which, alpha=None, alpha_dev=None, gscale=1.0):
        """Health pass over the bucket's (exchanged) gradient, the guarded update in the place of the plain one, and the restore of the
        moving statistics the bucket owns.  ``alpha``: the step size as a host number, written into the device float first (the eager
        form); None when the caller has refreshed ``alpha_dev`` itself (a captured launch, whose arguments are frozen)."""
        from . import ops
        bucket, health = self.store.buckets[which], self._guard_health[which]
        alpha_dev = self._guard_alpha[which] if alpha_dev is None else alpha_dev
        if alpha is not None:
            ops.fill_raw_(alpha_dev, float(alpha))
        ops.grad_health(bucket.grads, health, self._guard_work[which])
        if self.clip_norm is not None:      # clip_norm=C: the same launch geometry, the gradient scaled down when its norm exceeds C
            ops.adam_tf_flat_clipped_(bucket.params, bucket.grads, bucket.m, bucket.v, alpha_dev, self.beta1, self.beta2, self.adam_eps, health,
                                      self._clip_state[which], self.clip_norm, gscale=gscale)
        else:
            ops.adam_tf_flat_guarded_(bucket.params, bucket.grads, bucket.m, bucket.v, alpha_dev, self.beta1, self.beta2, self.adam_eps, health,
                                      gscale=gscale)
        live = self.store.moving.get(which)
        if live is not None:
            ops.guard_restore_(live, self.store.moving_shadow[which], health)

    def guard_report(self):
        """{bucket: skipped_total, skipped_run, updates, and of the last step nonfinite, grad_norm = gscale * sqrt(sum g^2) and max_abs over the
        finite gradient values}.  Synchronises; nothing else reads the health records from the host."""
        if not self.guard:
            raise ValueError('%s was built without guard=True: there is nothing to report' % self.__class__.name)
        from . import ops
        gscale = 1.0 / float(getattr(self, 'world_size', 1))
        out = {}
        for which, health in self._guard_health.items():
            h = ops.read_guard_health(health)
            out[which] = dict(skipped_total=h['skipped_total'], skipped_run=h['skipped_run'], updates=h['updates'], nonfinite=h['nonfinite'],
                              grad_norm=gscale * float(np.sqrt(h['sumsq'])), max_abs=h['maxabs'])
        return out

    # ---- gradient norms (clip_norm=C and grad_stats=True of the training models, train.py --clip-norm / --grad-stats) -----------------
    # clip_norm=C is tf.clip_by_global_norm over each bucket, per optimiser ('D' and 'G' clip separately): the guarded update's launch reads
    # the sum of squares the health pass already left in the bucket's record and scales the gradient by C / norm when norm > C
    # (kpx_adam_tf_flat_clipped_f32).  It needs the guard -- a norm over non-finite values has no meaning --, so clip_norm turns guard on.
    # One KpxClipState record per bucket in device memory holds the last norm, the last scale and the count of clipped updates; only
    # clip_report() reads it back.  grad_stats=True builds the segment table of every bucket once; grad_stats() then runs eagerly, outside
    # any capture, over bucket.grads, which still hold the step's exchanged gradient after train_step returns (no model clears them).
    # Neither is written into checkpoints: the counters restart on resume.
    clip_norm = None                   # the bound on gscale * ||g||, a float > 0; None: the guarded (or plain) update, exactly as before
    grad_stats_on = False

    def _clip_config(self, clip_norm, grad_stats=False):
        """Constructor half, before ``self.guard`` is set: check and keep the bound (training models only; a model that never steps has no
        gradient to clip, so the keyword is refused there)."""
        if clip_norm is not None:
            if not self.is_training:
                raise ValueError('clip_norm is for training models: %s with is_training=False never takes a step' % self.__class__.name)
            if isinstance(clip_norm, bool) or not isinstance(clip_norm, (int, float, np.floating, np.integer)) or not float(clip_norm) > 0.0:
                raise ValueError('clip_norm must be a number > 0 (got %r)' % (clip_norm,))
            self.clip_norm = float(clip_norm)
        if grad_stats and not self.is_training:
            raise ValueError('grad_stats is for training models: %s with is_training=False has no gradients' % self.__class__.name)
        self.grad_stats_on = bool(grad_stats)

    def _grad_stats_init(self, buckets):
        """The segment table, workspace and result records of every non-empty bucket (grad_stats=True only)."""
        self._seg = {}
        if not self.grad_stats_on or self.device.type != 'cuda':
            return
        from . import ops
        for which in buckets:
            bucket = self.store.buckets[which]
            if bucket.size:
                table = ops.grad_segment_table(bucket, self.device)
                self._seg[which] = (table,) + ops.grad_segment_workspace(table, self.device)

    def clip_report(self):
        """{bucket: norm = gscale * ||g|| and scale of the last update that was not skipped, clipped_total}.  Synchronises."""
        if self.clip_norm is None:
            raise ValueError('%s was built without clip_norm=C: there is nothing to report' % self.__class__.name)
        from . import ops
        return {which: ops.read_clip_state(clip) for which, clip in self._clip_state.items()}

    def grad_stats(self):
        """{bucket: {variable: grad_norm (gscale * ||g|| over the finite values), param_norm, max_abs, nonfinite}} of the gradient the last
        train_step left in the buckets.  Eager (two launches per bucket) and synchronising: call it between steps, never inside a capture."""
        if not self.grad_stats_on:
            raise ValueError('%s was built without grad_stats=True: there is no segment table' % self.__class__.name)
        from . import ops
        gscale = 1.0 / float(getattr(self, 'world_size', 1))
        report = {}
        for which, (table, work, out) in self._seg.items():
            bucket = self.store.buckets[which]
            rec = ops.read_segment_stats(ops.grad_segment_stats(bucket.grads, bucket.params, table, work, out))
            report[which] = {name: dict(grad_norm=gscale * float(np.sqrt(rec['sumsq_g'][i])), param_norm=float(np.sqrt(rec['sumsq_p'][i])),
                                        max_abs=float(rec['maxabs_g'][i]), nonfinite=int(rec['nonfinite_g'][i]))
                             for i, name in enumerate(table.names)}
        return report

    # ---- the averaged generator (ema=DECAY of the training models, train.py --ema) --------------------------------------------------
    # Bucket 'G' -- the bucket inference reads in every mode -- keeps an exponential moving average of its parameters in a fifth flat buffer
    # (Bucket.ema): ema += (p - ema) * rate after every 'G' Adam update, one kpx_ema_flat_f32 launch behind the Adam launch on its stream.
    # The rate lives in a [1] device float that is refreshed on the host where the Adam step size is (before each eager launch, before each
    # graph or segment replay, never inside a capture), so the launch is part of the captured step.  With guard=True the launch reads the
    # bucket's health record and a skipped update is no step for the average either; the schedule's index t = global_step before its
    # increment advances on a skipped step all the same, as beta powers and global_step do (the warm-up then runs a few steps ahead of the
    # average, which is harmless).  'D' is never averaged; batch-norm moving statistics are not trainable and are not averaged either:
    # inference under the averages reads the live ones.
    ema = None                         # the decay, a float in (0, 1); None: no averages (nothing below allocates or launches anything)
    ema_warmup = True                  # rate = 1 - min(decay, (1 + t) / (10 + t)), tf.train.ExponentialMovingAverage(decay, num_updates=t)
    _ema_active = False                # inside ema_weights()

    def _ema_config(self, ema, ema_warmup=True):
        """Constructor half: check and keep the decay (training models only)."""
        if ema is not None and self.is_training:
            if not (isinstance(ema, (int, float, np.floating)) and 0.0 < float(ema) < 1.0):
                raise ValueError('ema must be a decay with 0 < ema < 1 (got %r)' % (ema,))
            self.ema, self.ema_warmup = float(ema), bool(ema_warmup)

    def _ema_init(self):
        """After store.materialise(ema=...): the device float the launches read their rate from."""
        self._ema_rate_dev = self._ema_last_rate = None
        if self.ema is not None and self.device.type == 'cuda':
            self._ema_rate_dev = torch.zeros(1, dtype=torch.float32, device=self.device)

    def ema_rate(self, step):
        """The float32 step of the average at update index ``step`` (ema.rate, the one definition)."""
        from . import ema
        return ema.rate(self.ema, step, self.ema_warmup)

    def _ema_refresh(self, step):
        """The rate of update index ``step`` into the device float (host side: before an eager launch or a replay, never in a capture)."""
        from . import ops
        self._ema_last_rate = float(self.ema_rate(step))
        ops.fill_raw_(self._ema_rate_dev, self._ema_last_rate)

    def _ema_update(self, which, step, health=None):
        """Behind the Adam launch of bucket ``which``: nothing unless the bucket is averaged.  ``step``: the update's index (global_step
        before the increment), written into the device float first; None when the caller refreshes it itself (a captured launch, whose
        arguments are frozen).  ``health``: the bucket's guard record, or None."""
        bucket = self.store.buckets[which]
        if self.ema is None or bucket.ema is None:
            return
        from . import ops
        if step is not None:
            self._ema_refresh(step)
        ops.ema_flat_(bucket.ema, bucket.params, self._ema_rate_dev, health)

    def _ema_health(self, which):
        return self._guard_health.get(which) if self.guard else None

    def _ema_summary(self):
        """The train summaries' one more scalar, ema/rate of the step just taken ([] without ema)."""
        if self.ema is None or self._ema_last_rate is None:
            return []
        from . import summary
        return [[summary.scalar_value('ema/rate', self._ema_last_rate)]]

    def _ema_forbid_training(self):
        if self._ema_active:
            raise RuntimeError('train_step inside ema_weights(): the parameters are the averages there; leave the context first')

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model's 'G' variables ARE the averages (and Bucket.ema holds the parameters): one swap launch in place,
        so no address changes and captured graphs stay valid.  Leaving -- also by an exception -- swaps back.  Not reentrant; train_step
        inside is an error.  The batch-norm moving statistics are the live ones either way."""
        if self.ema is None:
            raise ValueError('%s was built without ema=DECAY: there are no averaged weights' % self.__class__.name)
        if self._ema_active:
            raise RuntimeError('ema_weights() is already active: the context does not nest')
        from . import ops
        bucket = self.store.buckets['G']
        ops.swap_flat_(bucket.params, bucket.ema)
        self.store.touch('G')
        self._ema_active = True
        try:
            yield self
        finally:
            ops.swap_flat_(bucket.params, bucket.ema)
            self.store.touch('G')
            self._ema_active = False

    def _restore_ema(self, arrays, checkpoint_path):
        """The averages' half of restore / resume, after the parameters are in place.  -> shadow keys in the checkpoint."""
        from .ema import SUFFIX
        n_shadows = sum(1 for n in arrays if n.endswith(SUFFIX))
        if self.ema is not None:
            found, missing = self.store.load_ema_numpy(arrays)
            if found == 0:
                log.info('%s holds no averaged weights: the averages start as the restored parameters', checkpoint_path)
            elif missing:
                log.info('%s holds averages of %d of %d variables: the others start as the restored parameters', checkpoint_path, found, found + missing)
        elif n_shadows and self.is_training:
            log.info('%s holds %d averaged weights, which this run (without ema) ignores: the next checkpoint will not carry them', checkpoint_path, n_shadows)
        return n_shadows

    def checkpoint_arrays(self):
        """Everything tf.train.Saver(tf.global_variables()) would hold (reference :74)."""
        return self.store.export_numpy(include_slots=self.is_training)

    def save_checkpoint(self, sess, step, fmt=None, keep=None):
        """reference :77-81 -> <log_dir>/<name>/model.ckpt-<step>.  ``fmt`` (or $KPX_CKPT_FORMAT): 'npz' (default, one file) or
        'tf' = a TensorFlow V2 bundle (.index + .data-00000-of-00001 + ``checkpoint``) that tf.train.Saver can restore.  Either container is
        written under a temporary name in the same directory and renamed into place: a write that fails or is killed leaves the checkpoint
        before it the newest one latest_checkpoint finds.  ``keep``: after the save, prune_checkpoints(keep)."""
        fmt = fmt or os.environ.get('KPX_CKPT_FORMAT', 'npz')
        if fmt not in ('npz', 'tf', 'bundle'):           # ('bundle' = 'tf'; anything else is a typo that must not silently write the other container)
            raise ValueError("checkpoint format %r: expected 'npz', 'tf' or 'bundle' (KPX_CKPT_FORMAT / --ckpt-format)" % (fmt,))
        prefix = osp.join(self.log_dir, self.__class__.name, 'model.ckpt-%d' % step)
        if fmt in ('tf', 'bundle'):
            from . import tf_bundle
            tf_bundle.write_bundle(prefix, self.checkpoint_arrays())
            path = prefix
        else:
            path = prefix + '.npz'
            tmp = path + TMP_SUFFIX
            try:
                with open(tmp, 'wb') as f:
                    np.savez(f, **{k.replace('/', '|'): v for k, v in self.checkpoint_arrays().items()})
                    f.flush()
                    os.fsync(f.fileno())
                os.replace(tmp, path)
            except BaseException:
                if osp.exists(tmp):
                    os.remove(tmp)
                raise
        if keep is not None:
            self.prune_checkpoints(keep)
        return path

    # ---- finding, pruning and resuming ----------------------------------------------------------------------------------------------
    @classmethod
    def list_checkpoints(cls, log_dir):
        """[(step, path, container)] of the COMPLETE checkpoints under <log_dir>/<name>/, ascending by step (numpy and the standard library
        only).  An .npz is complete when it opens as a zip archive and lists global_step; a bundle when its .index parses and its data file
        has the length the index implies (tf_bundle.bundle_complete).  Anything else -- temporary files of a write in progress, truncated
        files, other models' files -- is neither listed nor touched."""
        import zipfile
        from . import tf_bundle
        directory = osp.join(str(log_dir), cls.name)
        if not osp.isdir(directory):
            return []
        found = []
        for f in sorted(os.listdir(directory)):
            m = _CKPT_FILE.match(f)
            if m is None:
                continue
            step, path = int(m.group(1)), osp.join(directory, f)
            if m.group(2) == 'npz':
                try:
                    with zipfile.ZipFile(path) as z:
                        whole = 'global_step.npy' in z.namelist()
                except (OSError, zipfile.BadZipFile):
                    whole = False
                if whole:
                    found.append((step, path, 'npz'))
            elif tf_bundle.bundle_complete(path[:-len('.index')]):
                found.append((step, path[:-len('.index')], 'tf'))
        return sorted(found)

    @classmethod
    def latest_checkpoint(cls, log_dir):
        """(path, step) of the complete checkpoint with the highest step under <log_dir>/<name>/, in either container, or None."""
        found = cls.list_checkpoints(log_dir)
        return (found[-1][1], found[-1][0]) if found else None

    def rng_state_path(self, step, rank, directory=None):
        return osp.join(directory or osp.join(self.log_dir, self.__class__.name), 'model.ckpt-%d.rng-%d.npz' % (step, rank))

    def prune_checkpoints(self, keep):
        """Delete this model's complete checkpoints beyond the newest ``keep`` (by step, either container) with their generator-state side
        files, and list the surviving bundles in the ``checkpoint`` state file if there is one.  Only what list_checkpoints recognises as a
        whole checkpoint of this model is ever deleted.  -> the paths deleted."""
        from . import tf_bundle
        if int(keep) < 1:
            raise ValueError('keep must be at least 1 (got %r)' % (keep,))
        directory = osp.join(self.log_dir, self.__class__.name)
        found = self.list_checkpoints(self.log_dir)
        steps = sorted({step for step, _, _ in found})
        doomed = set(steps[:-int(keep)])
        removed = []
        for step, path, container in found:
            if step not in doomed:
                continue
            files = [path] if container == 'npz' else [path + '.index', path + '.data-00000-of-00001']     # the index first: no longer a checkpoint
            files += [osp.join(directory, f) for f in sorted(os.listdir(directory)) if _RNG_FILE.match(f) and int(_RNG_FILE.match(f).group(1)) == step]
            for f in files:
                if osp.exists(f):
                    os.remove(f)
                    removed.append(f)
        bundles = [osp.basename(path) for step, path, container in found if container == 'tf' and step not in doomed]
        if doomed and bundles and osp.exists(osp.join(directory, 'checkpoint')):
            tf_bundle.write_checkpoint_state(directory, bundles)
        return removed

    def trainable_names(self):
        return [n for n, (shape, kind) in self.store.specs.items() if self.store.is_trainable(kind)]

    def resume(self, sess, checkpoint_path):
        """train.py --resume: restore() made strict.  Every trainable variable of the model must be in the checkpoint with the model's
        shape (the fused translator head counts through its two reference variables); otherwise nothing is restored and the exception names
        the variables.  -> (restored global_step, variables restored, Adam slots restored)."""
        arrays = self.read_checkpoint(checkpoint_path)
        bad = []
        for name in self.trainable_names():
            want = tuple(self.store.vars[name].shape)
            if '_0+1/' in name:
                parts = [(name.replace('_0+1/', '_0/'), want[:-1] + (3,)), (name.replace('_0+1/', '_1/'), want[:-1] + (want[-1] - 3,))]
            else:
                parts = [(name, want)]
            for n, shape in parts:
                if n not in arrays:
                    bad.append('%s: missing' % n)
                elif tuple(arrays[n].shape) != shape:
                    bad.append('%s: checkpoint %s, model %s' % (n, tuple(arrays[n].shape), shape))
        if bad:
            raise Exception('cannot resume %s from %s: %d trainable variable(s) do not match: %s'
                            % (self.__class__.name, checkpoint_path, len(bad), '; '.join(bad)))
        self.store.load_numpy(arrays, strict=False)
        self._restore_extra(arrays)
        from .ema import SUFFIX
        n_shadows = self._restore_ema(arrays, checkpoint_path)
        if n_shadows and self.ema is not None:
            log.info('%d averaged weights restored from %s', n_shadows, checkpoint_path)
        n_vars = sum(1 for n in arrays if not n.endswith(('/Adam', '/Adam_1', SUFFIX)) and n not in _COUNTERS)     # (shadows are not variables)
        n_slots = sum(1 for n in arrays if n.endswith(('/Adam', '/Adam_1')))
        return int(getattr(self, 'global_step', 0)), n_vars, n_slots

    def save_rng_state(self, step, rank):
        """The torch CPU and device generator states of this rank beside checkpoint ``step`` (model.ckpt-<step>.rng-<rank>.npz): what a
        model that draws on the device (stage 2's eps_D / eps_G) needs to continue its noise stream bit for bit."""
        path = self.rng_state_path(step, rank)
        state = {'cpu': torch.get_rng_state().numpy()}
        if self.device.type == 'cuda':
            state['device'] = torch.cuda.get_rng_state(self.device).numpy()
        with open(path + TMP_SUFFIX, 'wb') as f:
            np.savez(f, **state)
        os.replace(path + TMP_SUFFIX, path)
        return path

    def load_rng_state(self, step, rank, directory=None):
        """-> True when this rank's side file of checkpoint ``step`` was there (in ``directory``, by default this model's checkpoint
        directory) and the generators continue from it."""
        path = self.rng_state_path(step, rank, directory)
        if not osp.exists(path):
            return False
        with np.load(path) as data:
            torch.set_rng_state(torch.from_numpy(data['cpu'].copy()))
            if 'device' in data.files and self.device.type == 'cuda':
                torch.cuda.set_rng_state(torch.from_numpy(data['device'].copy()), self.device)
        return True

    def restore(self, sess, checkpoint_path, ema=False):
        """reference :83-91: restore the intersection of checkpoint variables and model variables, by name.  Accepts the .npz
        container or the prefix of a TensorFlow V2 bundle (e.g. the published stage-1 / stage-2 checkpoints).  ``ema`` (the --ema of the
        inference tools): read the checkpoint under its averages (ema.select); one without averages is refused by name."""
        if ema:
            from .ema import read_selected
            arrays = read_selected(checkpoint_path)
        else:
            arrays = self.read_checkpoint(checkpoint_path)
        self._check_restore(arrays, checkpoint_path)
        self.store.load_numpy(arrays, strict=False)
        self._restore_extra(arrays)
        self._restore_ema(arrays, checkpoint_path)
        return sorted(arrays)

    def _check_restore(self, arrays, checkpoint_path):
        """What a model asks of a checkpoint beyond the reference's restore-by-intersection; raises before anything is loaded."""

    @staticmethod
    def read_checkpoint(checkpoint_path):
        """{variable name: array} of either container"""
        from . import tf_bundle
        if tf_bundle.is_bundle(checkpoint_path):
            return tf_bundle.read_bundle(checkpoint_path)
        data = np.load(checkpoint_path)
        return {k.replace('|', '/'): data[k] for k in data.files}

    def _restore_extra(self, arrays):
        pass
