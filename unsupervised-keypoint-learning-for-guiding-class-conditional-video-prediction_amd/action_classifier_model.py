"""Action recogniser over key-point sequences: the network behind evaluate.py --action-accuracy (no counterpart in the reference).

seq_classifier (stacked LSTM over the 32 key-point sets of a sequence, then a linear layer) -> logits [B,A]; the loss is
reduce_mean(softmax_cross_entropy_with_logits) against the sample's one-hot class.  It trains on the batches stage 2 trains on
(SequenceDataLoader: 'real_seq' and 'action_code'), with the optimiser of the other two models: tf.train.AdamOptimizer(lr, 0.5, 0.999)
over one flat bucket.  The LSTM layers, the linear layer, the loss, the scores and Adam are HIP kernels.
"""
import logging
import time
from datetime import datetime

import numpy as np
import torch

from . import networks, ops, summary, variables
from .base_model import BaseModel
from .variables import Sym

log = logging.getLogger('kpx')
N_FUTURE_FRAMES = 32
DEFAULT_CELLS = (256, 256)      # model.classifier_cells when the config has none: a judgement, not a measurement


class ActionClassifierModel(BaseModel):
    name = 'action_classifier'         # checkpoint / summary sub-directory

    def __init__(self, config, global_step=None, is_training=True, device='cuda', process_group=None, seed=777, guard=False, ema=None, ema_warmup=True,
                 clip_norm=None, grad_stats=False):
        super(ActionClassifierModel, self).__init__(is_training)
        self._ema_config(ema, ema_warmup)                  # train.py --ema: the averaged weights (BaseModel._ema_*)
        self._clip_config(clip_norm, grad_stats)           # train.py --clip-norm / --grad-stats: gradient norms (BaseModel._clip_*)
        self.guard = (bool(guard) or self.clip_norm is not None) and self.is_training      # train.py --guard: the step guard (BaseModel._guard_*); clipping reads its record
        train_config, model_config, paths_config = config['training'], config['model'], config['paths']
        self.lr = train_config['lr'] if self.is_training else None
        self.batch_size = train_config['batch_size']
        self.log_dir = paths_config['log_dir']
        self.n_points = model_config['n_pts']
        self.n_action = model_config.get('n_action', 9)
        self.cells = tuple(int(c) for c in model_config.get('classifier_cells', DEFAULT_CELLS))
        self.device = ops.normalize_device(device)
        self.global_step = int(global_step or 0)
        self.process_group = process_group
        self.world_size = torch.distributed.get_world_size(process_group) if (
            torch.distributed.is_available() and torch.distributed.is_initialized()) else 1
        self.store = variables.VariableStore(device=self.device, seed=seed)
        self.beta1, self.beta2, self.adam_eps = np.float32(0.5), np.float32(0.999), np.float32(1e-8)
        self.beta_power = [np.float32(0.5), np.float32(0.999)]
        self.last = {}

    def build(self, inputs=None):
        with variables.as_default(self.store):
            networks.seq_classifier(Sym(2, N_FUTURE_FRAMES, self.n_points * 2), self.n_action, self.cells)
        self.store.materialise(guard=self.guard, **({'ema': True} if self.ema is not None else {}))     # every variable lands in the 'G' bucket; 'D' stays empty and is never stepped
        self._guard_init(('G',))
        self._ema_init()
        if self.device.type == 'cuda':
            self._one = torch.ones(1, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------------------------------------ graph pieces
    def _sequences(self, seq):
        """[M,32,K,2] or [M,32,2K] -> contiguous [M,32,2K]"""
        if seq.dim() not in (3, 4) or seq.shape[1] != N_FUTURE_FRAMES or seq.numel() != seq.shape[0] * N_FUTURE_FRAMES * self.n_points * 2:
            raise ValueError('ActionClassifierModel: sequences must be [M,%d,%d,2] or [M,%d,%d] (got %s)'
                             % (N_FUTURE_FRAMES, self.n_points, N_FUTURE_FRAMES, self.n_points * 2, tuple(seq.shape)))
        return seq.reshape(seq.shape[0], N_FUTURE_FRAMES, self.n_points * 2).contiguous()

    def _forward(self, feed_dict):
        """-> (loss [1], logits [B,A], target int32 [B])"""
        labels = feed_dict['action_code'].contiguous()
        logits, _ = networks.seq_classifier(self._sequences(feed_dict['real_seq']), self.n_action, self.cells)
        logits = logits.contiguous()
        return ops.softmax_xent(logits, labels), logits, labels.argmax(dim=1).to(torch.int32)

    def classify(self, seq):
        """seq [M,32,K,2] or [M,32,2K] on the model's device -> (logits [M,A], features [M,U]), no gradients."""
        with variables.as_default(self.store), torch.no_grad():
            logits, features = networks.seq_classifier(self._sequences(seq), self.n_action, self.cells)
        return logits.contiguous(), features.contiguous()

    def current_lr(self):
        p = np.float32(self.global_step) / np.float32(self.lr['step'])
        return np.float32(np.float32(self.lr['start_val']) * np.power(np.float32(self.lr['decay']), p, dtype=np.float32))

    def _apply_adam(self, lr):
        bucket = self.store.buckets['G']
        ops.join_side_stream(self.device)
        if self.world_size > 1:                      # data parallel: one all-reduce of the flat bucket, 1/world folded into Adam
            torch.distributed.all_reduce(bucket.grads, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
        b1p, b2p = self.beta_power
        alpha = np.float32(np.float32(lr) * np.sqrt(np.float32(1) - b2p) / (np.float32(1) - b1p))
        if self.guard:                               # (after the exchange: every rank judges the same summed gradient)
            self._guarded_adam('G', alpha, gscale=1.0 / self.world_size)
        else:
            ops.adam_tf_flat_(bucket.params, bucket.grads, bucket.m, bucket.v, alpha, self.beta1, self.beta2, self.adam_eps,
                              gscale=1.0 / self.world_size)
        self._ema_update('G', self.global_step, self._ema_health('G'))     # (global_step before its increment: the update's index)
        self.store.touch()
        self.beta_power = [np.float32(b1p * self.beta1), np.float32(b2p * self.beta2)]

    @staticmethod
    def _n_correct(logits, target):
        """Rows whose target class ranks first (ops.class_scores: a tie counts against the model)."""
        _, rank, _ = ops.class_scores(logits, target, check_target=False)        # the arg max of a one-hot row lies in [0, A)
        return int((rank == 1).sum())

    # ------------------------------------------------------------------------------------------------ model surface
    def train_step(self, sess, feed_dict, step, batch_size, should_write_log=False, should_write_summary=False):
        """feed_dict: 'real_seq' [B,32,K,2] and 'action_code' [B,A] (the SequenceDataLoader batch; other keys are ignored)."""
        self._ema_forbid_training()
        start_time = time.time()
        lr = self.current_lr()
        with variables.as_default(self.store):
            loss, logits, target = self._forward(feed_dict)
            ops.begin_backward()
            torch.autograd.backward([loss], [self._one])
            self._apply_adam(lr)
        self.global_step += 1
        self.last = dict(loss=loss.detach(), logits=logits.detach(), target=target, lr=float(lr))
        if should_write_summary and self.train_writer is not None:
            self._write_summaries(self.train_writer, step, self._summaries(self.loss_values()) + [[summary.scalar_value('lr', self.last['lr'])]]
                                  + self._ema_summary())
        if should_write_log:
            v = self.loss_values()
            duration = time.time() - start_time
            log.info('%s: step %d, loss = %.4f, accuracy = %.3f (%.1f examples/sec) %.3f sec/batch',
                     datetime.now(), step, v['loss'], v['accuracy'], batch_size / float(duration), duration)

    def loss_values(self):
        """The last train step's loss, the accuracy of its batch before the update, and its learning rate."""
        n = self.last['logits'].shape[0]
        return dict(loss=float(self.last['loss'].cpu()[0]), accuracy=self._n_correct(self.last['logits'], self.last['target']) / float(n),
                    lr=self.last['lr'])

    def test_step(self, sess, feed_dict, step, test_idx, batch_size):
        """One forward, no update -> (loss, n_correct, duration, batch_size)."""
        start_time = time.time()
        with variables.as_default(self.store), torch.no_grad():
            loss, logits, target = self._forward(feed_dict)
        loss_h, n_correct = float(loss.cpu()[0]), self._n_correct(logits, target)
        duration = time.time() - start_time
        if test_idx == 0 and self.test_writer is not None:
            self._write_summaries(self.test_writer, step, self._summaries(dict(loss=loss_h, accuracy=n_correct / float(logits.shape[0]))))
        return loss_h, n_correct, duration, batch_size

    @staticmethod
    def _summaries(vals):
        return [[summary.scalar_value('xent_loss', vals['loss']), summary.scalar_value('accuracy', vals['accuracy'])]]

    def collect_test_results(self, results, step):
        """-> (mean loss weighted by the batch sizes, accuracy) over one test pass."""
        n = sum(x[3] for x in results)
        average_loss = sum(x[0] * x[3] for x in results) / n
        accuracy = sum(x[1] for x in results) / float(n)
        total_duration = sum(x[2] for x in results)
        log.info('test: %s: step %d, loss = %.4f, accuracy = %.3f (%.1f examples/sec) %.3f sec/batch', datetime.now(), step,
                 average_loss, accuracy, n / total_duration, total_duration / len(results))
        return average_loss, accuracy

    def checkpoint_arrays(self):
        arrays = self.store.export_numpy(include_slots=self.is_training)
        arrays['global_step'] = np.int32(self.global_step)
        if self.is_training:
            arrays.update({'beta1_power': self.beta_power[0], 'beta2_power': self.beta_power[1]})
        return arrays

    def restore(self, sess, checkpoint_path, strict=False, ema=False):
        """BaseModel.restore; ``strict`` (evaluate.py --action-accuracy): every seq_classifier variable must be in the checkpoint with this
        model's shape -- a recogniser trained at another width cannot score anything.  ``ema``: read it under its averages (BaseModel.restore)."""
        if strict:
            from .ema import read_selected
            arrays = read_selected(checkpoint_path) if ema else self.read_checkpoint(checkpoint_path)
            bad = ['%s: %s' % (n, 'missing' if n not in arrays else 'checkpoint %s, model %s' % (tuple(arrays[n].shape), tuple(v.shape)))
                   for n, v in self.store.vars.items() if n not in arrays or tuple(arrays[n].shape) != tuple(v.shape)]
            if bad:
                raise Exception('%s is not an action_classifier checkpoint for model.classifier_cells = %s, n_pts = %d, n_action = %d '
                                '(train.py --mode action_classifier writes one; the config must name the cells it was trained with): %s'
                                % (checkpoint_path, list(self.cells), self.n_points, self.n_action, '; '.join(bad)))
        return super(ActionClassifierModel, self).restore(sess, checkpoint_path, ema=ema)

    def _restore_extra(self, arrays):
        if 'global_step' in arrays:
            self.global_step = int(arrays['global_step'])
        if 'beta1_power' in arrays:
            self.beta_power = [np.float32(arrays['beta1_power']), np.float32(arrays['beta2_power'])]
        if self.is_training:                 # the Adam slots, as DetectorTranslatorModel restores its own: training continues bit for bit
            b = self.store.buckets['G']
            with torch.no_grad():
                for name in b.entries:
                    for slot, flat in (('/Adam', b.m), ('/Adam_1', b.v)):
                        if name + slot in arrays:
                            b.view(flat, name).copy_(torch.from_numpy(np.ascontiguousarray(arrays[name + slot], np.float32)).to(flat.device))
