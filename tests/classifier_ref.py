"""Restatement of the key-point action classifier: float64 numpy versions of the three C entries (kpx_softmax_xent_fwd_f32,
kpx_softmax_xent_bwd_f32, kpx_class_scores_f32) and of the arrays evaluate.py --action-accuracy writes, and the classifier's forward / train
step on oracle.restatement._dynamic_rnn with torch-CPU autograd, in fp32 or fp64.  No GPU, no kpx_amd."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import restatement as R

FLT_MIN = float(np.finfo(np.float32).tiny)


# ------------------------------------------------------------------------------------------------ the three entries, float64
def lse(logits):
    x = np.asarray(logits, np.float32).astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(over='ignore', invalid='ignore'):
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def softmax_xent_fwd(logits, labels):
    """-> (loss float64, lse float64 [B]): mean_i -sum_j labels_ij (logits_ij - lse_i), the rows added in ascending order"""
    x, y = np.asarray(logits, np.float32).astype(np.float64), np.asarray(labels, np.float32).astype(np.float64)
    l = lse(x)
    rows = -(y * (x - l[:, None])).sum(axis=1)
    total = 0.0
    for r in rows:
        total += float(r)
    return total / x.shape[0], l


def softmax_xent_bwd(logits, labels, lse32, gscale_dev=None, gscale_host=1.0):
    """dlogits float64 [B,A] = g / B * (exp(logits - lse) - labels), lse the fp32 values of the forward, g = fl32(host * dev)"""
    x, y = np.asarray(logits, np.float32).astype(np.float64), np.asarray(labels, np.float32).astype(np.float64)
    g = np.float32(gscale_host) * (np.float32(gscale_dev) if gscale_dev is not None else np.float32(1.0))
    scale = float(g) / x.shape[0]
    return scale * (np.exp(x - np.asarray(lse32, np.float32).astype(np.float64)[:, None]) - y)


def class_scores(logits, target, confusion=None):
    """-> (pred int32 [M], rank int32 [M], logp float64 [M]); ``confusion`` int [A,A] is updated in place"""
    x = np.asarray(logits, np.float32)
    t = np.asarray(target).astype(np.int64)
    m, a = x.shape
    pred, rank, logp = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
    l = lse(x)
    for i in range(m):
        if not np.isfinite(x[i]).all():
            pred[i], rank[i], logp[i] = -1, a, np.nan
            continue
        pred[i] = int(np.argmax(x[i]))                                  # the first maximum
        rank[i] = 1 + int((x[i] >= x[i, t[i]]).sum()) - 1               # the others with logit >= the target's
        logp[i] = float(x[i, t[i]]) - l[i]
        if confusion is not None:
            confusion[t[i], pred[i]] += 1
    return pred, rank, logp


def ulps(got, want64, floor=0.0):
    """|got - fl32(want64)| in fp32 ulps taken at max(|fl32(want64)|, floor); NaN against NaN and equal infinities count 0"""
    got = np.asarray(got, np.float32)
    want = np.asarray(want64, np.float64).astype(np.float32)
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    ref = np.maximum(np.abs(want), np.float32(floor)).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        spacing = np.spacing(ref).astype(np.float64)
        out = np.abs(got.astype(np.float64) - want.astype(np.float64)) / spacing
    return np.where(same, 0.0, out)


# ------------------------------------------------------------------------------------------------ the classifier
def classifier_manifest(n_pts, n_action=9, cells=(256, 256)):
    out = OrderedDict()
    R._lstm_vars(out, 'seq_classifier/rnn', 2 * n_pts, cells)
    out['seq_classifier/fully_connected/weights'] = (cells[-1], n_action)
    out['seq_classifier/fully_connected/biases'] = (n_action,)
    return out


def init_classifier(n_pts, n_action=9, cells=(256, 256), seed=5, bias_scale=0.0):
    """Glorot-uniform matrices; ``bias_scale`` > 0 draws the biases too (the model initialises them to zero)"""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for name, shape in classifier_manifest(n_pts, n_action, cells).items():
        if len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rs.uniform(-lim, lim, size=shape).astype(np.float32)
        else:
            out[name] = (rs.randn(*shape) * bias_scale).astype(np.float32)
    return out


def classifier_forward(p, seq, cells):
    """seq [B,32,2K] (torch, the dtype of p) -> (logits [B,A], features [B,U])"""
    feats = R._dynamic_rnn(p, 'seq_classifier/rnn', seq, cells)[:, -1]
    return feats @ p['seq_classifier/fully_connected/weights'] + p['seq_classifier/fully_connected/biases'], feats


def classifier_loss(p, real_seq, action_code, cells):
    b = real_seq.shape[0]
    logits, feats = classifier_forward(p, real_seq.reshape(b, real_seq.shape[1], -1), cells)
    loss = -(action_code * torch.log_softmax(logits, dim=1)).sum(dim=1).mean()
    return loss, logits, feats


class ClassifierTrainState:
    def __init__(self, params, cells, lr_cfg=None, dtype=torch.float32):
        self.dtype, self.cells = dtype, tuple(cells)
        self.params = OrderedDict((k, torch.as_tensor(np.asarray(v)).clone().to(dtype)) for k, v in params.items())
        self.names = list(self.params)
        self.opt = R.AdamTF(self.names, self.params)
        self.global_step = 0
        self.lr_cfg = lr_cfg or {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}


def classifier_gradients(params, real_seq, action_code, cells, dtype=torch.float32):
    """-> ({name: gradient}, loss, logits) of one forward / backward at ``params`` in ``dtype``"""
    p = OrderedDict((k, torch.as_tensor(np.asarray(v)).clone().to(dtype).requires_grad_(True)) for k, v in params.items())
    loss, logits, _ = classifier_loss(p, torch.as_tensor(real_seq).to(dtype), torch.as_tensor(action_code).to(dtype), cells)
    gs = torch.autograd.grad(loss, list(p.values()))
    return {n: g.detach() for n, g in zip(p, gs)}, float(loss.detach()), logits.detach()


def classifier_train_step(state, real_seq, action_code):
    """ActionClassifierModel.train_step: forward, backward, tf.train.AdamOptimizer(lr, 0.5, 0.999) on every variable"""
    p = state.params
    rs, ac = (torch.as_tensor(a).to(state.dtype) for a in (real_seq, action_code))
    lr = R.exponential_decay(state.lr_cfg['start_val'], state.global_step, state.lr_cfg['step'], state.lr_cfg['decay'])
    for n in state.names:
        p[n].requires_grad_(True)
    loss, logits, _ = classifier_loss(p, rs, ac, state.cells)
    grads = R._grads(loss, p, state.names)
    state.opt.step(p, grads, lr)
    state.global_step += 1
    for n in state.names:
        p[n].requires_grad_(False)
    target = ac.argmax(dim=1)
    with torch.no_grad():
        own = logits.gather(1, target[:, None])
        n_correct = int(((logits >= own).sum(dim=1) == 1).sum())
    return dict(loss=float(loss.detach()), logits=logits.detach(), grads=grads, accuracy=n_correct / float(rs.shape[0]), lr=float(lr))


# ------------------------------------------------------------------------------------------------ evaluate.py's arrays
def accuracy_arrays(n_action, own, real_logits, pred_logits, actions=None, act_logits=None):
    """The cls_* arrays of metrics.npz from logits: own int [S], real_logits [S,A], pred_logits [S,D,A], act_logits [S,C,D,A]; logp float64"""
    own = np.asarray(own).astype(np.int64)
    s, d = pred_logits.shape[:2]
    out = {'cls_own': own.astype(np.int32)}
    conf = np.zeros((n_action, n_action), np.int32)
    out['cls_real_pred'], out['cls_real_rank'], out['cls_real_logp'] = class_scores(real_logits, own, conf)
    out['cls_confusion_real'] = conf
    conf = np.zeros((n_action, n_action), np.int32)
    p, r, l = class_scores(pred_logits.reshape(s * d, -1), np.repeat(own, d), conf)
    out.update(cls_pred_pred=p.reshape(s, d), cls_pred_rank=r.reshape(s, d), cls_pred_logp=l.reshape(s, d), cls_confusion_pred=conf)
    if actions is not None:
        c = len(actions)
        conf = np.zeros((n_action, n_action), np.int32)
        target = np.broadcast_to(np.asarray(actions, np.int64)[None, :, None], (s, c, d)).reshape(-1)
        p, r, l = class_scores(act_logits.reshape(s * c * d, -1), target, conf)
        out.update(cls_act_pred=p.reshape(s, c, d), cls_act_rank=r.reshape(s, c, d), cls_act_logp=l.reshape(s, c, d), cls_confusion_commanded=conf)
    return out
