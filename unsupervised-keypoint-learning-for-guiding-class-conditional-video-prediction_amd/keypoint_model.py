"""Inference-only key-point extractor (reference: models/keypoint_model.py) -- SURVEY 8f row 3, the first "next" row.

Runs ``pose_encoder`` with ``is_training=False`` (batch norm on the moving statistics, reference keypoint_model.py:48-50) over
whole videos and returns ``pts`` [B, T, K, 2].  The reference hard-codes T=663 and K=40 in a reshape (:52); here both follow
the input / config.  Frames are processed in slabs so a 663-frame video (9.7 GB of activations at once) stays bounded.
"""
import numpy as np
import torch

from . import networks, ops, variables
from .base_model import BaseModel
from .variables import Sym


class KeypointModel(BaseModel):
    name = 'stage1'                      # reference :18

    def __init__(self, config, device='cuda', image_size=128, frames_per_launch=128, seed=1234):
        super(KeypointModel, self).__init__(False)
        self.n_points = config['model']['n_pts']
        self.log_dir = config['paths']['log_dir']
        self.image_size = image_size
        self.frames_per_launch = frames_per_launch
        self.device = ops.normalize_device(device)
        self.store = variables.VariableStore(device=self.device, seed=seed)

    def build(self, inputs=None):
        """Declares the pose_encoder variables (same scopes as stage 1, so DetectorTranslatorModel checkpoints restore by
        name intersection, reference base_model.py:83-91)."""
        r = self.image_size
        with variables.as_default(self.store):
            networks.pose_encoder(Sym(1, r, r, 3), self.n_points, False, final_res=r)
        self.store.materialise()

    def run(self, sess, feed_dict):
        """reference run (:60-61).  feed_dict: {'image': [B,T,H,W,3] in [-1,1], 'idx': [B], 'len': [B]}."""
        im = feed_dict['image']
        b, t = im.shape[0], im.shape[1]
        pts = self._detect(im.reshape(b * t, self.image_size, self.image_size, 3))
        return {'pts': pts.reshape(b, t, self.n_points, 2), 'idx': feed_dict.get('idx'), 'len': feed_dict.get('len'), 'im': im}

    def _detect(self, frames):
        """pose_encoder over frames [M,H,W,3] in slabs of ``frames_per_launch`` -> pts [M,K,2] (``run``'s loop)."""
        outs = []
        with variables.as_default(self.store), torch.no_grad():
            for s in range(0, frames.shape[0], self.frames_per_launch):
                outs.append(networks.pose_encoder(frames[s:s + self.frames_per_launch].contiguous(), self.n_points, False,
                                                  final_res=self.image_size))
        return torch.cat(outs, dim=0) if len(outs) > 1 else outs[0]

    def stability(self, frames, coef_px, fwd, pts=None):
        """The detector's equivariance under given maps (not in the reference).  frames: fp32 [T,H,W,3] in [-1,1] on
        the model's device; coef_px, fwd: float64 [T,W,6] (``stability.draw_warps``): per frame W inverse maps in pixel units and the
        forward maps in normalised units; pts: the detector's [T,K,2] on ``frames`` where the caller has them (they are not detected
        again).  One ``ops.affine_warp`` launch makes the T*W warped frames (row t*W + w), the detector runs over them in slabs of
        ``frames_per_launch`` and one ``ops.equivariance_scores`` launch scores them.  -> {'pts' [T,K,2], 'pts_w' [T,W,K,2], 'scores'
        [T,W,K,2] = (err, moved), 'valid' uint8 [T,W,K], 'frame_mean' [T,W,2], 'n_valid' int32 [T,W]}, device tensors."""
        coef_px, fwd = np.ascontiguousarray(coef_px, np.float64), np.ascontiguousarray(fwd, np.float64)
        t = frames.shape[0]
        if coef_px.ndim != 3 or coef_px.shape[0] != t or coef_px.shape[2] != 6 or fwd.shape != coef_px.shape:
            raise ValueError('stability: coef_px and fwd must be [%d, W, 6] (got %s, %s)' % (t, coef_px.shape, fwd.shape))
        w = coef_px.shape[1]
        frames = frames.contiguous()
        dev = frames.device
        rows = torch.arange(t, dtype=torch.int32, device=dev).repeat_interleave(w).contiguous()
        warped = ops.affine_warp(frames, rows, torch.from_numpy(coef_px.reshape(t * w, 6)).to(dev))
        if pts is None:
            pts = self._detect(frames)
        pts = pts.reshape(t, self.n_points, 2).contiguous()
        pts_w = self._detect(warped).contiguous()
        del warped
        scores, valid, frame_mean, n_valid = ops.equivariance_scores(pts, pts_w, rows, torch.from_numpy(fwd.reshape(t * w, 6)).to(dev))
        k = self.n_points
        return {'pts': pts, 'pts_w': pts_w.reshape(t, w, k, 2), 'scores': scores.reshape(t, w, k, 2), 'valid': valid.reshape(t, w, k),
                'frame_mean': frame_mean.reshape(t, w, 2), 'n_valid': n_valid.reshape(t, w)}

    def train_step(self, sess, feed_dict, step, batch_size, should_write_log=False, should_write_summary=False):
        raise NotImplementedError          # reference :63-72: this model is not trainable

    def test_step(self, sess, feed_dict, step, test_idx, batch_size):
        raise NotImplementedError

    def collect_test_results(self, results, step):
        raise NotImplementedError
