"""Synthetic Penn-shaped inputs: the output contract of the reference's ImagePairDataLoader
(data/image_pair_dataloader.py:38-48,65-70): float32 NHWC in [-1,1], keys 'image' and 'future_image'."""
import numpy as np


def synthetic_pair(batch, res=128, seed0=0, seed1=1):
    def one(seed):
        u = np.random.RandomState(seed).randint(0, 256, size=(batch, res, res, 3)).astype(np.float32)
        return (u / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)   # map_fn: x/255*2-1
    return {'image': one(seed0), 'future_image': one(seed1)}


def planted_action_batch(batch, n_points, n_action, seed=0, n_frames=32, drift=0.4, noise=0.01):
    """A planted action-recognition problem with the SequenceDataLoader batch contract (float32 'keypoints' [B,K,2], 'real_seq'
    [B,32,K,2], one-hot 'action_code' [B,A]): every point of a sample drifts linearly from its random start in the direction
    2 pi c / A that its class c decides, ``drift`` over the sequence, plus a little Gaussian noise.  train.py --mode action_classifier
    --synthetic feeds it; the class is recoverable from the motion alone."""
    rs = np.random.RandomState(seed)
    cls = rs.randint(0, n_action, size=batch)
    start = rs.uniform(-0.5, 0.5, size=(batch, 1, n_points, 2))
    ang = 2.0 * np.pi * cls / float(n_action)
    direction = np.stack([np.cos(ang), np.sin(ang)], axis=-1).reshape(batch, 1, 1, 2)
    t = (np.arange(1, n_frames + 1) / float(n_frames)).reshape(1, n_frames, 1, 1)
    seq = start + drift * t * direction + noise * rs.randn(batch, n_frames, n_points, 2)
    return {'keypoints': start[:, 0].astype(np.float32), 'real_seq': seq.astype(np.float32),
            'action_code': np.eye(n_action, dtype=np.float32)[cls]}
