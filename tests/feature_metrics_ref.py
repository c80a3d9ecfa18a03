"""float64 restatement of the VGG feature-space metrics (evaluate.py --vgg-metrics), numpy only:

    per layer and spatial position over the C channels  saa = sum a^2, sbb = sum b^2, dot = sum a b
    c = 1 where saa == 0 and sbb == 0;  c = 0 where exactly one of them is 0;  else c = min(1, dot / sqrt(saa sbb))
    cos_layer = mean of c over positions;  l1_layer = mean |a - b| over positions and channels
    vgg_cos / vgg_l1 = the means of cos_layer / l1_layer over the five layers Vgg19.build returns

The VGG19 forward of the 8-bit frames (q = metrics_ref.png8(x) on the 0..255 scale, BGR, minus VGG_MEAN) goes through
oracle.restatement.vgg19 in float64.  The CPU tests check the closed forms, the GPU tests hold the kernel, the scorer and evaluate.py to it."""
import numpy as np

from metrics_ref import png8

LAYERS = ['conv1_2', 'conv2_2', 'conv3_4', 'conv4_4', 'conv5_4']


def layer_metrics(fa, fb):
    """-> float64 [N,2] = (cos_layer, l1_layer) of fa[n] against fb[n], both [N,H,W,C]."""
    a = np.asarray(fa, dtype=np.float64)
    b = np.asarray(fb, dtype=np.float64)
    assert a.ndim == 4 and a.shape == b.shape
    saa, sbb, dot = (a * a).sum(axis=-1), (b * b).sum(axis=-1), (a * b).sum(axis=-1)
    za, zb = saa == 0, sbb == 0
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.minimum(1.0, dot / np.sqrt(saa * sbb))
    c = np.where(za & zb, 1.0, np.where(za | zb, 0.0, c))
    return np.stack([c.mean(axis=(1, 2)), np.abs(a - b).mean(axis=(1, 2, 3))], axis=1)


def vgg_features(weights, frames, quantise=True):
    """The five float64 feature arrays of ``frames`` [N,H,W,3]: values in [-1,1] quantised as evaluate.py writes them (``quantise``), or
    8-bit values as they are; ``weights`` = {'conv1_1': (HWIO filter, bias), ...} (oracle.restatement.synthetic_vgg)."""
    import torch
    from oracle import restatement as R
    q = png8(frames).astype(np.float64) if quantise else np.asarray(frames, dtype=np.float64)
    w64 = {k: (torch.from_numpy(np.asarray(w, np.float64)), torch.from_numpy(np.asarray(b, np.float64))) for k, (w, b) in weights.items()}
    with torch.no_grad():
        return [f.contiguous().numpy() for f in R.vgg19(w64, torch.from_numpy(q))]


def frame_scores(feats_a, feats_b):
    """-> float64 [N,5,2]: per frame and layer (cos_layer, l1_layer); vgg_cos = [..., 0].mean(-1), vgg_l1 = [..., 1].mean(-1)."""
    return np.stack([layer_metrics(a, b) for a, b in zip(feats_a, feats_b)], axis=1)


def vgg_frame_metrics(weights, a, b, quantise=True):
    """Frames a against b through the float64 VGG19 -> (scores [N,5,2], features of a, features of b)."""
    n = len(a)
    feats = vgg_features(weights, np.concatenate([a, b], axis=0), quantise)
    fa, fb = [f[:n] for f in feats], [f[n:] for f in feats]
    return frame_scores(fa, fb), fa, fb


def fragile(feats):
    """Per layer, the smallest non-zero position norm over the layer's mean position norm: how close the features come to the cosine's
    zero rule, where rounding in the network could move a position across it (1 when every position is zero)."""
    out = []
    for f in feats:
        norm = np.sqrt((np.asarray(f, np.float64) ** 2).sum(axis=-1))
        nz = norm[norm > 0]
        out.append(float(nz.min() / norm.mean()) if nz.size else 1.0)
    return out
