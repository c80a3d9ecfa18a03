"""Helpers of the resident key-point label tests (tests/test_resident_seq_cpu.py, tests/test_resident_seq_gpu.py): a tiny Penn-shaped
dataset with pseudo labels, hand-made ``SeqPlan``s that cover every decision, the collated ``SequenceDataLoader.render`` outputs, and a
numpy restatement of csrc/augment_seq.hip with explicit float32 / float64 casts and one rounding per operation -- the specification the
kernel is written from.  (Helper module, no tests.)"""
import os
import random

import numpy as np
from PIL import Image

K, N_ACTION = 5, 9
FRAMES = (100, 70, 40, 33, 32, 17)           # gap 3, 2, 1, 1 and two short videos; the last one allows im_idx 0 only
f32, f64 = np.float32, np.float64


def bits(a):
    """The bit patterns of a float32 array or tensor: -0.0 and +0.0 differ here."""
    if hasattr(a, 'cpu'):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def video_name(v):
    return 'frames/%04d' % (v + 1)


def write_dataset(root, frames=FRAMES, k=K, n_action=N_ACTION, w=160, h=96, seed=0):
    """frames/NNNN/000001.jpg.. (w x h), pseudo_labels/NNNN.npy float32 [len, k, 2] in [-1, 1] with some exact +0.0 / -0.0 entries,
    train_set.txt = test_set.txt = one line per video (the first video listed a second time).  -> {video: label array}"""
    rs = np.random.RandomState(seed)
    root = str(root)
    os.makedirs(os.path.join(root, 'pseudo_labels'))
    labels, lines = {}, []
    for v, n in enumerate(frames):
        name = video_name(v)
        os.makedirs(os.path.join(root, name))
        base = rs.randint(0, 256, size=(h // 8, w // 8, 3)).astype(np.uint8)
        for i in range(n):
            im = Image.fromarray(np.roll(base, i, axis=1)).resize((w, h), Image.BILINEAR)
            im.save(os.path.join(root, name, '%06d.jpg' % (i + 1)), format='JPEG', quality=85)
        a = (rs.rand(n, k, 2) * 2.0 - 1.0).astype(np.float32)
        for _ in range(6):                   # exact zeros of both signs, at the start, at the end and in between
            a[rs.randint(n), rs.randint(k), rs.randint(2)] = 0.0
            a[rs.randint(n), rs.randint(k), rs.randint(2)] = -0.0
        a[0, 0], a[n - 1, k - 1] = (0.0, -0.0), (-0.0, 0.0)
        np.save(os.path.join(root, 'pseudo_labels', '%04d.npy' % (v + 1)), a)
        labels[name] = a
        lines.append('%s %d' % (name, (3 * v + 1) % n_action))
    lines.append('%s %d' % (video_name(0), n_action - 1))
    for subset in ('train', 'test'):
        with open(os.path.join(root, subset + '_set.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return labels


def loader(root, random_order, randomness, seed=0, k=K, n_action=N_ACTION, subset='train'):
    from kpx_amd.data import SequenceDataLoader
    return SequenceDataLoader(str(root), subset, k, n_action, random_order=random_order, randomness=randomness, rng=random.Random(seed),
                              np_rng=np.random.RandomState(seed))


def last_im_idx(n):
    """The largest start frame ``plan()`` can draw for a video of n frame files."""
    gap = int(n / 33)
    return n - 33 * gap if gap >= 1 else n - 17


def hand_plans(randomness, frames=FRAMES):
    """SeqPlans over every listing line, alternating between the first and the last legal im_idx of the video.  With ``randomness``: every
    angle -15..15 on every line; one video with gap >= 1 and one short video take each angle with both flips x scales 0.70 / 1.00 / 1.20,
    the other lines cycle through those six.  Without it the random fields are None, as ``plan()`` leaves them."""
    from kpx_amd.data import SeqPlan
    lines = list(range(len(frames))) + [0]                      # the listing's last line is video 0 again
    plans = []
    for index, v in enumerate(lines):
        n = frames[v]
        starts = sorted({0, last_im_idx(n)})
        if not randomness:
            plans += [SeqPlan(index, video_name(v), n, s, None, None, None) for s in starts]
            continue
        combos = [(flip, scale) for flip in (0, 1) for scale in (70 / 100.0, 100 / 100.0, 120 / 100.0)]
        full = index in (1, 4)               # one video of each form meets the whole cross product, the others every angle once
        j = 0
        for angle in range(-15, 16):
            for flip, scale in (combos if full else [combos[(angle + index) % 6]]):
                plans.append(SeqPlan(index, video_name(v), n, starts[j % len(starts)], angle, flip, scale))
                j += 1
    return plans


def collated(ld, plans):
    """What ``batches`` delivers for these plans, on the host: ``render`` then ``_collate``'s stack + astype(float32)."""
    samples = [ld.render(p) for p in plans]
    return {key: np.stack([s[key] for s in samples]).astype(np.float32) for key in ('keypoints', 'real_seq', 'action_code')}


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in numpy
def _transform(x, y, flags, c, s, scale, T):
    """seq_transform of csrc/augment_seq.hip in type T: every constant is cast to T first, every product and sum is one T operation."""
    from kpx_amd import resident as R
    if flags & R.SEQ_ROTATE:
        ct, st = T(c), T(s)
        qx = (T(0) + ct * x) - st * y
        qy = (T(0) + st * x) + ct * y
        x, y = qx, qy
    if flags & R.SEQ_FLIP:
        x = x * T(-1)
    if flags & R.SEQ_SCALE:
        x, y = x * T(scale), y * T(scale)
    return x, y


def restate_row(labels, row, trig, n_action):
    """One table row on one video's label array float32 [len, K, 2] -> (keypoints [K,2], real_seq [32,K,2], action_code [A]) float32."""
    from kpx_amd import resident as R
    assert labels.dtype == np.float32
    im_idx, gap, flags = int(row[R.S_IM_IDX]), int(row[R.S_GAP]), int(row[R.S_FLAGS])
    c, s = trig[row[R.S_ANGLE]]
    scale = np.array([row[R.S_SCALE_LO], row[R.S_SCALE_HI]], np.int32).view(np.float64)[0]
    if gap >= 1:
        g = labels[[im_idx + gap * t for t in range(R.SEQ_LEN)]]
        x, y = _transform(g[..., 0], g[..., 1], flags, c, s, scale, f32)
        assert x.dtype == np.float32 and y.dtype == np.float32
    else:
        g = np.empty((R.SEQ_LEN,) + labels.shape[1:], np.float32)
        for t in range(R.SEQ_LEN):
            p = labels[im_idx + t // 2]
            g[t] = (p + labels[im_idx + t // 2 + 1]) * f32(0.5) if t & 1 else p          # float32 add, float32 halving
        x, y = _transform(g[..., 0].astype(f64), g[..., 1].astype(f64), flags, c, s, scale, f64)
        assert x.dtype == np.float64 and y.dtype == np.float64
        x, y = x.astype(f32), y.astype(f32)
    seq = np.stack([x, y], -1)
    code = np.zeros(n_action, np.float32)
    code[row[R.S_ACTION]] = 1
    return seq[0], seq[1:], code


def restate(planner, rows):
    """-> the collated batch of ``rows`` as the kernel computes it (numpy, host)."""
    from kpx_amd import resident as R
    trig = R.seq_trig()
    outs = [restate_row(planner.index.array(planner.index.names[r[R.S_VIDEO]]), r, trig, planner.n_action) for r in rows]
    return {key: np.stack([o[i] for o in outs]) for i, key in enumerate(('keypoints', 'real_seq', 'action_code'))}
