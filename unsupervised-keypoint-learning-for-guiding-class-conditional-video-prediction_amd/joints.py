"""Host side of the landmark regression (make_pseudo_labels.py --joints; not in the reference).

The usual quality measure of an unsupervised key-point detector: a linear map from the K discovered points of a frame to its J annotated
joints is fitted on the train split, and its error and PCK are reported on the test split.  ``read_labels`` reads Penn Action's label
files, ``crop_map`` takes an annotation to the coordinates the key points live in, ``solve`` fits the regressor from the normal equations
the device accumulated (csrc/joints.hip), ``summarise`` reduces the device's scores, ``JointRegression`` ties them together.  Everything but
``JointRegression`` is numpy float64 and runs the same with or without a GPU.

Conventions: a point is (x, y); a feature row is phi = (x_0, y_0, ..., x_{K-1}, y_{K-1}, 1), D = 2K + 1; the regressor of joint j is
W[j] [D, 2], pred = phi W[j]; coordinates are the key points' normalised ones ([-1, 1], pixel i of the res x res crop at -1 + 2 i / (res - 1)).
"""
import os

import numpy as np

from .stability import jsonable          # noqa: F401  (the same rule: a value that is not finite becomes null)

DEFAULT_ALPHAS = (0.05, 0.1, 0.2)
# The ridge keeps the normal equations solvable when key points are collinear over the train split (a detector that parks a point in a
# corner).  1e-6 of the number of frames per unit of squared coordinate is a judgement, not a measurement: it is far below the points' own
# variance (coordinates span [-1, 1]) and far above float64's rounding of G.
DEFAULT_RIDGE = 1e-6
MAX_ALPHAS = 8
LABEL_FIELDS = ('x', 'y', 'visibility', 'bbox', 'nframes')

NOTE = ("landmark regression as in the unsupervised key-point literature: a linear map from the discovered points to the annotated joints, "
        "fitted on the train split, error and PCK reported per split; the crop, the PCK normaliser and the joint set are this project's, so "
        "the figures are comparable across this project's checkpoints, and with published ones only under the same choices")


def read_labels(path, n_frames=None):
    """A Penn Action label file (``labels/NNNN.mat``, read through ``scipy.io.loadmat``) or an ``.npz`` with the same keys -> {'x', 'y'
    float64 [F,J], 'visibility' bool [F,J], 'bbox' float64 [F,4] = (x0, y0, x1, y1), 'nframes' int}.  Uses the fields x, y, visibility,
    bbox and nframes and ignores the others.  Raises ValueError when a field is missing, when the arrays disagree with each other or with
    the file's nframes, or when ``n_frames`` (the video's frame count) is given and differs."""
    if str(path).endswith('.npz'):
        with np.load(path) as z:
            raw = {k: z[k] for k in z.files}
    else:
        from scipy.io import loadmat
        raw = loadmat(path)
    missing = [k for k in LABEL_FIELDS if k not in raw]
    if missing:
        raise ValueError('%s: no field %s (a Penn Action label file has %s)' % (path, ', '.join(missing), ', '.join(LABEL_FIELDS)))
    nframes = np.asarray(raw['nframes']).reshape(-1)
    if nframes.size != 1:
        raise ValueError('%s: nframes must be one number (got shape %s)' % (path, np.asarray(raw['nframes']).shape))
    f = int(nframes[0])
    x, y = np.asarray(raw['x'], np.float64), np.asarray(raw['y'], np.float64)
    vis, bbox = np.asarray(raw['visibility']), np.asarray(raw['bbox'], np.float64)
    if x.ndim != 2 or x.shape[0] != f or y.shape != x.shape or vis.shape != x.shape or bbox.shape != (f, 4):
        raise ValueError('%s: with nframes = %d, x, y and visibility must be [%d, J] and bbox [%d, 4] (got x %s, y %s, visibility %s, bbox %s)'
                         % (path, f, f, f, x.shape, y.shape, vis.shape, bbox.shape))
    if n_frames is not None and int(n_frames) != f:
        raise ValueError('%s: annotates %d frames, the video has %d' % (path, f, int(n_frames)))
    return {'x': x, 'y': y, 'visibility': vis != 0, 'bbox': bbox, 'nframes': f}


def crop_map(w, h, res=128):
    """(ax, bx, ay, by), float64: pixel position (x, y) of the original w x h frame -> (ax x + bx, ay y + by), the normalised coordinate of
    the same image point after ``KeypointDataLoader.render_video``:
      the resize to [rw, rh] = [int(w / ratio), int(h / ratio)], ratio = min(w, h) / res, with PIL's pixel-centre convention, u = (x + 0.5)
        rw / w - 0.5 (the two axis scales rw / w and rh / h differ slightly, int() truncates the longer side);
      the crop ``center_crop_box(w, h)[0]``, whose edges PIL rounds half to even (``round``): u - left;
      pixel i of the crop -> -1 + 2 i / (res - 1).
    Annotation coordinates are taken as 0-BASED pixel positions as stored (integer x = the centre of pixel column x); Penn Action's files
    come from MATLAB, and if they are 1-based the map is off by one original pixel, under half a pixel of the crop."""
    from .data import center_crop_box
    w, h, res = int(w), int(h), int(res)
    if w < 1 or h < 1 or res < 2:
        raise ValueError('crop_map: needs w, h >= 1 and res >= 2 (got %r, %r, %r)' % (w, h, res))
    box, ratio = center_crop_box(w, h, res)
    rw, rh = int(w / ratio), int(h / ratio)
    left, top = int(round(box[0])), int(round(box[1]))
    sx, sy, g = rw / float(w), rh / float(h), 2.0 / (res - 1.0)
    return np.array([sx * g, (0.5 * sx - 0.5 - left) * g - 1.0, sy * g, (0.5 * sy - 0.5 - top) * g - 1.0], np.float64)


def solve(G, Bm, n, ridge=DEFAULT_RIDGE):
    """Per joint W[j] = (G[j] + ridge n[j] diag(1, ..., 1, 0))^-1 Bm[j] in float64: G [J,D,D], Bm [J,D,2], n [J] -> W [J,D,2].  The last
    feature is the constant 1 and its row, the bias, is not penalised; the penalty grows with n so that it stays the same share of G.
    ``ridge`` defaults to ``DEFAULT_RIDGE`` (a judgement, see there).  A joint with n[j] = 0, or whose system is singular (possible with
    ridge = 0), gets a NaN regressor, not an exception."""
    G, Bm, n = np.asarray(G, np.float64), np.asarray(Bm, np.float64), np.asarray(n)
    if G.ndim != 3 or G.shape[1] != G.shape[2] or Bm.shape != (G.shape[0], G.shape[1], 2) or n.shape != (G.shape[0],):
        raise ValueError('solve: needs G [J,D,D], Bm [J,D,2] and n [J] (got %s, %s, %s)' % (G.shape, Bm.shape, n.shape))
    if not ridge >= 0:
        raise ValueError('solve: ridge must be >= 0 (got %r)' % (ridge,))
    d = G.shape[1]
    pen = np.ones(d, np.float64)
    pen[-1] = 0.0
    W = np.full(Bm.shape, np.nan, np.float64)
    for j in range(G.shape[0]):
        if n[j] <= 0 or not (np.isfinite(G[j]).all() and np.isfinite(Bm[j]).all()):
            continue
        try:
            W[j] = np.linalg.solve(G[j] + np.diag(pen * (float(ridge) * float(n[j]))), Bm[j])
        except np.linalg.LinAlgError:
            pass
    return W


def video_record(subset, idx, n_frames, sum_err, count, pck_count, hit_count):
    """What ``summarise`` keeps of one video: ``ops.joint_scores``'s per-call outputs (sum_err [J], count [J], pck_count [J], hit_count
    [J,A]) and the number of its frames."""
    return {'subset': str(subset), 'idx': int(idx), 'frames': int(n_frames), 'sum_err': np.asarray(sum_err, np.float64),
            'count': np.asarray(count, np.int64), 'pck_count': np.asarray(pck_count, np.int64), 'hit_count': np.asarray(hit_count, np.int64)}


def _div(a, b):
    return float(a) / float(b) if b else float('nan')


def _summary(records, n_joints, alphas, res, solved):
    a = len(alphas)
    sum_err, count, pck_count = np.zeros(n_joints), np.zeros(n_joints, np.int64), np.zeros(n_joints, np.int64)
    hit = np.zeros((n_joints, a), np.int64)
    for r in records:
        sum_err, count, pck_count, hit = sum_err + r['sum_err'], count + r['count'], pck_count + r['pck_count'], hit + r['hit_count']
    entries = int(sum(r['frames'] for r in records)) * n_joints
    px = (res - 1) / 2.0
    per_err = [_div(sum_err[j], count[j]) if solved[j] else float('nan') for j in range(n_joints)]
    per_pck = [[_div(hit[j, i], pck_count[j]) if solved[j] else float('nan') for i in range(a)] for j in range(n_joints)]
    s = solved
    out = {'videos': len(records), 'frames': int(sum(r['frames'] for r in records)), 'entries': entries, 'valid_entries': int(count.sum()),
           'pck_entries': int(pck_count.sum()), 'valid_fraction': _div(count.sum(), entries), 'scored_joints': int(s.sum()),
           'scored_entries': int(count[s].sum()), 'scored_pck_entries': int(pck_count[s].sum()),
           'err': _div(sum_err[s].sum(), count[s].sum()), 'pck': [_div(hit[s, i].sum(), pck_count[s].sum()) for i in range(a)]}
    out['err_px'] = out['err'] * px
    out['per_joint'] = {'err': per_err, 'err_px': [e * px for e in per_err], 'pck': per_pck, 'count': count.tolist(),
                        'pck_count': pck_count.tolist()}
    return out


def summarise(records, n_joints, alphas, res, solved=None, protocol=None):
    """records: the ``video_record`` of every scored video, in the order they were added; alphas: the PCK thresholds; res: the crop's
    side; solved: bool [J], the joints that have a regressor (default all); protocol: the parameters of the run, copied into the result.
    -> {'note', 'res', 'alphas', 'protocol', 'overall', 'subsets': {name: ...}} with, overall and per subset: ``err`` the mean error over
    the valid entries (annotated visible inside the crop, finite key points) in normalised units and ``err_px`` the same times (res - 1) /
    2, pixels of the crop; ``pck`` per alpha the share of the valid entries with a finite normaliser whose error is within alpha times the
    normaliser; ``valid_fraction`` the share of (frame, joint) entries that are valid; the counts; and ``per_joint`` the same per joint.
    ``valid_entries``, ``pck_entries`` and ``valid_fraction`` describe the annotations and count every joint.  The overall ``err`` and ``pck``
    leave out the joints without a regressor, whose own figures are NaN: ``scored_joints`` says how many joints are in, and ``scored_entries``
    and ``scored_pck_entries`` are the denominators of ``err`` and ``pck`` (equal to ``valid_entries`` and ``pck_entries`` when every joint
    has a regressor).  NaN where nothing is valid."""
    alphas = [float(v) for v in alphas]
    solved = np.ones(n_joints, bool) if solved is None else np.asarray(solved, bool)
    subsets = []
    for r in records:
        if r['subset'] not in subsets:
            subsets.append(r['subset'])
    return {'note': NOTE, 'res': int(res), 'alphas': alphas, 'protocol': dict(protocol or {}),
            'overall': _summary(list(records), n_joints, alphas, res, solved),
            'subsets': {name: _summary([r for r in records if r['subset'] == name], n_joints, alphas, res, solved) for name in subsets}}


def per_video_arrays(records):
    """The per-video arrays of joints.npz: subset, idx, frames, err (the mean over the video's valid entries, NaN without any), count and
    pck_count (over the joints)."""
    return {'subset': np.array([r['subset'] for r in records], dtype='U16'), 'idx': np.array([r['idx'] for r in records], np.int64),
            'frames': np.array([r['frames'] for r in records], np.int64),
            'err': np.array([_div(r['sum_err'].sum(), r['count'].sum()) for r in records], np.float64),
            'count': np.array([r['count'].sum() for r in records], np.int64),
            'pck_count': np.array([r['pck_count'].sum() for r in records], np.int64)}


def check_alphas(alphas):
    """The PCK thresholds as a list of floats: 1 to ``MAX_ALPHAS`` numbers in (0, 1]; ValueError otherwise."""
    try:
        out = [float(v) for v in alphas]
    except (TypeError, ValueError):
        raise ValueError('PCK thresholds must be numbers (got %r)' % (alphas,))
    if not 1 <= len(out) <= MAX_ALPHAS or any(not 0.0 < v <= 1.0 for v in out):
        raise ValueError('needs 1 to %d PCK thresholds in (0, 1] (got %r)' % (MAX_ALPHAS, alphas))
    return out


class JointRegression(object):
    """The regression over a run of videos: ``add`` every video once, in any mix of subsets, then ``finish``.  The points, targets, masks
    and normalisers of every video stay on the device (a few MB for all of Penn Action), so the caller needs no second pass and every
    subset is scored by the one regressor fitted on 'train'.

    The moments are accumulated in the order the train videos are added: W is a function of that sequence, bit for bit, whatever videos of
    other subsets come in between.  Adding the train videos in another order may change the last bits of W; that is not guarded against."""

    def __init__(self, n_points, n_joints, alphas=DEFAULT_ALPHAS, norm='bbox', ridge=DEFAULT_RIDGE, device='cuda', res=128):
        import torch
        from . import ops
        if norm not in ('bbox', 'image'):
            raise ValueError("JointRegression: norm must be 'bbox' or 'image' (got %r)" % (norm,))
        if not ridge >= 0:
            raise ValueError('JointRegression: ridge must be >= 0 (got %r)' % (ridge,))
        if not (1 <= n_points <= ops.JOINT_MAX_POINTS and 1 <= n_joints <= ops.JOINT_MAX_JOINTS):
            raise ValueError('JointRegression: needs 1 <= n_points <= %d and 1 <= n_joints <= %d (got %r, %r)'
                             % (ops.JOINT_MAX_POINTS, ops.JOINT_MAX_JOINTS, n_points, n_joints))
        self.ops, self.torch = ops, torch
        self.k, self.j, self.alphas, self.norm, self.ridge, self.res = int(n_points), int(n_joints), check_alphas(alphas), norm, float(ridge), int(res)
        self.device = ops.normalize_device(device)
        d = 2 * self.k + 1
        self.G = torch.zeros((self.j, d, d), dtype=torch.float64, device=self.device)
        self.Bm = torch.zeros((self.j, d, 2), dtype=torch.float64, device=self.device)
        self.n = torch.zeros((self.j,), dtype=torch.int64, device=self.device)
        self.kept = []

    def add(self, subset, idx, pts, labels, frame_size):
        """One video: pts fp32 [F,K,2] on the device (``KeypointModel.run``'s ``outputs['pts'][0, :len]``; copied), labels a
        ``read_labels`` result for the same F frames, frame_size = (w, h) of the original frames.  One ``ops.joint_targets`` launch, and
        for the 'train' subset one ``ops.joint_moments_add`` launch."""
        torch, ops = self.torch, self.ops
        f = int(pts.shape[0])
        if tuple(pts.shape) != (f, self.k, 2):
            raise ValueError('JointRegression.add: pts must be [F, %d, 2] (got %s)' % (self.k, tuple(pts.shape)))
        if labels['x'].shape != (f, self.j):
            raise ValueError('JointRegression.add: video %s has %d frames of %d points, its labels are %s' % (idx, f, self.j, labels['x'].shape))
        pts = pts.detach().to(self.device, torch.float32).clone(memory_format=torch.contiguous_format)
        xy = torch.from_numpy(np.ascontiguousarray(np.stack([labels['x'], labels['y']], axis=-1), dtype=np.float32)).to(self.device)   # loadmat: Fortran order
        vis = torch.from_numpy(np.ascontiguousarray(labels['visibility']).astype(np.uint8)).to(self.device)
        bbox = torch.from_numpy(np.ascontiguousarray(labels['bbox']).astype(np.float32)).to(self.device)
        cmap = torch.from_numpy(crop_map(frame_size[0], frame_size[1], self.res)).to(self.device)
        target, mask, norm = ops.joint_targets(xy, vis, bbox, cmap)
        if self.norm == 'image':
            norm = torch.full_like(norm, 2.0)                         # the side of the crop in normalised units
        if subset == 'train':
            ops.joint_moments_add(pts, target, mask, self.G, self.Bm, self.n)
        self.kept.append({'subset': str(subset), 'idx': int(idx), 'pts': pts, 'target': target, 'mask': mask, 'norm': norm})

    def finish(self):
        """Solves once on the host and scores every kept video (one ``ops.joint_scores`` launch each) -> {'summary' (``summarise``), 'W',
        'G', 'Bm', 'n' (numpy), 'records', 'first': per video (target, mask, pred) of its first frame, numpy}."""
        torch, ops = self.torch, self.ops
        G, Bm, n = self.G.cpu().numpy(), self.Bm.cpu().numpy(), self.n.cpu().numpy()
        W = solve(G, Bm, n, self.ridge)
        solved = np.isfinite(W).all(axis=(1, 2))
        w_dev = torch.from_numpy(W).to(self.device)
        alpha = torch.tensor(self.alphas, dtype=torch.float64, device=self.device)
        records, first = [], []
        for v in self.kept:
            pred, _, _, sum_err, count, pck_count, hit_count = ops.joint_scores(v['pts'], v['target'], v['mask'], v['norm'], w_dev, alpha)
            records.append(video_record(v['subset'], v['idx'], v['pts'].shape[0], sum_err.cpu().numpy(), count.cpu().numpy(),
                                        pck_count.cpu().numpy(), hit_count.cpu().numpy()))
            first.append((v['target'][0].cpu().numpy(), v['mask'][0].cpu().numpy(), pred[0].cpu().numpy()))
        protocol = {'n_points': self.k, 'n_joints': self.j, 'norm': self.norm, 'ridge': self.ridge, 'train_frames_per_joint': n.tolist()}
        return {'summary': summarise(records, self.j, self.alphas, self.res, solved, protocol), 'W': W, 'G': G, 'Bm': Bm, 'n': n,
                'records': records, 'first': first}


def find_label_file(labels_dir, idx):
    """The label file of video ``idx`` under labels_dir (NNNN.mat, else NNNN.npz), or None."""
    for ext in ('.mat', '.npz'):
        p = os.path.join(labels_dir, '%04d%s' % (int(idx), ext))
        if os.path.exists(p):
            return p
    return None


def planted_labels(seed, n_frames, n_joints, frame_size):
    """Planted annotations for the script's --synthetic mode, from ``np.random.RandomState(seed)``: joints uniform over the frame, nine in
    ten visible, a box around them.  They have nothing to do with the frames: they exercise the path, the scores mean nothing."""
    rs = np.random.RandomState(seed)
    w, h = frame_size
    x, y = rs.uniform(0, w - 1, size=(n_frames, n_joints)), rs.uniform(0, h - 1, size=(n_frames, n_joints))
    bbox = np.stack([x.min(1), y.min(1), x.max(1) + 1.0, y.max(1) + 1.0], axis=1)
    return {'x': x, 'y': y, 'visibility': rs.uniform(size=(n_frames, n_joints)) < 0.9, 'bbox': bbox, 'nframes': int(n_frames)}
