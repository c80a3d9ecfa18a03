"""The nearest training motion of a key-point sequence (csrc/novelty.hip, include/kpx.h ABI 25): evaluate.py --novelty.

Does the motion generator invent motions or replay training sequences?  Every rollout is searched in the set of sequences the stage-2 loader
can draw without augmentation (``WindowIndex``: per listing line every legal start frame at the video's own gap), optionally also mirrored,
per action class; the same search of the held-out real futures is the baseline.  The labels stay where ``resident.ResidentLabels`` keeps them,
in one flat HBM buffer; the search (``seq_nearest``) reads the windows straight from it, and ``MotionStore.gather`` returns a found window
through the existing gather, ``ResidentLabels.augment``.  Distances are this project's own key-point-space quantity.
"""
import numpy as np

from . import resident as R

# mirrors of include/kpx.h (tests/test_novelty_cpu.py holds them equal to the header)
NEAREST_ROW_INTS, NEAREST_GROUP, NEAREST_MAX_QUERIES, NEAREST_MAX_WINDOWS = 4, 64, 4096, (1 << 30) - 1
N_VIDEO, N_IM_IDX, N_GAP, N_ACTION = range(4)


def _error(msg):
    from ._lib import KpxError
    return KpxError(msg)


def last_start(n_files):
    """The largest start frame ``SequenceDataLoader.plan`` can draw for a video of n_files frame files (negative: it can draw none)."""
    gap = int(n_files / R.SEQ_LEN)
    return n_files - R.SEQ_LEN * gap if gap >= 1 else n_files - R.SEQ_SHORT


class WindowIndex(object):
    """The candidate windows: exactly the un-augmented sequences ``SequenceDataLoader.plan()`` can draw from ``listing``.  Line by line in
    listing order (a video listed twice contributes twice, each time under that line's action), every start 0 .. last_start ascending, at the
    video's own gap = int(n_files / 33).  ``table`` int32 [W, 4] = (video, im_idx, gap, action); the window id is the row number; ``line``
    int32 [W] the listing line of each window.  Host only."""

    def __init__(self, label_index, listing):
        self.index = label_index
        rows, lines = [], []
        for li, text in enumerate(listing):
            name, action = text.split()[0], int(text.split()[1])
            v, n = label_index.video(name), label_index.count(name)
            gap = int(n / R.SEQ_LEN)
            starts = np.arange(last_start(n) + 1, dtype=np.int64)
            rows.append(np.stack([np.full_like(starts, v), starts, np.full_like(starts, gap), np.full_like(starts, action)], 1))
            lines.append(np.full(len(starts), li, np.int64))
        table = np.concatenate(rows) if rows else np.zeros((0, NEAREST_ROW_INTS), np.int64)
        if table.shape[0] > NEAREST_MAX_WINDOWS:
            raise _error('%d candidate windows, the search takes %d' % (table.shape[0], NEAREST_MAX_WINDOWS))
        self.table = np.ascontiguousarray(table.astype(np.int32))
        self.line = (np.concatenate(lines) if lines else np.zeros(0, np.int64)).astype(np.int32)

    def __len__(self):
        return int(self.table.shape[0])

    def check(self, n_action, table=None):
        """Raises ``KpxError`` for a table the kernel cannot take (as ``SequencePlanner.check_rows``); it trusts the table and clamps nothing."""
        t = np.asarray(self.table if table is None else table)
        if t.dtype != np.int32 or t.ndim != 2 or t.shape[1] != NEAREST_ROW_INTS or not 0 < t.shape[0] <= NEAREST_MAX_WINDOWS:
            raise _error('windows: int32 [1..%d, %d] expected, got %s %s' % (NEAREST_MAX_WINDOWS, NEAREST_ROW_INTS, t.dtype, t.shape))
        idx = self.index
        if len(idx.label_rows) and int(idx.label_rows.max()) * idx.n_points * 2 >= 1 << 31:
            raise _error("windows: a video's label array holds 2^31 or more values, the search addresses one with 32 bits")
        video = t[:, N_VIDEO].astype(np.int64)
        if (video < 0).any() or (video >= len(idx.names)).any():
            raise _error('windows: video number outside the store (0..%d)' % (len(idx.names) - 1))
        im_idx, gap = t[:, N_IM_IDX].astype(np.int64), t[:, N_GAP].astype(np.int64)
        last = np.where(gap >= 1, im_idx + (R.SEQ_LEN - 1) * gap, im_idx + R.SEQ_SHORT - 1)
        if (im_idx < 0).any() or (gap < 0).any() or (last >= idx.label_rows[video]).any():
            raise _error("windows: a window leaves its video's label rows")
        if (t[:, N_ACTION] < 0).any() or (t[:, N_ACTION] >= n_action).any():
            raise _error('windows: action index outside 0..%d' % (n_action - 1))
        return t

    def plan(self, n_action):
        """-> (order int32 [G * NEAREST_GROUP], group_first int32 [n_action + 1]): the window ids grouped by class, ascending inside a class,
        every class starting a new block of NEAREST_GROUP and its last block closed with -1; class a owns the blocks group_first[a] ..
        group_first[a + 1] - 1.  One workgroup of the search takes one block, so one class; the codes keep referring to ``table``."""
        action = self.table[:, N_ACTION]
        order, first = [], [0]
        for a in range(n_action):
            ids = np.flatnonzero(action == a).astype(np.int32)
            blocks = (len(ids) + NEAREST_GROUP - 1) // NEAREST_GROUP
            order.append(np.concatenate([ids, np.full(blocks * NEAREST_GROUP - len(ids), -1, np.int32)]))
            first.append(first[-1] + blocks)
        return np.concatenate(order).astype(np.int32), np.array(first, np.int32)

    def describe(self, codes):
        """codes int [...] -> int32 [..., 4] = (listing line, im_idx, gap, mirrored); -1 everywhere for the code -1 (nothing was found)."""
        codes = np.asarray(codes, np.int64)
        found = codes >= 0
        w = np.where(found, codes >> 1, 0)
        out = np.stack([self.line[w], self.table[w, N_IM_IDX], self.table[w, N_GAP], (codes & 1).astype(np.int32)], -1).astype(np.int32)
        out[~found] = -1
        return out


def seq_nearest(labels, label_off, windows, order, group_first, queries, exclude=None, mirror=True, out=None):
    """kpx_seq_nearest_f32 (include/kpx.h): per query and action class the squared RMS point distance to the nearest candidate window and
    its code.  labels fp32 [*], label_off int64 [V]: the resident label store; windows int32 [W, 4], order int32 [G * 64], group_first
    int32 [A + 1]: ``WindowIndex.table`` and ``WindowIndex.plan`` ON THE DEVICE, validated by the caller with ``WindowIndex.check`` (the
    kernel trusts them); queries contiguous fp32 [Q, 32, K, 2], 1 <= Q <= 4096; exclude int32 [Q] or None -> (d2 fp64 [Q, A], code int32
    [Q, A]), code = 2 * window + mirrored, -1 and +inf for a class without a finite candidate.  ``out``: (d2, code) tensors to write into.
    Two launches on the current stream, no atomics; every value's bits depend on the query's and the window's data alone."""
    import torch
    from ._args import OPTIONAL, _ptr, _stream, check_out, check_tensors, scratch
    from ._lib import lib, check, KpxError
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    dev = check_tensors('seq_nearest', [('queries', queries, f32, (None, R.SEQ_LEN - 1, None, 2), 8)])
    q, _, k, _ = queries.shape
    check_tensors('seq_nearest', [('labels', labels, f32, None, 8), ('label_off', label_off, i64, (None,)), ('windows', windows, i32, (None, NEAREST_ROW_INTS)),
                                  ('order', order, i32, (None,)), ('group_first', group_first, i32, (None,)),
                                  ('exclude', exclude, i32, (q,), *OPTIONAL)], dev)
    w, a, groups = windows.shape[0], group_first.shape[0] - 1, order.shape[0] // NEAREST_GROUP
    if not 1 <= q <= NEAREST_MAX_QUERIES or not 1 <= k <= R.SEQ_MAX_POINTS:
        raise KpxError('seq_nearest: needs 1 <= Q <= %d queries of 1 <= K <= %d points (got %s)' % (NEAREST_MAX_QUERIES, R.SEQ_MAX_POINTS, tuple(queries.shape)))
    if not 1 <= w <= NEAREST_MAX_WINDOWS or not 1 <= a <= R.SEQ_MAX_ACTIONS:
        raise KpxError('seq_nearest: needs 1 <= W <= %d windows and 1 <= A <= %d classes (got W = %d, A = %d)' % (NEAREST_MAX_WINDOWS, R.SEQ_MAX_ACTIONS, w, a))
    if groups < 1 or groups * NEAREST_GROUP != order.shape[0] or groups > (w + NEAREST_GROUP - 1) // NEAREST_GROUP + a:
        raise KpxError('seq_nearest: order must hold the %d windows in whole blocks of %d, one run per class (got %d entries)'
                       % (w, NEAREST_GROUP, order.shape[0]))
    d2, code = out if out is not None else (None, None)
    d2 = check_out('seq_nearest', 'out d2', d2, f64, (q, a), dev)
    code = check_out('seq_nearest', 'out code', code, i32, (q, a), dev)
    nbytes = lib.kpx_seq_nearest_workspace_bytes(groups, q)
    work = scratch.get('seq_nearest', nbytes, dev)
    check(lib.kpx_seq_nearest_f32(labels.data_ptr(), label_off.data_ptr(), windows.data_ptr(), w, order.data_ptr(), group_first.data_ptr(), groups,
                                  queries.data_ptr(), _ptr(exclude), q, k, a, 1 if mirror else 0, work.data_ptr(), nbytes, d2.data_ptr(),
                                  code.data_ptr(), _stream()), 'kpx_seq_nearest_f32')
    return d2, code


class MotionStore(object):
    """The training motions on the device: a ``ResidentLabels`` store (its buffers are the search's), the window table and its class-grouped
    order.  ``index``: a ``LabelIndex`` built from arrays takes the place of the files under ``data_dir``."""

    def __init__(self, data_dir, listing, n_points, n_action, device, index=None):
        import torch
        self.labels = R.ResidentLabels(data_dir, listing, n_points, n_action, device, index=index)
        self.device, self.n_points, self.n_action = self.labels.device, self.labels.index.n_points, self.labels.n_action
        self.windows = WindowIndex(self.labels.index, listing)
        if not len(self.windows):
            raise _error('the listing holds no video of %d or more frames: there is no window to search' % R.SEQ_SHORT)
        self.windows.check(self.n_action)
        order, first = self.windows.plan(self.n_action)
        self.table = torch.from_numpy(self.windows.table).to(self.device)
        self.order = torch.from_numpy(order).to(self.device)
        self.group_first = torch.from_numpy(first).to(self.device)

    def video(self, name):
        """The store's number of a video, -1 when it holds none of that name: what ``exclude_video`` takes."""
        return self.labels.index._video.get(name, -1)

    def nearest(self, queries, mirror=True, exclude_video=None):
        """queries fp32 [Q, 32, K, 2] on the device; exclude_video int32 [Q] on the device (-1: none) or None -> (d2 fp64 [Q, A], code int32
        [Q, A]).  More than 4096 queries go in several calls; a query's result does not depend on its place."""
        import torch
        queries = queries.contiguous()
        if queries.dim() != 4 or queries.shape[2] != self.n_points:
            raise _error('nearest: queries [Q, %d, %d, 2] expected, got %s' % (R.SEQ_LEN - 1, self.n_points, tuple(queries.shape)))
        q = queries.shape[0]
        with torch.cuda.device(self.device):
            d2 = torch.empty((q, self.n_action), dtype=torch.float64, device=self.device)
            code = torch.empty((q, self.n_action), dtype=torch.int32, device=self.device)
            for lo in range(0, q, NEAREST_MAX_QUERIES):
                hi = min(q, lo + NEAREST_MAX_QUERIES)
                seq_nearest(self.labels.labels, self.labels.label_off, self.table, self.order, self.group_first, queries[lo:hi],
                            None if exclude_video is None else exclude_video[lo:hi].contiguous(), mirror, out=(d2[lo:hi], code[lo:hi]))
        return d2, code

    def gather(self, codes):
        """codes: ints in [0, 2 W) -> fp32 [n, 32, K, 2] on the device: the windows as the search reads them, a mirrored code's x negated
        (``ResidentLabels.augment`` with the row flag SEQ_FLIP; no other flag)."""
        import torch
        codes = np.asarray(codes.cpu() if hasattr(codes, 'cpu') else codes, np.int64).reshape(-1)
        if codes.size and (codes.min() < 0 or codes.max() >= 2 * len(self.windows)):
            raise _error('gather: codes lie in [0, %d) (got values from %d to %d)' % (2 * len(self.windows), codes.min(), codes.max()))
        t = self.windows.table[codes >> 1]
        lo, hi = np.array([1.0], np.float64).view(np.int32)
        rows = np.zeros((codes.size, R.SEQ_ROW_INTS), np.int32)
        rows[:, R.S_VIDEO], rows[:, R.S_IM_IDX], rows[:, R.S_GAP], rows[:, R.S_ACTION] = t[:, N_VIDEO], t[:, N_IM_IDX], t[:, N_GAP], t[:, N_ACTION]
        rows[:, R.S_FLAGS] = np.where(codes & 1, R.SEQ_FLIP, 0)
        rows[:, R.S_SCALE_LO], rows[:, R.S_SCALE_HI] = lo, hi
        parts = [self.labels.augment_rows(rows[i:i + R.SEQ_MAX_ROWS])['real_seq'] for i in range(0, codes.size, R.SEQ_MAX_ROWS)]
        if not parts:
            return torch.empty((0, R.SEQ_LEN - 1, self.n_points, 2), dtype=torch.float32, device=self.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)
