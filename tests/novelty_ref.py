"""Helpers of the novelty tests (tests/test_novelty_cpu.py, tests/test_novelty_gpu.py): a float64 numpy restatement of the nearest-motion
search of csrc/novelty.hip -- the window enumeration written independently of ``kpx_amd.novelty.WindowIndex``, the window frames through
``resident_seq_ref.restate_row`` with no flag, d2 by ``np.sum`` in float64, the minimum and the tie rules by an explicit loop -- and the
small stores the tests search.  (Helper module, no tests.)"""
import numpy as np

import resident_seq_ref as S

REL_D2 = 1e-12         # 32 K 2 float64 additions at K <= 40: at most 2560 * 2^-53 = 2.8e-13 relative, whatever the order
REL_MARGIN = 1e-11     # the argmin is compared where the restatement's runner-up of the class is further than this


def enumerate_windows(listing, counts, numbers):
    """listing: lines 'video action'; counts: {video: frame files}; numbers: {video: the store's video number} -> (table int32 [W, 4] =
    (video, im_idx, gap, action), line int32 [W]): every sequence SequenceDataLoader.plan() can draw, line by line."""
    table, line = [], []
    for li, text in enumerate(listing):
        name, action = text.split()
        n = counts[name]
        gap = n // 33
        last = n - 33 * gap if gap >= 1 else n - 17
        for start in range(0, last + 1):
            table.append((numbers[name], start, gap, int(action)))
            line.append(li)
    return np.array(table, np.int32).reshape(-1, 4), np.array(line, np.int32)


def window_frames(arrays, table):
    """arrays: per video number its label array float32 [len, K, 2] -> float32 [W, 32, K, 2]: real_seq of every window, no flag set."""
    from kpx_amd import resident as R
    trig = R.seq_trig()
    lo, hi = np.array([1.0], np.float64).view(np.int32)
    out = []
    for video, im_idx, gap, action in table:
        row = np.array([video, im_idx, gap, 0, 0, lo, hi, action], np.int32)
        out.append(S.restate_row(arrays[video], row, trig, int(action) + 1)[1])
    return np.stack(out)


def distances(query, frames, mirror):
    """query float32 [32, K, 2], frames float32 [W, 32, K, 2] -> float64 [W, 2 or 1]: d2 of the plain and the mirrored candidate."""
    q, v = query.astype(np.float64), frames.astype(np.float64)
    n = q.shape[0] * q.shape[1]
    with np.errstate(invalid='ignore', over='ignore'):
        ey2 = (q[None, ..., 1] - v[..., 1]) ** 2
        cols = [np.sum((q[None, ..., 0] - v[..., 0]) ** 2 + ey2, axis=(1, 2)) / n]
        if mirror:
            cols.append(np.sum((q[None, ..., 0] + v[..., 0]) ** 2 + ey2, axis=(1, 2)) / n)
    return np.stack(cols, 1)


def nearest(queries, frames, table, n_action, mirror=True, exclude=None):
    """-> (d2 float64 [Q, A], code int32 [Q, A], runner float64 [Q, A]): per class the lowest finite d2, the lowest code that reaches it
    (code = 2 w + m), and the lowest d2 of any OTHER candidate of the class (+inf without one); +inf and -1 for a class without a finite
    candidate.  exclude: per query a video number whose windows are skipped (-1: none)."""
    nq = queries.shape[0]
    d2 = np.full((nq, n_action), np.inf)
    code = np.full((nq, n_action), -1, np.int32)
    runner = np.full((nq, n_action), np.inf)
    for qi in range(nq):
        d = distances(queries[qi], frames, mirror)
        for w in range(frames.shape[0]):
            if exclude is not None and table[w, 0] == exclude[qi]:
                continue
            a = table[w, 3]
            for m in range(d.shape[1]):
                v, c = d[w, m], 2 * w + m
                if not np.isfinite(v):
                    continue
                if v < d2[qi, a] or (v == d2[qi, a] and c < code[qi, a]):
                    if code[qi, a] >= 0:
                        runner[qi, a] = min(runner[qi, a], d2[qi, a])
                    d2[qi, a], code[qi, a] = v, c
                else:
                    runner[qi, a] = min(runner[qi, a], v)
    return d2, code, runner


def clear_margin(d2, runner):
    """bool [Q, A]: the runner-up of the class is more than REL_MARGIN (relative) above the minimum, or there is none"""
    with np.errstate(invalid='ignore'):
        return ~np.isfinite(runner) | (runner - d2 > REL_MARGIN * runner)


def assert_matches(got_d2, got_code, want_d2, want_code, runner, planted=None):
    """The kernel's (d2, code) against the restatement's: d2 within REL_D2 where finite and equal where not, the code equal wherever the
    margin is clear -- which must be everywhere but at the ``planted`` [Q, A] pairs, whose code must be equal all the same."""
    got_d2, got_code = np.asarray(got_d2), np.asarray(got_code)
    assert got_d2.dtype == np.float64 and got_code.dtype == np.int32 and got_d2.shape == want_d2.shape == got_code.shape
    fin = np.isfinite(want_d2)
    assert (np.isfinite(got_d2) == fin).all() and (got_d2[~fin] == np.inf).all() and (got_code[~fin] == -1).all()
    err = np.abs(got_d2[fin] - want_d2[fin])
    assert (err <= REL_D2 * want_d2[fin]).all(), (err / np.maximum(want_d2[fin], 1e-300)).max()
    clear = clear_margin(want_d2, runner)
    if planted is not None:
        clear = clear | planted
    assert clear.all(), 'the inputs leave a query-class pair inside the margin: choose another seed'
    assert (got_code == want_code).all()


def array_store(seed, n_videos=70, k=40, n_action=9, lengths=(17, 32, 33, 65, 66, 200)):
    """A store from arrays alone: ``lengths`` and seeded lengths in 17..200 up to n_videos, labels in [-1, 1], every line its own action.
    -> (names, counts, arrays, listing)"""
    rs = np.random.RandomState(seed)
    counts = list(lengths) + [int(v) for v in rs.randint(17, 201, size=n_videos - len(lengths))]
    names = ['frames/%04d' % (v + 1) for v in range(n_videos)]
    arrays = [(rs.rand(n, k, 2) * 2.0 - 1.0).astype(np.float32) for n in counts]
    listing = ['%s %d' % (name, rs.randint(n_action)) for name in names]
    return names, counts, arrays, listing
