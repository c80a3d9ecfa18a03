"""Float64 restatement and planted inputs for the per-variable gradient statistics (csrc/grad_stats.hip: kpx_grad_segment_stats_f32);
shared by test_clip_cpu.py and test_clip_gpu.py.  Imports nothing from the package under test.

A bucket is ``entries``: name -> (offset, shape), and ``size``; a variable is the elements [offset, offset + numel).  Per variable: the count
of non-finite gradient values and the largest finite magnitude are exact in any order; the sums of squares are fixed-order float64 sums of
exact non-negative terms, within guard_ref.sumsq_bound(numel, .) of the exact sum.
"""
from collections import OrderedDict

import numpy as np

F32 = np.float32
CHUNK = 16384
SEG_LENGTHS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)
N_ONES = 300                                           # then a run of one-element variables: more variables than a wavefront has lanes
SHIFTS = (0, 1, 2, 3)                                  # floats the whole table is moved by: only shift 0 starts every variable 16-byte aligned


class FlatBucket:
    """entries / size as variables.Bucket lays them out (every variable padded to a multiple of 4 floats), moved by ``shift`` floats."""

    def __init__(self, lengths, shift=0):
        self.entries, at = OrderedDict(), shift
        for i, n in enumerate(lengths):
            self.entries['v%03d_%d' % (i, n)] = (at, (n,))
            at += (n + 3) // 4 * 4
        self.size = at


def synthetic_bucket(shift=0):
    return FlatBucket(SEG_LENGTHS + (1,) * N_ONES, shift)


def chunk_table(bucket):
    """[(start, len, seg)]: every variable cut into chunks of at most CHUNK elements counted from its own start."""
    out = []
    for seg, (offset, shape) in enumerate(bucket.entries.values()):
        n = int(np.prod(shape))
        out += [(offset + at, min(CHUNK, n - at), seg) for at in range(0, n, CHUNK)]
    return out


def values(bucket, seed, wide=True):
    """One fp32 vector per variable (the same for every shift of the same lengths): magnitudes over twelve decades."""
    rs = np.random.RandomState(7000 + seed)
    out = []
    for offset, shape in bucket.entries.values():
        n = int(np.prod(shape))
        mag = 10.0 ** rs.uniform(-6.0, 6.0, size=n) if wide else np.ones(n)
        out.append((rs.choice([-1.0, 1.0], size=n) * mag * rs.uniform(1.0, 2.0, size=n)).astype(F32))
    return out


def plant_positions(n):
    """Indices inside a variable of n elements that receive a non-finite value: the first and the last element and both sides of every
    chunk boundary inside it."""
    pos = {0, n - 1}
    for edge in range(CHUNK, n, CHUNK):
        pos |= {edge - 1, edge}
    return sorted(pos)


def planted(vals, which, value):
    """A copy of ``vals`` with ``value`` planted into the variables ``which`` at plant_positions."""
    out = [v.copy() for v in vals]
    for s in which:
        out[s][plant_positions(out[s].size)] = F32(value)
    return out


def flat(bucket, vals, gap=np.nan, tail=4):
    """The flat buffer: every variable's values at its offset, ``gap`` everywhere else (the padding, the shift and ``tail`` floats behind)."""
    buf = np.full(bucket.size + tail, gap, dtype=F32)
    for (offset, shape), v in zip(bucket.entries.values(), vals):
        buf[offset:offset + v.size] = v
    return buf


def segment_stats(bucket, g, p=None, dtype=np.float64):
    """-> dict of per-variable arrays sumsq_g, sumsq_p (``dtype``), maxabs_g (fp32), nonfinite_g, numel, read from the flat buffers."""
    rows = []
    for offset, shape in bucket.entries.values():
        n = int(np.prod(shape))
        x = np.asarray(g[offset:offset + n], dtype=F32)
        ok = np.isfinite(x)
        fin = x[ok].astype(dtype)
        sp = dtype(0)
        if p is not None:
            y = np.asarray(p[offset:offset + n], dtype=F32)
            y = y[np.isfinite(y)].astype(dtype)
            sp = (y * y).sum(dtype=dtype)
        rows.append(((fin * fin).sum(dtype=dtype) if fin.size else dtype(0), sp, F32(np.abs(x[ok]).max()) if fin.size else F32(0),
                     int(n - ok.sum()), n))
    cols = list(zip(*rows))
    return dict(sumsq_g=np.array(cols[0], dtype=dtype), sumsq_p=np.array(cols[1], dtype=dtype), maxabs_g=np.array(cols[2], dtype=F32),
                nonfinite_g=np.array(cols[3], dtype=np.int64), numel=np.array(cols[4], dtype=np.int64))
