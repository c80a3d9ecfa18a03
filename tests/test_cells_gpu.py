"""GPU: kpx_cell_frames_u8_f32 (animate.py's grids) -- without markers bit for bit against the route it replaces (a staging stack and
kpx_sheet_paste_u8_f32) on every load / store path, with every byte outside the cell untouched; with markers bit for bit against the numpy
restatement (cells_ref.py) at exact rounding ties, at the edges of the cell and of the +-4 limit, for non-finite points, coincident points
and overlapping discs; graph replay; argument errors."""
import numpy as np
import pytest
import torch

import cells_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FILL = 0xA5


def _ops():
    from kpx_amd import ops
    return ops


def _values(shape, seed):
    """frame values: noise beyond both quantisers' ranges with NaN, the infinities and bucket edges mixed in"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.3, 1.3, size=shape).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, 1.0, 0.0, 127.0 / 255, 128.0 / 255 * 2 - 1, 3e38, -0.25], np.float32)
    flat[::max(1, flat.size // special.size)][:special.size] = special[:flat[::max(1, flat.size // special.size)].size]
    return x


def _dev_at(a, off):
    """a on the device, contiguous, its first element ``off`` elements past a 16-byte boundary"""
    t0 = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(a.size + 16, dtype=t0.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(t0.to(DEV))
    assert t.is_contiguous() and t.data_ptr() % 16 == (off * a.itemsize) % 16
    return t


def _canvas(b, frames, rows, cols, h, w, off=0):
    """-> (guard buffer, canvas view into it ``off`` bytes past a 16-byte boundary), all FILL"""
    n = b * frames * rows * h * cols * w * 3
    guard = torch.full((n + 48,), FILL, dtype=torch.uint8, device=DEV)
    return guard, guard[16 + off:16 + off + n].view(b, frames, rows * h, cols * w, 3)


def _check_outside(guard, got, off, row, col, h, w):
    g = guard.cpu().numpy()
    assert (g[:16 + off] == FILL).all() and (g[16 + off + got.size:] == FILL).all()
    outside = np.ones(got.shape, bool)
    outside[:, :, row * h:(row + 1) * h, col * w:(col + 1) * w] = False
    assert (got[outside] == FILL).all()


# ------------------------------------------------------------------------------------------------ r = 0 against stack + sheet_paste
PLAIN = [(1, 1, 1, 1, 3), (2, 3, 5, 7, 3), (2, 2, 16, 16, 1), (1, 2, 33, 17, 3), (1, 1, 4, 12, 3)]


@pytest.mark.parametrize('shape', PLAIN, ids=['x'.join(str(v) for v in s) for s in PLAIN])
def test_without_markers_the_cell_is_what_sheet_paste_gives(shape):
    ops = _ops()
    b, t, h, w, c = shape
    rows, cols = 2, 3
    first_np, seq_np = _values((b, h, w, c), 1), _values((b, t, h, w, c), 2)
    for premap in ('unit', 'raw'):
        for row, col in ((0, 0), (rows - 1, cols - 1)):
            for seq_off, canvas_off in ((0, 0), (1, 1)):
                first, seq = _dev_at(first_np, 0), _dev_at(seq_np, seq_off)
                stack = torch.empty((b, t + 1, h, w, c), dtype=torch.float32, device=DEV)       # the route of RolloutGifs._canvas
                stack[:, 0].copy_(first)
                stack[:, 1:].copy_(seq)
                want = torch.full((b * (t + 1), rows * h, cols * w, 3), FILL, dtype=torch.uint8, device=DEV)
                ops.sheet_paste(want, stack.view(b * (t + 1), 1, h, w, c), [0], row, col, premap)
                guard, canvas = _canvas(b, t + 1, rows, cols, h, w, canvas_off)
                assert ops.cell_frames(canvas, first, seq, row, col, premap) is canvas
                got = canvas.cpu().numpy()
                assert np.array_equal(got, want.view(canvas.shape).cpu().numpy()), (shape, premap, row, col, seq_off)
                _check_outside(guard, got, canvas_off, row, col, h, w)
                assert np.array_equal(got, R.cell_frames(np.full(got.shape, FILL, np.uint8), first_np, seq_np, row, col, premap))


# ------------------------------------------------------------------------------------------------ markers against cells_ref
def _point_pool():
    """(x, y) pairs: exact rint ties at W = 17 (x = (n + 0.5) / 128 - 1 lands on n + 0.5 sixteenths), the corners +-1, partly visible points
    at 1.2 and -1.3, the limit +-4 and its float32 neighbours beyond, NaN and the infinities, two coincident points, two overlapping discs,
    then noise"""
    tie = lambda n: np.float32((n + 0.5) / 128.0 - 1.0)
    f4 = np.float32(4.0)
    beyond, below = np.nextafter(f4, np.float32(5)), np.nextafter(-f4, np.float32(-5))
    tie_y = lambda n: np.float32((n + 0.5) / 64.0 - 1.0)                   # H = 9: n + 0.5 sixteenths down the rows
    fixed = [(tie(0), tie(1)), (tie(127), tie(64)), (tie(128), tie(255)), (tie(33), 0.0), (tie(34), 0.1), (tie(70), tie_y(40)), (tie(71), tie_y(41)),
             (-1.0, -1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (1.2, 0.0), (0.0, -1.3), (1.2, -1.3),
             (4.0, 0.0), (-4.0, 0.0), (0.0, 4.0), (0.0, -4.0), (4.0, 4.0), (-4.0, -4.0),
             (beyond, 0.0), (0.0, below), (below, beyond),
             (np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (np.nan, np.inf),
             (0.3, -0.2), (0.3, -0.2),                                      # coincident
             (-0.5, 0.5), (-0.4, 0.45)]                                     # overlapping
    rs = np.random.RandomState(3)
    noise = rs.uniform(-1.1, 1.1, size=(97 - len(fixed), 2))
    return np.concatenate([np.asarray(fixed, np.float64), noise]).astype(np.float32)


POOL = _point_pool()


def _points(shape, shift):
    n = int(np.prod(shape[:-1]))
    idx = (np.arange(n) * 7 + shift) % POOL.shape[0]                       # 7 and 97 are coprime: every entry is reached
    return POOL[idx].reshape(shape)


#          (B, T, H, W, C)     grid    cell   src off, canvas off
MARKED = [((2, 2, 9, 17, 3),   (2, 3), (1, 2), 0, 0),                      # scalar path; the ties
          ((2, 2, 9, 17, 1),   (1, 2), (0, 1), 0, 1),                      # grey, scalar, canvas one byte off
          ((2, 2, 16, 16, 3),  (2, 2), (1, 0), 0, 0),                      # 16 values per lane: items start inside a pixel
          ((1, 2, 8, 12, 3),   (2, 3), (0, 1), 0, 0),                      # 4 values per lane
          ((1, 2, 16, 16, 1),  (1, 1), (0, 0), 0, 0),                      # grey, 16 values per lane
          ((1, 1, 4, 16, 3),   (1, 2), (0, 1), 0, 4),                      # W % 16 == 0, canvas 4-byte aligned
          ((2, 1, 1, 1, 3),    (2, 2), (1, 1), 0, 0),                      # H = W = 1
          ((1, 1, 40, 300, 3), (1, 1), (0, 0), 0, 0)]                      # several workgroups per frame


@pytest.mark.parametrize('case', MARKED, ids=['x'.join(str(v) for v in c[0]) for c in MARKED])
def test_markers_are_bit_equal_to_the_restatement(case):
    ops = _ops()
    (b, t, h, w, c), (rows, cols), (row, col), src_off, canvas_off = case
    first_np, seq_np = _values((b, h, w, c), 4), _values((b, t, h, w, c), 5)
    first, seq = _dev_at(first_np, src_off), _dev_at(seq_np, src_off)
    drew = 0
    for n, (k, r) in enumerate((k, r) for k in (1, 3, 64) for r in (1, 2, 5, 16)):
        pf_np, ps_np = _points((b, k, 2), 11 * n), _points((b, t, k, 2), 11 * n + 5)
        colors_np = np.random.RandomState(n).randint(0, 256, size=(k, 3)).astype(np.uint8)
        colors_np[0] = (255, 0, 165)
        premap = ('unit', 'raw')[n % 2]
        guard, canvas = _canvas(b, t + 1, rows, cols, h, w, canvas_off)
        ops.cell_frames(canvas, first, seq, row, col, premap, _dev_at(pf_np, 0), _dev_at(ps_np, n % 2), _dev_at(colors_np, n % 3), r)
        got = canvas.cpu().numpy()
        want = R.cell_frames(np.full(got.shape, FILL, np.uint8), first_np, seq_np, row, col, premap, pf_np, ps_np, colors_np, r)
        assert np.array_equal(got, want), (case[0], k, r, int((got != want).sum()))
        _check_outside(guard, got, canvas_off, row, col, h, w)
        drew += int((want != R.cell_frames(np.full(got.shape, FILL, np.uint8), first_np, seq_np, row, col, premap)).sum())
    assert drew > 0                                                        # the markers are there to be compared


def test_the_marker_rules_on_hand_placed_points():
    """lowest k on top, clipping to the cell, nothing for NaN / beyond 4, through the kernel itself"""
    ops = _ops()
    h = w = 17
    zeros = np.zeros((1, h, w, 3), np.float32)
    first, seq = _dev_at(zeros, 0), _dev_at(zeros[:, None], 0)
    colors_np = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    base = 127                                                             # q_unit(0)

    def run(pts, r):
        pts = np.asarray(pts, np.float32)[None]
        _, canvas = _canvas(1, 2, 1, 2, h, w)
        ops.cell_frames(canvas, first, seq, 0, 0, 'unit', _dev_at(pts, 0), _dev_at(pts[:, None], 0), _dev_at(colors_np[:pts.shape[1]], 0), r)
        got = canvas.cpu().numpy()
        assert np.array_equal(got[0, 0], got[0, 1]) and (got[0, :, :, w:] == FILL).all()
        return got[0, 0, :, :w]

    one = run([(0.0, 0.0)], 3)                                             # centre pixel (8, 8): fill to distance 2, outline to 3
    assert tuple(one[8, 8]) == (10, 20, 30) and tuple(one[8, 10]) == (10, 20, 30) and tuple(one[8, 11]) == (0, 0, 0)
    assert tuple(one[8, 12]) == (base,) * 3 and tuple(one[10, 10]) == (0, 0, 0) and tuple(one[11, 11]) == (base,) * 3
    two = run([(0.0, 0.0), (0.0, 0.0), (0.25, 0.0)], 3)                    # coincident: k = 0 alone shows; k = 2 at (10, 8) is under k = 0's disc
    assert tuple(two[8, 8]) == (10, 20, 30) and tuple(two[8, 11]) == (0, 0, 0) and tuple(two[8, 12]) == (70, 80, 90)
    assert not (two == np.array([40, 50, 60], np.uint8)).all(axis=-1).any()
    edge = run([(1.25, 0.0)], 3)                                           # centre at column 18: the outline column 15.. is inside, fill from 16
    assert tuple(edge[8, 16]) == (10, 20, 30) and tuple(edge[8, 15]) == (0, 0, 0) and tuple(edge[8, 14]) == (base,) * 3
    for gone in ([(np.nan, 0.0)], [(0.0, np.inf)], [(np.nextafter(np.float32(4), np.float32(5)), 0.0)], [(0.0, -4.5)]):
        assert (run(gone, 16) == base).all()


def test_graph_replay_is_bitwise_the_eager_result():
    ops = _ops()
    b, t, h, w, k = 2, 3, 16, 16, 5
    first, seq = _dev_at(_values((b, h, w, 3), 6), 0), _dev_at(_values((b, t, h, w, 3), 7), 0)
    grey_first, grey_seq = _dev_at(_values((b, h, w, 1), 8), 0), _dev_at(_values((b, t, h, w, 1), 9), 0)
    pf, ps = _dev_at(_points((b, k, 2), 26), 0), _dev_at(_points((b, t, k, 2), 28), 0)
    colors = _dev_at(np.arange(3 * k, dtype=np.uint8).reshape(k, 3) * 9, 0)
    _, canvas = _canvas(b, t + 1, 1, 2, h, w)

    def enqueue():
        ops.cell_frames(canvas, first, seq, 0, 0, 'unit', pf, ps, colors, 3)
        ops.cell_frames(canvas, grey_first, grey_seq, 0, 1, 'raw')

    enqueue()
    torch.cuda.synchronize()
    eager = canvas.clone()
    assert not bool((eager == FILL).all())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    canvas.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(canvas, eager)                                      # (the two cells cover the canvas)


def test_bad_arguments_raise_kpx_error_and_launch_nothing():
    from kpx_amd import _lib
    from kpx_amd._lib import KpxError
    ops = _ops()
    b, t, h, w, k = 2, 3, 8, 8, 4
    first, seq = torch.zeros((b, h, w, 3), device=DEV), torch.zeros((b, t, h, w, 3), device=DEV)
    pf, ps = torch.zeros((b, k, 2), device=DEV), torch.zeros((b, t, k, 2), device=DEV)
    colors = torch.zeros((k, 3), dtype=torch.uint8, device=DEV)
    _, canvas = _canvas(b, t + 1, 2, 3, h, w)
    z8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    zf = lambda *s: torch.zeros(s, device=DEV)
    mark = lambda **kw: ops.cell_frames(canvas, first, seq, 0, 0, 'unit', **dict(dict(pts_first=pf, pts_seq=ps, colors=colors, radius=2), **kw))
    bad = [lambda: ops.cell_frames(canvas.float(), first, seq, 0, 0, 'unit'),                     # dtype
           lambda: ops.cell_frames(canvas, first.double(), seq, 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq.double(), 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas.cpu(), first, seq, 0, 0, 'unit'),                       # device
           lambda: ops.cell_frames(canvas, first.cpu(), seq, 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq.cpu(), 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq.transpose(2, 3), 0, 0, 'unit'),             # contiguity
           lambda: ops.cell_frames(canvas[0], first, seq, 0, 0, 'unit'),                          # dimensions
           lambda: ops.cell_frames(canvas, first[0], seq, 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq[:, 0], 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas[:1], first, seq, 0, 0, 'unit'),                         # batch sizes
           lambda: ops.cell_frames(canvas, first[:1], seq, 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas[:, :t], first, seq, 0, 0, 'unit'),                      # T + 1 frames
           lambda: ops.cell_frames(canvas, first, seq[:, :, :5].contiguous(), 0, 0, 'unit'),      # first is another size; 16 rows % 5
           lambda: ops.cell_frames(canvas, zf(b, 5, w, 3), zf(b, t, 5, w, 3), 0, 0, 'unit'),
           lambda: ops.cell_frames(canvas, zf(b, h, w, 2), zf(b, t, h, w, 2), 0, 0, 'unit'),      # C = 2
           lambda: ops.cell_frames(z8(1, 2, 65, 1, 3), zf(1, 1, 1, 3), zf(1, 1, 1, 1, 3), 0, 0, 'unit'),        # 65 rows of cells
           lambda: ops.cell_frames(z8(1, 2, 1, 65, 3), zf(1, 1, 1, 3), zf(1, 1, 1, 1, 3), 0, 0, 'unit'),        # 65 columns
           lambda: ops.cell_frames(z8(1, 2, 1, 1025, 3), zf(1, 1, 1025, 3), zf(1, 1, 1, 1025, 3), 0, 0, 'unit'),  # W = 1025
           lambda: ops.cell_frames(z8(1, 2, 1025, 1, 3), zf(1, 1025, 1, 3), zf(1, 1, 1025, 1, 3), 0, 0, 'unit'),  # H = 1025
           lambda: ops.cell_frames(canvas, first, seq, 2, 0, 'unit'),                             # the cell
           lambda: ops.cell_frames(canvas, first, seq, -1, 0, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq, 0, 3, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq, 0, -1, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq, 0.0, 0, 'unit'),
           lambda: ops.cell_frames(canvas, first, seq, 0, 0, 'png'),                              # premap
           lambda: ops.cell_frames(canvas, first, seq, 0, 0, 0),
           lambda: mark(radius=17),                                                               # radius
           lambda: mark(radius=-1),
           lambda: mark(radius=2.0),
           lambda: mark(radius=0),                                                                # points without markers
           lambda: mark(pts_first=None),                                                          # markers without points
           lambda: mark(pts_seq=None),
           lambda: mark(colors=None),
           lambda: mark(pts_first=pf.cpu()),
           lambda: mark(pts_seq=ps.double()),
           lambda: mark(colors=colors.float()),
           lambda: mark(colors=colors.cpu()),
           lambda: mark(colors=colors[:3]),                                                       # K differs
           lambda: mark(pts_seq=ps[:, :, :3].contiguous()),
           lambda: mark(pts_seq=ps[:, :2].contiguous()),                                          # T differs
           lambda: mark(pts_first=pf[:1]),
           lambda: mark(pts_first=zf(b, 65, 2), pts_seq=zf(b, t, 65, 2), colors=z8(65, 3)),       # K = 65
           lambda: mark(pts_first=zf(b, k, 3), pts_seq=zf(b, t, k, 3))]
    launched = _lib.abi_calls[0]
    for i, fn in enumerate(bad):
        with pytest.raises(KpxError):
            fn()
            pytest.fail('case %d raised nothing' % i)
    assert _lib.abi_calls[0] == launched                                   # no entry was called ...
    assert bool((canvas == FILL).all())                                    # ... and nothing was written
    mark(pts_first=zf(b, 64, 2), pts_seq=zf(b, t, 64, 2), colors=z8(64, 3), radius=16)            # the limits themselves are accepted
    assert _lib.abi_calls[0] == launched + 1 and not bool((canvas[:, :, :h, :w] == FILL).any())
