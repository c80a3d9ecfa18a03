"""HBM-resident training frames and the image-pair augmentation on the GPU (csrc/augment.hip, include/kpx.h ABI 9).

``ImagePairDataLoader.batches(..., resident=True)`` decodes every frame of the subset ONCE, keeps the decoded uint8 frames in one flat
device buffer and produces each batch with two HIP launches that do what ``ImagePairDataLoader.render`` does with PIL -- byte for byte.
Per step the host draws the ``PairPlan``s exactly as the CPU pipeline does (same code, same generators) and ships one small integer
table; no JPEG is decoded, no PIL call is made and no pixels cross PCIe.
The tile side S is the loader's ``image_size`` (default 128): the tables, the rows' validation and the two launches are built for it.

Everything of Pillow's arithmetic that involves double precision is done HERE, in Python floats, and reaches the kernels as integers:

* ``resize_table``      Pillow's antialiased BICUBIC (a = -0.5) coefficients of one pass, normalised in double and rounded to 22 bits
                        (Resample.c: precompute_coeffs + normalize_coeffs_8bpc);
* ``rotate_constants``  ``Image.rotate``'s matrix (``round(cos, 15)`` ...) in the 16.16 fixed point of Geometry.c: affine_fixed;
* ``filter_kernels``    the six ``ImageFilter`` kernels divided by their scale in double, rounded to float32 once.

tests/test_resident_cpu.py applies these tables in numpy and compares with PIL itself; tests/test_resident_gpu.py compares the kernels'
output with ``render``.  There is no fallback: ``resident=True`` on a CPU device raises ``KpxError``.

The second half of the file is stage 2's counterpart (csrc/augment_seq.hip, ABI 12): ``SequenceDataLoader.batches(..., resident=True)`` keeps
the pseudo labels of every listed video in HBM and produces the key-point batches of ``SequenceDataLoader.render`` with one launch each.
"""
import math
import os
import os.path as osp
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

from .data import IMAGE_SIZE, _KERNEL_FILTERS, _DeviceBatcher, _resized_size, _to_device_unit, check_image_size

# mirrors of include/kpx.h (tests/test_resident_cpu.py holds them equal to the header)
ROW_INTS, FLIP, ROTATE, IDENTITY = 24, 1, 2, 4
BAND, BANDS, KERNEL_FLOATS = 16, 8, 32
MAX_SIDE, MAX_TAPS, MAX_BAND_ROWS, MAX_ROWS = 2048, 32, 160, 32768
TILE_MIN, TILE_MAX, LDS_BYTES = 32, 256, 122880      # the *_sq_* entries: tile sides, and the LDS one workgroup of the geometry kernel may ask for
(R_FRAME, R_W, R_H, R_X0, R_Y0, R_FLAGS, R_FILT, R_FVAL, R_A0, R_A1, R_A2, R_A3, R_A4, R_A5,
 R_HTAB, R_HSTRIDE, R_VTAB, R_VSTRIDE, R_RW, R_RH) = range(20)
ALIGN = 16                         # every frame starts at a multiple of 16 bytes
DEFAULT_MAX_BYTES = 64 << 30


def _error(msg):
    from ._lib import KpxError
    return KpxError(msg)


# ------------------------------------------------------------------------------------------------ Pillow's arithmetic, host side
def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_table(n_in, n_out):
    """One pass of ``Image.resize`` (BICUBIC, antialiased) from n_in to n_out samples -> (xmin int32 [n_out], count int32 [n_out],
    k int32 [n_out, taps]): output i = clip((2^21 + sum_j k[i, j] * in[xmin[i] + j]) >> 22, 0, 255).  Pillow skips a pass whose lengths
    are equal; its table here is the identity {i, 1, 2^22}, which that formula maps to in[i] exactly."""
    if n_in == n_out:
        return (np.arange(n_out, dtype=np.int32), np.ones(n_out, np.int32), np.full((n_out, 1), 1 << 22, np.int32))
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    rows = []
    for i in range(n_out):
        c = (i + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - xmin
        w = [_bicubic((j + xmin - c + 0.5) * (1.0 / fs)) for j in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        w = [v / ww for v in w]
        rows.append((xmin, [int(v * (1 << 22) - 0.5) if v < 0 else int(v * (1 << 22) + 0.5) for v in w]))
    taps = max(len(k) for _, k in rows)
    if taps > MAX_TAPS:
        raise _error('resize %d -> %d needs %d taps per output sample, the kernels take %d' % (n_in, n_out, taps, MAX_TAPS))
    xmin = np.array([r[0] for r in rows], np.int32)
    cnt = np.array([len(r[1]) for r in rows], np.int32)
    k = np.zeros((n_out, taps), np.int32)
    for i, (_, kk) in enumerate(rows):
        k[i, :len(kk)] = kk
    if 255 * int(np.abs(k.astype(np.int64)).sum(1).max()) >= 1 << 31:
        raise _error('resize %d -> %d: the 32-bit sums of a pass could overflow' % (n_in, n_out))
    return xmin, cnt, k


def band_rows(xmin, cnt):
    """The most input rows any BAND consecutive outputs of a pass read: what one workgroup of the geometry kernel keeps in LDS."""
    top = (xmin + cnt).astype(np.int64)
    n = len(xmin)
    if n < BAND:
        return int(top.max() - xmin.min())
    return max(int(top[i:i + BAND].max() - xmin[i]) for i in range(n - BAND + 1))


def rotate_constants(w, h, angle):
    """``Image.rotate(angle)`` (NEAREST, same size, about the centre) as Pillow's 16.16 fixed-point coefficients a0..a5:
    output (x, y) reads source ((a2 + a1*y + a0*x) >> 16, (a5 + a4*y + a3*x) >> 16).  None for a multiple of 360 (the identity)."""
    if angle % 360 == 0:
        return None
    t = -math.radians(angle % 360.0)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + cx
    m[5] = m[3] * -cx + m[4] * -cy + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def filter_kernels():
    """float32 [6, KERNEL_FLOATS]: per ImageFilter kernel of data._KERNEL_FILTERS its size, float32(offset) + 0.5, then the
    size x size coefficients float32(k / scale) (the division in double), rows top to bottom."""
    out = np.zeros((len(_KERNEL_FILTERS), KERNEL_FLOATS), np.float32)
    for i, f in enumerate(_KERNEL_FILTERS):
        (kw, kh), scale, offset, k = f.filterargs
        assert kw == kh and kw in (3, 5) and len(k) == kw * kh
        out[i, 0] = kw
        out[i, 1] = np.float32(offset) + np.float32(0.5)
        out[i, 2:2 + kw * kh] = (np.array(k, np.float64) / scale).astype(np.float32)
    return out


def centre_origin(rw, image_size=IMAGE_SIZE):
    """Left edge of ``render``'s centre crop box (ox - S/2, 0, ox + S/2, S): PIL rounds the corners with Python's round (ties to even)."""
    return int(round(rw / 2.0 - image_size // 2))


# ------------------------------------------------------------------------------------------------ the store's bookkeeping (no device)
def store_layout(videos):
    """videos: [(w, h, n_frames)] -> (per frame byte offset int64, per video first frame number int64, total bytes).  Frames lie one
    after the other in listing order, each HWC uint8 and starting at a multiple of ALIGN bytes."""
    offsets, first, pos, k = [], [], 0, 0
    for w, h, n in videos:
        step = (w * h * 3 + ALIGN - 1) // ALIGN * ALIGN
        first.append(k)
        offsets.extend(pos + i * step for i in range(n))
        pos += n * step
        k += n
    return np.array(offsets, np.int64), np.array(first, np.int64), pos


class FrameIndex(object):
    """Which frames a store holds and where: per video its size, first frame number and frame count; per frame its byte offset.
    Host only.  ``plan()`` takes frame sizes and counts from here instead of ``Image.open`` / ``os.listdir`` (the same values)."""

    def __init__(self, names, sizes, counts, max_bytes=DEFAULT_MAX_BYTES):
        self.names = list(names)
        self.width = np.array([s[0] for s in sizes], np.int64)
        self.height = np.array([s[1] for s in sizes], np.int64)
        self.n_frames = np.array(counts, np.int64)
        self._video = {name: i for i, name in enumerate(self.names)}
        for name, w, h in zip(self.names, self.width, self.height):
            if max(w, h) > MAX_SIDE or min(w, h) < 1:
                raise _error('%s: frames of %d x %d, the augmentation kernels take sides up to %d' % (name, w, h, MAX_SIDE))
        self.offsets, self.first, self.total_bytes = store_layout(zip(self.width.tolist(), self.height.tolist(), self.n_frames.tolist()))
        if self.total_bytes > max_bytes:
            raise _error('the decoded frames need %d bytes (%.2f GiB) of HBM, max_bytes allows %d: the resident path keeps the whole '
                         'subset on the device' % (self.total_bytes, self.total_bytes / float(1 << 30), max_bytes))

    @classmethod
    def scan(cls, data_dir, listing, max_bytes=DEFAULT_MAX_BYTES, threads=16):
        """From the files: every frame's header is opened (as ``render`` opens it); a frame that is not RGB, or whose size differs
        from its video's first frame, raises with the file name."""
        names = []
        for line in listing:
            v = line.split()[0]
            if v not in names:
                names.append(v)
        counts = [len(os.listdir(osp.join(data_dir, v))) for v in names]

        def header(path):
            with Image.open(path) as im:
                return im.mode, im.size
        sizes = []
        with ThreadPoolExecutor(max_workers=max(1, min(16, threads))) as pool:
            for v, n in zip(names, counts):
                paths = [frame_path(data_dir, v, i) for i in range(n)]
                heads = list(pool.map(header, paths))
                for p, (mode, size) in zip(paths, heads):
                    if mode != 'RGB':
                        raise _error('%s: mode %s, the image-pair pipeline takes RGB frames only' % (p, mode))
                    if size != heads[0][1]:
                        raise _error('%s: %d x %d, but its video starts with %d x %d frames' % ((p,) + tuple(size) + tuple(heads[0][1])))
                sizes.append(heads[0][1])
        return cls(names, sizes, counts, max_bytes)

    def video(self, name):
        return self._video[name]

    def count(self, name):
        return int(self.n_frames[self._video[name]])

    def size(self, name):
        v = self._video[name]
        return int(self.width[v]), int(self.height[v])

    def frame_number(self, name, idx):
        v = self._video[name]
        if not 0 <= idx < self.n_frames[v]:
            raise _error('%s has no frame %d' % (name, idx))
        return int(self.first[v]) + idx


def frame_path(data_dir, video, idx):
    return osp.join(data_dir, video, '{:06d}'.format(idx + 1) + '.jpg')


class ResizeTables(object):
    """The int32 buffer the geometry kernel reads its coefficients from: one table per distinct (n_in, n_out), entries of
    ``stride`` = 2 + taps ints {first input, tap count, coefficients}."""

    def __init__(self):
        self._parts, self._size, self.entries = [], 0, {}

    def add(self, n_in, n_out):
        """-> (offset, stride, rows of the input any BAND outputs read)"""
        key = (n_in, n_out)
        if key not in self.entries:
            xmin, cnt, k = resize_table(n_in, n_out)
            part = np.concatenate([xmin[:, None], cnt[:, None], k], axis=1).astype(np.int32)
            self.entries[key] = (self._size, part.shape[1], band_rows(xmin, cnt))
            self._parts.append(part.reshape(-1))
            self._size += part.size
        return self.entries[key]

    def buffer(self):
        return np.concatenate(self._parts) if self._parts else np.zeros(0, np.int32)


class AugmentPlanner(object):
    """Table rows (include/kpx.h: kpx_augment_geometry_sq_u8) from ``PairPlan``s or by hand, and their validation, for tiles of
    ``image_size`` x ``image_size``.  Host only.  ``lds_bytes``: what one workgroup of the geometry kernel may keep in LDS; a video whose
    band needs more is held in the store but refused by ``check_rows`` when a row asks for it."""

    def __init__(self, index, image_size=IMAGE_SIZE, lds_bytes=LDS_BYTES):
        self.index = index
        self.image_size = s = check_image_size(image_size, 'image_size')
        self.bands = s // BAND
        self.lds_bytes = int(lds_bytes)
        self.tables = ResizeTables()
        self._per_video = []
        self._rot = {}
        self.band_need = []                          # per video: rows of the horizontally resized frame one band reads
        for v in range(len(index.names)):
            w, h = int(index.width[v]), int(index.height[v])
            rw, rh, _ = _resized_size(w, h, s)
            if rw < s or rh < s:
                raise _error('%s: %d x %d resizes to %d x %d, smaller than the %d x %d crop' % (index.names[v], w, h, rw, rh, s, s))
            ho, hs, _ = self.tables.add(w, rw)
            vo, vs, need = self.tables.add(h, rh)
            if need > MAX_BAND_ROWS:
                raise _error('%s: a %d-row band of the %d -> %d resize reads %d rows, the kernels take %d' % (index.names[v], BAND, h, rh, need, MAX_BAND_ROWS))
            self.band_need.append(need)
            self._per_video.append((w, h, rw, rh, ho, hs, vo, vs))
        self.band_need = np.array(self.band_need, np.int64).reshape(-1)
        fits = self.band_need[self.band_need * s * 3 <= self.lds_bytes]
        self.band_rows_cap = max([BAND] + fits.tolist())         # the launches' LDS: the largest need among the videos check_rows admits
        self._tab_by_offset = {off: (key, stride) for key, (off, stride, _) in self.tables.entries.items()}

    def row(self, video, idx, angle=None, x0=0, y0=0, flip=0, filt=-1, filt_val=None):
        """One table row: frame ``idx`` (0-based) of ``video``, rotated by ``angle`` degrees (None / 0: not at all), resized, cropped at
        (x0, y0) of the resized frame, flipped, filtered (-1: no filter; 6..9 take ``filt_val``, the enhancer's factor times ten)."""
        w, h, rw, rh, ho, hs, vo, vs = self._per_video[self.index.video(video)]
        flags = FLIP if flip else 0
        a = None
        if angle:
            a = self._rot.get((w, h, angle))
            if a is None:
                a = self._rot[(w, h, angle)] = rotate_constants(w, h, angle)
        if a is not None:
            flags |= ROTATE
        fbits = 0
        if filt is not None and filt >= 6:
            f = filt_val * 0.1                                   # ImageEnhance.X(im).enhance(filt_val * 0.1)
            if f == 1.0:
                flags |= IDENTITY
            fbits = int(np.float32(f).view(np.int32))
        return [self.index.frame_number(video, idx), w, h, x0, y0, flags, -1 if filt is None else filt, fbits] + list(a or (65536, 0, 0, 0, 65536, 0)) + \
               [ho, hs, vo, vs, rw, rh, 0, 0, 0, 0]

    def rows_for_plans(self, plans, randomness):
        """int32 [2 * len(plans), ROW_INTS]: the rows of every plan's ``image``, then of every plan's ``future_image``."""
        first, second = [], []
        for p in plans:
            w, h, rw, rh = self._per_video[self.index.video(p.video)][:4]
            if randomness:
                x0, y0 = (p.crop, 0) if w > h else (0, p.crop)
                kw = dict(angle=p.angle, x0=x0, y0=y0, flip=p.flip, filt=p.filt, filt_val=p.filt_val)
            else:
                kw = dict(x0=centre_origin(rw, self.image_size))         # render's else branch: centred on the width, the top S rows
            first.append(self.row(p.video, p.im_idx, **kw))
            second.append(self.row(p.video, p.fu_idx, **kw))
        return np.array(first + second, np.int64).astype(np.int32).reshape(-1, ROW_INTS)

    def check_rows(self, rows):
        """Raises ``KpxError`` for a row the kernels cannot take; they trust the table and clamp nothing."""
        rows = np.asarray(rows)
        if rows.dtype != np.int32 or rows.ndim != 2 or rows.shape[1] != ROW_INTS or not 0 < rows.shape[0] <= MAX_ROWS:
            raise _error('augmentation rows: int32 [1..%d, %d] expected, got %s %s' % (MAX_ROWS, ROW_INTS, rows.dtype, rows.shape))
        idx = self.index
        frame = rows[:, R_FRAME].astype(np.int64)
        if (frame < 0).any() or (frame >= len(idx.offsets)).any():
            raise _error('augmentation rows: frame number outside the store (0..%d)' % (len(idx.offsets) - 1))
        video = np.searchsorted(idx.first, frame, side='right') - 1
        if (rows[:, R_W] != idx.width[video]).any() or (rows[:, R_H] != idx.height[video]).any():
            raise _error("augmentation rows: frame size differs from the store's")
        over = self.band_need[video] * self.image_size * 3 > self.lds_bytes
        if over.any():
            v = int(video[np.argmax(over)])
            raise _error('augmentation rows: %s: a %d-row band of its %d x %d tile reads %d rows of the resized frame = %d bytes of LDS, a '
                         'workgroup has %d' % (idx.names[v], BAND, self.image_size, self.image_size, self.band_need[v],
                                               self.band_need[v] * self.image_size * 3, self.lds_bytes))
        if (rows[:, R_FILT] < -1).any() or (rows[:, R_FILT] > 9).any():
            raise _error('augmentation rows: filter id outside -1..9')
        if (rows[:, R_FLAGS] & ~(FLIP | ROTATE | IDENTITY)).any():
            raise _error('augmentation rows: unknown flag')
        lin, off = rows[:, [R_A0, R_A1, R_A3, R_A4]].astype(np.int64), rows[:, [R_A2, R_A5]].astype(np.int64)
        if (np.abs(lin) > 65536).any() or (np.abs(off) >= 1 << 29).any():
            raise _error('augmentation rows: rotation coefficients outside the 32-bit bounds')
        for tab, stride, n_in, n_out, origin in ((R_HTAB, R_HSTRIDE, R_W, R_RW, R_X0), (R_VTAB, R_VSTRIDE, R_H, R_RH, R_Y0)):
            for o in np.unique(rows[:, tab]):
                known = self._tab_by_offset.get(int(o))
                sel = rows[:, tab] == o
                if known is None or (rows[sel, stride] != known[1]).any() or (rows[sel, n_in] != known[0][0]).any() or (rows[sel, n_out] != known[0][1]).any():
                    raise _error('augmentation rows: resize table does not belong to the frame size')
            if (rows[:, origin] < 0).any() or (rows[:, origin] + self.image_size > rows[:, n_out]).any():
                raise _error('augmentation rows: crop window outside the resized frame')
        return rows


# ------------------------------------------------------------------------------------------------ the store on the device
class ResidentFrames(AugmentPlanner):
    """Every frame of the listed videos, decoded once, in ONE flat uint8 device buffer (HWC, frame after frame, 16-byte aligned), with
    the frame offsets and the per-video table beside it on the host (``index``) and on the device, plus the coefficient tables of the
    augmentation kernels.  Each data-parallel rank builds its own."""
    STAGE_BYTES = 64 << 20

    def __init__(self, data_dir, listing, device, max_bytes=DEFAULT_MAX_BYTES, threads=16, image_size=IMAGE_SIZE):
        import time
        import torch
        device = torch.device(device)
        if device.type != 'cuda':
            raise _error('resident frames live in HBM: device %s is not a GPU (the package has no CPU fallback)' % device)
        t0 = time.perf_counter()
        index = FrameIndex.scan(data_dir, listing, max_bytes, threads)        # raises before anything is allocated
        super(ResidentFrames, self).__init__(index, image_size)
        self.data_dir, self.device = data_dir, device
        with torch.cuda.device(device):
            self.frames = torch.empty(max(index.total_bytes, ALIGN), dtype=torch.uint8, device=device)
            self.frame_off = torch.from_numpy(index.offsets).to(device)
            self.video_table = torch.from_numpy(np.stack([index.width, index.height, index.first, index.n_frames], 1)).to(device)
            self.resize_tabs = torch.from_numpy(self.tables.buffer()).to(device)
            self.kernels = torch.from_numpy(filter_kernels()).to(device)
            self._ingest(min(16, max(1, threads)))
        self.ingest_seconds = time.perf_counter() - t0

    def _decode_into(self, buf, base, k):
        idx = self.index
        v = int(np.searchsorted(idx.first, k, side='right')) - 1
        path = frame_path(self.data_dir, idx.names[v], k - int(idx.first[v]))
        with Image.open(path) as im:
            if im.mode != 'RGB' or im.size != (idx.width[v], idx.height[v]):
                raise _error('%s: %s %s, expected RGB %d x %d' % (path, im.mode, im.size, idx.width[v], idx.height[v]))
            a = np.asarray(im)
        o = int(idx.offsets[k]) - base
        buf[o:o + a.size] = a.reshape(-1)

    def _ingest(self, threads):
        """Decode on a thread pool into two pinned staging buffers; the copy of one overlaps the decoding of the other."""
        import torch
        idx = self.index
        n = len(idx.offsets)
        ends = np.append(idx.offsets[1:], idx.total_bytes)          # a frame's slot ends where the next begins
        stage = [torch.zeros(self.STAGE_BYTES, dtype=torch.uint8).pin_memory() for _ in range(2)]
        done = [None, None]
        i = chunk = 0
        with ThreadPoolExecutor(max_workers=threads) as pool:
            while i < n:
                lo = int(idx.offsets[i])
                j = max(i + 1, int(np.searchsorted(ends, lo + self.STAGE_BYTES, side='right')))     # MAX_SIDE^2 * 3 < STAGE_BYTES: j > i
                hi = int(ends[j - 1])
                slot = chunk % 2
                if done[slot] is not None:
                    done[slot].synchronize()
                buf = stage[slot].numpy()
                list(pool.map(lambda k: self._decode_into(buf, lo, k), range(i, j)))
                self.frames[lo:hi].copy_(stage[slot][:hi - lo], non_blocking=True)
                done[slot] = torch.cuda.Event()
                done[slot].record()
                i, chunk = j, chunk + 1
        torch.cuda.current_stream().synchronize()

    def augment(self, rows_dev, n_rows, out=None):
        """The two launches on the current stream: rows_dev = DEVICE int32 [>= n_rows, ROW_INTS] (validated by the caller with
        ``check_rows``) -> float32 [n_rows, S, S, 3] in [-1, 1], S = image_size."""
        import torch
        from . import ops
        with torch.cuda.device(self.device):
            tiles, lsum = ops.augment_geometry(self.frames, self.frame_off, rows_dev, n_rows, self.resize_tabs, self.band_rows_cap, self.image_size)
            return ops.augment_filter(tiles, lsum, rows_dev, n_rows, self.kernels, self.image_size, out=out)

    def augment_rows(self, rows):
        """Host rows (``row`` / ``rows_for_plans``) -> the augmented frames: validation, upload, the two launches."""
        import torch
        rows = self.check_rows(np.ascontiguousarray(rows))
        rows_dev = torch.from_numpy(rows).to(self.device)
        return self.augment(rows_dev, rows.shape[0])


class ResidentBatcher(object):
    """``batches(..., resident=True)``: the iterator contract of ``_DeviceBatcher`` ({'image', 'future_image'} float32 [B,S,S,3] on
    the device; repeat / shuffle; a short last batch) on a ``ResidentFrames`` store.  The plans come from the SAME ``_plan_stream``, so
    both iterators consume ``rng`` / ``np_rng`` identically.  Per batch one pinned int32 table goes to the device asynchronously and the
    two augmentation launches are enqueued on the consumer's stream; the host never waits for the device."""
    SHUFFLE_BUFFER = _DeviceBatcher.SHUFFLE_BUFFER
    SLOTS = 4
    _plan_stream = _DeviceBatcher._plan_stream

    def __init__(self, loader, batch_size, device, repeat, shuffle, max_bytes):
        import torch
        self._torch = torch
        self.loader, self.batch_size, self.repeat, self.shuffle = loader, batch_size, repeat, shuffle
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _error('resident=True needs a GPU device, got %s (the package has no CPU fallback)' % self.device)
        self.store = loader.resident_frames(self.device, max_bytes)
        self.host = [torch.empty((2 * batch_size, ROW_INTS), dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)]
        self.copied = [None] * self.SLOTS          # per pinned slot: event after its last H2D copy
        self._slot = 0
        self._plans = self._plan_stream()

    def __iter__(self):
        return self

    def __next__(self):
        torch = self._torch
        plans = []
        for plan in self._plans:
            plans.append(plan)
            if len(plans) == self.batch_size:
                break
        if not plans:
            raise StopIteration
        n = len(plans)
        rows = self.store.check_rows(self.store.rows_for_plans(plans, self.loader._randomness))
        slot = self._slot
        self._slot = (slot + 1) % self.SLOTS
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()        # SLOTS batches ago: long complete
        host = self.host[slot][:2 * n]
        host.numpy()[:] = rows
        with torch.cuda.device(self.device):
            rows_dev = host.to(self.device, non_blocking=True)
            self.copied[slot] = torch.cuda.Event()
            self.copied[slot].record()
            s = self.store.image_size
            both = self.store.augment(rows_dev, 2 * n).view(2, n, s, s, 3)
        return {'image': both[0], 'future_image': both[1]}


# ================================================================================================ stage 2: resident key-point labels
# csrc/augment_seq.hip, include/kpx.h ABI 12.  ``SequenceDataLoader.batches(..., resident=True)`` keeps every listed video's pseudo-label
# array in one flat float32 device buffer and produces {'keypoints', 'real_seq', 'action_code'} with ONE launch per batch -- the floats
# ``SequenceDataLoader.render`` + ``_collate`` produce, bit for bit.  The start frame, which the model never reads, is not produced;
# ``start_images`` renders it on the host for the two samples an image summary shows.  Cosine, sine and the scale are Python floats
# computed here (``seq_trig``; ``plan.scale``) and reach the kernel as doubles: the device runs no transcendental and no division.

# mirrors of include/kpx.h (tests/test_resident_seq_cpu.py holds them equal to the header)
SEQ_ROW_INTS, SEQ_ROTATE, SEQ_FLIP, SEQ_SCALE = 8, 1, 2, 4
SEQ_LEN, SEQ_ANGLES, SEQ_MAX_ROWS, SEQ_MAX_POINTS, SEQ_MAX_ACTIONS = 33, 31, 4096, 256, 256
S_VIDEO, S_IM_IDX, S_GAP, S_FLAGS, S_ANGLE, S_SCALE_LO, S_SCALE_HI, S_ACTION = range(8)
SEQ_ANGLE_MIN = -15                # plan(): randrange(-15, 16); the angle's index into the trig table is angle - SEQ_ANGLE_MIN
SEQ_SHORT = (SEQ_LEN - 1) // 2 + 1      # label rows the short-video form (gap 0) reads


def seq_trig():
    """float64 [SEQ_ANGLES, 2]: cos and sin of radians(-angle) for angle = -15..15, the expressions of data.rotate_keypoints."""
    return np.array([[math.cos(math.radians(-a)), math.sin(math.radians(-a))] for a in range(SEQ_ANGLE_MIN, SEQ_ANGLE_MIN + SEQ_ANGLES)],
                    np.float64)


def label_path(data_dir, video):
    return osp.join(data_dir, video.replace('frames', 'pseudo_labels') + '.npy')


class LabelIndex(object):
    """Which videos a label store holds: per video its frame count (what ``SequenceDataLoader._n_frames`` lists), its label rows and the
    element offset of its array in the flat buffer ``labels``; per line of the listing its action index.  Host only."""

    def __init__(self, names, counts, arrays, actions, n_points):
        self.names, self.n_points = list(names), int(n_points)
        if not 1 <= self.n_points <= SEQ_MAX_POINTS:
            raise _error('n_points = %d, the key-point kernel takes 1..%d' % (self.n_points, SEQ_MAX_POINTS))
        self._video = {name: i for i, name in enumerate(self.names)}
        self.n_frames = np.array(counts, np.int64).reshape(-1)
        for name, n, a in zip(self.names, self.n_frames, arrays):
            if a.dtype != np.float32 or a.ndim != 3 or a.shape[1:] != (self.n_points, 2):
                raise _error('%s: pseudo labels %s %s, expected float32 [len, %d, 2]' % (name, a.dtype, a.shape, self.n_points))
            if a.shape[0] < n:
                raise _error('%s: %d label rows for %d frame files' % (name, a.shape[0], n))
        self.label_rows = np.array([a.shape[0] for a in arrays], np.int64).reshape(-1)
        self.offsets = np.concatenate([[0], np.cumsum(self.label_rows * self.n_points * 2)[:-1]]).astype(np.int64)
        self.labels = np.concatenate([a.reshape(-1) for a in arrays]) if arrays else np.zeros(0, np.float32)
        self.actions = [int(a) for a in actions]

    @classmethod
    def scan(cls, data_dir, listing, n_points):
        """From the files: one ``os.listdir`` and one ``np.load`` per distinct video, in listing order."""
        names = []
        for line in listing:
            v = line.split()[0]
            if v not in names:
                names.append(v)
        counts = [len(os.listdir(osp.join(data_dir, v))) for v in names]
        arrays = [np.load(label_path(data_dir, v)) for v in names]
        return cls(names, counts, arrays, [line.split()[1] for line in listing], n_points)

    def video(self, name):
        return self._video[name]

    def count(self, name):
        return int(self.n_frames[self._video[name]])

    def array(self, name):
        v = self._video[name]
        o = int(self.offsets[v])
        return self.labels[o:o + int(self.label_rows[v]) * self.n_points * 2].reshape(-1, self.n_points, 2)


class SequencePlanner(object):
    """Table rows (include/kpx.h: kpx_keypoint_seq_augment_f32) from ``SeqPlan``s or by hand, and their validation.  Host only."""

    def __init__(self, index, n_action):
        self.index, self.n_action = index, int(n_action)
        if not 1 <= self.n_action <= SEQ_MAX_ACTIONS:
            raise _error('n_action = %d, the key-point kernel takes 1..%d' % (self.n_action, SEQ_MAX_ACTIONS))

    def row(self, video, im_idx, gap, action, angle=None, flip=0, scale=None):
        """One table row.  ``angle`` None: no rotation, ``scale`` None: no scaling (the loader without ``randomness``); an angle of 0 and a
        scale of 1.0 ARE performed, as ``render`` performs them."""
        flags = (SEQ_ROTATE if angle is not None else 0) | (SEQ_FLIP if flip else 0) | (SEQ_SCALE if scale is not None else 0)
        lo, hi = np.array([1.0 if scale is None else scale], np.float64).view(np.int32)        # little endian: low word first
        return [self.index.video(video), im_idx, gap, flags, 0 if angle is None else angle - SEQ_ANGLE_MIN, int(lo), int(hi), action]

    def rows_for_plans(self, plans):
        """int32 [len(plans), SEQ_ROW_INTS]; a plan drawn without ``randomness`` (angle None) sets no flag."""
        rows = [self.row(p.video, p.im_idx, int(p.n_files / SEQ_LEN), self.index.actions[p.index], p.angle, p.flip, p.scale) for p in plans]
        return np.array(rows, np.int64).astype(np.int32).reshape(-1, SEQ_ROW_INTS)

    def check_rows(self, rows):
        """Raises ``KpxError`` for a row the kernel cannot take; it trusts the table and clamps nothing."""
        rows = np.asarray(rows)
        if rows.dtype != np.int32 or rows.ndim != 2 or rows.shape[1] != SEQ_ROW_INTS or not 0 < rows.shape[0] <= SEQ_MAX_ROWS:
            raise _error('key-point rows: int32 [1..%d, %d] expected, got %s %s' % (SEQ_MAX_ROWS, SEQ_ROW_INTS, rows.dtype, rows.shape))
        idx = self.index
        video = rows[:, S_VIDEO].astype(np.int64)
        if (video < 0).any() or (video >= len(idx.names)).any():
            raise _error('key-point rows: video number outside the store (0..%d)' % (len(idx.names) - 1))
        im_idx, gap = rows[:, S_IM_IDX].astype(np.int64), rows[:, S_GAP].astype(np.int64)
        last = np.where(gap >= 1, im_idx + (SEQ_LEN - 1) * gap, im_idx + SEQ_SHORT - 1)
        if (im_idx < 0).any() or (gap < 0).any() or (last >= idx.label_rows[video]).any():
            raise _error("key-point rows: the sequence leaves its video's label rows")
        if (rows[:, S_FLAGS] & ~(SEQ_ROTATE | SEQ_FLIP | SEQ_SCALE)).any():
            raise _error('key-point rows: unknown flag')
        if (rows[:, S_ANGLE] < 0).any() or (rows[:, S_ANGLE] >= SEQ_ANGLES).any():
            raise _error('key-point rows: angle index outside 0..%d' % (SEQ_ANGLES - 1))
        if (rows[:, S_ACTION] < 0).any() or (rows[:, S_ACTION] >= self.n_action).any():
            raise _error('key-point rows: action index outside 0..%d' % (self.n_action - 1))
        return rows


class ResidentLabels(SequencePlanner):
    """Every listed video's pseudo labels in ONE flat float32 device buffer, with the offsets and the trig table beside it."""

    def __init__(self, data_dir, listing, n_points, n_action, device, index=None):
        """``index``: a ``LabelIndex`` built by the caller (from arrays, say) takes the place of the scan of ``data_dir``."""
        import torch
        device = torch.device(device)
        if device.type != 'cuda':
            raise _error('resident labels live in HBM: device %s is not a GPU (the package has no CPU fallback)' % device)
        if index is None:
            index = LabelIndex.scan(data_dir, listing, n_points)
        super(ResidentLabels, self).__init__(index, n_action)      # raises before anything is allocated
        self.device = device
        self.labels = torch.from_numpy(self.index.labels).to(device)
        self.label_off = torch.from_numpy(self.index.offsets).to(device)
        self.trig = torch.from_numpy(seq_trig()).to(device)

    def augment(self, rows_dev, n_rows):
        """The launch on the current stream: rows_dev = DEVICE int32 [>= n_rows, SEQ_ROW_INTS] (validated by the caller with
        ``check_rows``) -> {'keypoints' [n,K,2], 'real_seq' [n,32,K,2], 'action_code' [n,A]} float32."""
        import torch
        from ._lib import lib, check
        k, a = self.index.n_points, self.n_action
        with torch.cuda.device(self.device):
            out = {'keypoints': torch.empty((n_rows, k, 2), dtype=torch.float32, device=self.device),
                   'real_seq': torch.empty((n_rows, SEQ_LEN - 1, k, 2), dtype=torch.float32, device=self.device),
                   'action_code': torch.empty((n_rows, a), dtype=torch.float32, device=self.device)}
            check(lib.kpx_keypoint_seq_augment_f32(self.labels.data_ptr(), self.label_off.data_ptr(), rows_dev.data_ptr(), n_rows, k, a,
                                                   self.trig.data_ptr(), out['keypoints'].data_ptr(), out['real_seq'].data_ptr(),
                                                   out['action_code'].data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
                  'kpx_keypoint_seq_augment_f32')
        return out

    def augment_rows(self, rows):
        """Host rows (``row`` / ``rows_for_plans``) -> the batch: validation, upload, the launch."""
        import torch
        rows = self.check_rows(np.ascontiguousarray(rows))
        return self.augment(torch.from_numpy(rows).to(self.device), rows.shape[0])


class ResidentSeqBatcher(object):
    """``SequenceDataLoader.batches(..., resident=True)``: the host iterator's batching (``batch_size`` plans of a pass, a short batch at
    the end of every pass, passes repeated with ``repeat``) on a ``ResidentLabels`` store, from the same ``plans()``.  Per batch one pinned
    int32 table goes to the device asynchronously and one launch is enqueued on the consumer's stream; the host never waits for the device."""
    SLOTS = 4

    def __init__(self, loader, batch_size, device, repeat):
        import torch
        self._torch = torch
        self.loader, self.batch_size, self.repeat = loader, batch_size, repeat
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _error('resident=True needs a GPU device, got %s (the package has no CPU fallback)' % self.device)
        if loader._with_image_seq:
            raise _error('resident=True yields key points only: a loader with_image_seq=True needs the host path')
        if batch_size > SEQ_MAX_ROWS:
            raise _error('batch_size %d, the key-point kernel takes %d rows' % (batch_size, SEQ_MAX_ROWS))
        self.store = loader.resident_labels(self.device)
        self.host = [torch.empty((batch_size, SEQ_ROW_INTS), dtype=torch.int32).pin_memory() for _ in range(self.SLOTS)]
        self.copied = [None] * self.SLOTS          # per pinned slot: event after its last H2D copy
        self._slot = 0
        self._chunks = self._chunk_stream()
        self._last = []

    def _chunk_stream(self):
        while True:
            chunk = []
            for plan in self.loader.plans():
                chunk.append(plan)
                if len(chunk) == self.batch_size:
                    yield chunk
                    chunk = []
            if chunk:
                yield chunk
            if not self.repeat:
                break

    def __iter__(self):
        return self

    def __next__(self):
        torch = self._torch
        plans = next(self._chunks)
        n = len(plans)
        rows = self.store.check_rows(self.store.rows_for_plans(plans))
        slot = self._slot
        self._slot = (slot + 1) % self.SLOTS
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()        # SLOTS batches ago: long complete
        host = self.host[slot][:n]
        host.numpy()[:] = rows
        with torch.cuda.device(self.device):
            rows_dev = host.to(self.device, non_blocking=True)
            self.copied[slot] = torch.cuda.Event()
            self.copied[slot].record()
            out = self.store.augment(rows_dev, n)
        self._last = plans
        return out

    def start_images(self, n):
        """float32 [n, S, S, 3] in [-1, 1] on the device: the start frames of the first ``n`` samples of the batch most recently
        yielded, rendered on the host by the PIL code of ``render`` (what the host feed's 'image' holds for those samples)."""
        plans = self._last[:n]
        if not plans:
            raise _error('start_images: no batch has been yielded yet')
        return _to_device_unit(np.stack([self.loader.render_start_image(p) for p in plans]), self.device)
