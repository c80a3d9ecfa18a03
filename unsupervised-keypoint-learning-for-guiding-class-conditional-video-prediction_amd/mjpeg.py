"""True-colour video files of rollouts (evaluate.py --video, animate.py --video; DESIGN.md sections 2 and 4.4): Motion-JPEG in an AVI.

Every frame is a baseline JPEG (4:2:0, the Annex K tables of ITU T.81 scaled by the IJG quality rule, one restart interval per row of
16 x 16 MCUs).  The device writes the entropy-coded scan (``jpeg_scans`` / ``jpeg_encode`` below, public as ``ops.jpeg_encode``:
csrc/mjpeg.hip, integers only); everything else in this file is host work on bytes that needs neither torch nor a GPU, so
``python -m kpx_amd.mjpeg FILE.avi --png DIR`` unpacks a file on any machine the package imports on:

    quant_tables(quality)           the two quantisation tables
    frame_prefix(H, W, qtables)     SOI .. SOS, the same bytes for every frame of a call
    frame_bytes(prefix, scan)       one JPEG
    write_avi / read_avi            the RIFF container: hdrl (avih, strl: strh + strf), movi (00dc chunks), idx1
"""
import json
import os
import struct

import numpy as np

FPS_RANGE = (1, 240)
QUALITY_RANGE = (1, 100)
MAX_FILE_BYTES = 1 << 31                          # a plain AVI (no OpenDML): 32-bit sizes and offsets

# ---- ITU T.81 Annex K.1 / K.2, natural (row-major) order
QUANT_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
QUANT_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# ---- Annex K.3 - K.6: (number of codes of each length 1..16, symbols in code order); the table class and id of its DHT segment
_AC_TAIL = tuple(r << 4 | s for r in range(8, 16) for s in range(2, 11))
HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
      0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27,
      0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a) + tuple(r << 4 | s for r in range(4, 8) for s in range(3, 11))
     + (0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a) + _AC_TAIL[9:54] + tuple(r << 4 | s for r in (14, 15) for s in range(1, 11))),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
      0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a,
      0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a) + tuple(r << 4 | s for r in range(4, 8) for s in range(3, 11)) + _AC_TAIL),
)

# ZIGZAG[k] = the natural index of the k-th coefficient of the scan (DQT stores its table in this order)
ZIGZAG = tuple(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) & 1 else i % 8)))


def quant_tables(quality):
    """The IJG quality rule on the Annex K tables: s = 5000 // q below 50, else 200 - 2 q; Q = clamp((base s + 50) // 100, 1, 255)
    -> uint8 [2, 64] (luma, chroma) in natural order: the tables PIL uses for ``quality=q``."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not QUALITY_RANGE[0] <= quality <= QUALITY_RANGE[1]:
        raise ValueError('quant_tables: quality is an integer in 1..100 (got %r)' % (quality,))
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((np.array(base, np.int64) * s + 50) // 100, 1, 255) for base in (QUANT_LUMA, QUANT_CHROMA)]).astype(np.uint8)


def _segment(marker, payload):
    return struct.pack('>BBH', 0xff, marker, len(payload) + 2) + payload


def frame_prefix(H, W, qtables):
    """SOI, APP0 (JFIF 1.1), DQT x 2, SOF0 (Y 2x2, Cb 1x1, Cr 1x1), DHT x 4, DRI (one row of MCUs), SOS: everything before the scan"""
    qtables = np.asarray(qtables)
    if qtables.shape != (2, 64) or qtables.dtype.kind not in 'iu' or qtables.min() < 1 or qtables.max() > 255:
        raise ValueError('frame_prefix: qtables must be integers [2, 64] in 1..255')
    if H % 16 or W % 16 or not 16 <= H <= 4096 or not 16 <= W <= 4096:
        raise ValueError('frame_prefix: H and W are multiples of 16 in 16..4096 (got %r x %r)' % (H, W))
    parts = [b'\xff\xd8', _segment(0xe0, b'JFIF\x00' + struct.pack('>BBBHHBB', 1, 1, 0, 1, 1, 0, 0))]
    for i in range(2):
        parts.append(_segment(0xdb, bytes([i]) + bytes(int(qtables[i, z]) for z in ZIGZAG)))
    parts.append(_segment(0xc0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, bits, vals in HUFFMAN:
        parts.append(_segment(0xc4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    parts.append(_segment(0xdd, struct.pack('>H', W // 16)))
    parts.append(_segment(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(parts)


def frame_bytes(prefix, scan):
    return prefix + bytes(scan) + b'\xff\xd9'


# ------------------------------------------------------------------------------------------------------------------- the container
_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10


def avi_bytes(frames, fps, H, W):
    """frames: JPEG byte strings -> the bytes of a RIFF 'AVI ' file:

        RIFF size 'AVI '
          LIST size 'hdrl'
            'avih' 56: us per frame, max bytes per second, 0, AVIF_HASINDEX, frames, 0, 1 stream, largest chunk, W, H, 4 x 0
            LIST size 'strl'
              'strh' 56: 'vids' 'MJPG', 0, 0, 0, 0, dwScale 1, dwRate fps, 0, frames, largest chunk, quality -1, 0, rcFrame (0, 0, W, H)
              'strf' 40: BITMAPINFOHEADER 40, W, H, 1 plane, 24 bits, 'MJPG', W H 3, 0, 0, 0, 0
          LIST size 'movi': per frame '00dc' size data, a zero byte after an odd size
          'idx1' 16 per frame: '00dc', AVIIF_KEYFRAME, offset of the chunk from the 'movi' fourcc, size
    """
    frames = [bytes(f) for f in frames]
    if isinstance(fps, bool) or not isinstance(fps, (int, np.integer)) or not FPS_RANGE[0] <= fps <= FPS_RANGE[1]:
        raise ValueError('write_avi: fps is an integer in %d..%d (got %r)' % (FPS_RANGE + (fps,)))
    if not frames or min(len(f) for f in frames) < 1:
        raise ValueError('write_avi: at least one frame, none of them empty')
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError('write_avi: H and W in 1..65535 (got %r x %r)' % (H, W))
    n, largest = len(frames), max(len(f) for f in frames)
    movi_size = 4 + sum(8 + len(f) + (len(f) & 1) for f in frames)
    total = 12 + (8 + 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))) + (8 + movi_size) + (8 + 16 * n)
    if total >= MAX_FILE_BYTES:
        raise ValueError('write_avi: the file would hold %d bytes, and a plain AVI ends below 2^31' % total)
    strh = struct.pack('<4s4sIHHIIIIIIiI4h', b'vids', b'MJPG', 0, 0, 0, 0, 1, int(fps), 0, n, largest, -1, 0, 0, 0, W, H)
    strf = struct.pack('<IiiHH4sIiiII', 40, W, H, 1, 24, b'MJPG', W * H * 3, 0, 0, 0, 0)
    strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
    avih = struct.pack('<14I', 1000000 // int(fps), largest * int(fps), 0, _AVIF_HASINDEX, n, 0, 1, largest, W, H, 0, 0, 0, 0)
    hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
    movi, idx, off = [b'movi'], [], 4
    for f in frames:
        movi.append(b'00dc' + struct.pack('<I', len(f)) + f + (b'\x00' if len(f) & 1 else b''))
        idx.append(struct.pack('<4sIII', b'00dc', _AVIIF_KEYFRAME, off, len(f)))
        off += 8 + len(f) + (len(f) & 1)
    movi, idx = b''.join(movi), b''.join(idx)
    body = (b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl + b'LIST' + struct.pack('<I', len(movi)) + movi
            + b'idx1' + struct.pack('<I', len(idx)) + idx)
    data = b'RIFF' + struct.pack('<I', len(body)) + body
    assert len(data) == total and len(movi) == movi_size
    return data


def write_avi(path, frames, fps, H, W):
    data = avi_bytes(frames, fps, H, W)
    with open(path, 'wb') as f:
        f.write(data)
    return len(data)


def _chunks(data, start, end):
    """(fourcc, payload start, payload size) of the chunks of data[start:end]"""
    pos = start
    while pos + 8 <= end:
        cc, size = data[pos:pos + 4], struct.unpack_from('<I', data, pos + 4)[0]
        if pos + 8 + size > end:
            raise ValueError('read_avi: chunk %r at %d runs past its parent' % (cc, pos))
        yield cc, pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path):
    """-> (fps, H, W, [the JPEG of every frame]) of a file ``write_avi`` wrote; the frames are found through idx1 and checked against movi"""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'AVI ' or struct.unpack_from('<I', data, 4)[0] + 8 != len(data):
        raise ValueError('read_avi: %s is not a RIFF AVI file of its stated size' % path)
    fps = size_hw = movi = idx1 = None
    for cc, at, size in _chunks(data, 12, len(data)):
        if cc == b'LIST' and data[at:at + 4] == b'hdrl':
            for cc2, at2, size2 in _chunks(data, at + 4, at + size):
                if cc2 == b'avih':
                    n_frames, (w, h) = struct.unpack_from('<I', data, at2 + 16)[0], struct.unpack_from('<II', data, at2 + 32)
                    size_hw = (h, w)
                elif cc2 == b'LIST' and data[at2:at2 + 4] == b'strl':
                    for cc3, at3, size3 in _chunks(data, at2 + 4, at2 + size2):
                        if cc3 == b'strh':
                            if data[at3:at3 + 8] != b'vidsMJPG':
                                raise ValueError('read_avi: the stream is %r, not vids / MJPG' % data[at3:at3 + 8])
                            scale, rate = struct.unpack_from('<II', data, at3 + 20)
                            fps = rate // scale
        elif cc == b'LIST' and data[at:at + 4] == b'movi':
            movi = (at, size)
        elif cc == b'idx1':
            idx1 = (at, size)
    if fps is None or size_hw is None or movi is None or idx1 is None:
        raise ValueError('read_avi: %s lacks one of avih, strh, movi, idx1' % path)
    frames = []
    for i in range(idx1[1] // 16):
        cc, _flags, off, size = struct.unpack_from('<4sIII', data, idx1[0] + 16 * i)
        at = movi[0] + off
        if cc != b'00dc' or data[at:at + 4] != b'00dc' or struct.unpack_from('<I', data, at + 4)[0] != size or at + 8 + size > movi[0] + movi[1]:
            raise ValueError('read_avi: index entry %d does not point at a 00dc chunk of its size' % i)
        frames.append(data[at + 8:at + 8 + size])
    if len(frames) != n_frames:
        raise ValueError('read_avi: avih counts %d frames, idx1 %d' % (n_frames, len(frames)))
    return fps, size_hw[0], size_hw[1], frames


# ------------------------------------------------------------------------------------------------------------------- the device wrappers
# (``ops.jpeg_scans``, ``ops.jpeg_encode``: they reach ``tool_ops`` and ``ops`` by the import at the end of each, like ``prdc.prdc``)
JPEG_MIN_SIDE, JPEG_MAX_SIDE = 16, 4096           # = the limits of kpx_jpeg_encode_u8 (include/kpx.h); both sides multiples of 16
JPEG_BUDGET = 256 << 20                           # bytes of workspace + scans one chunk of frames may ask for (a single frame may exceed it)
_pinned = [None]


def _jpeg_sizes(what, canvas):
    import torch
    from ._args import check_tensors
    from ._lib import KpxError
    dev = check_tensors(what, [('canvas', canvas, torch.uint8, (None, None, None, 3))])
    n, h, w = (int(v) for v in canvas.shape[:3])
    if (n < 1 or h % 16 or w % 16 or not JPEG_MIN_SIDE <= h <= JPEG_MAX_SIDE or not JPEG_MIN_SIDE <= w <= JPEG_MAX_SIDE
            or n * h * w > 0x7fffffff):
        raise KpxError('%s: canvas must be [N,H,W,3] with N >= 1, H and W multiples of 16 in [16, 4096] and N H W < 2^31 (got %s)'
                       % (what, tuple(canvas.shape)))
    return dev, n, h, w


def jpeg_scans(canvas, quality, scans=None, offsets=None):
    """The entropy-coded scans of baseline JPEGs of 8-bit frames (DESIGN.md sections 2 and 4.4), all on the device.  canvas: contiguous uint8
    [N,H,W,3]; quality 1..100 (``quant_tables``) -> (scans uint8 [N * kpx_jpeg_scan_bound(H, W)], offsets int64 [N + 1]): frame n's scan is
    scans[offsets[n]:offsets[n + 1]], what ``frame_bytes`` puts between ``frame_prefix`` and EOI.  Five launches, no copy or
    synchronisation: capturable once the scratch buffer of the stream exists."""
    import torch
    from ._args import _stream, check_out, scratch
    from ._lib import KpxError, check, lib
    dev, n, h, w = _jpeg_sizes('jpeg_scans', canvas)
    try:
        qt = np.ascontiguousarray(quant_tables(quality))
    except ValueError as e:
        raise KpxError('jpeg_scans: %s' % e)
    bound = int(lib.kpx_jpeg_scan_bound(h, w))
    scans = check_out('jpeg_scans', 'scans', scans, torch.uint8, (n * bound,), dev)
    offsets = check_out('jpeg_scans', 'offsets', offsets, torch.int64, (n + 1,), dev)
    nbytes = int(lib.kpx_jpeg_workspace_bytes(n, h, w))
    ws = scratch.get('jpeg', nbytes, dev)
    check(lib.kpx_jpeg_encode_u8(canvas.data_ptr(), n, h, w, qt.ctypes.data, scans.data_ptr(), offsets.data_ptr(), ws.data_ptr(), nbytes,
                                 _stream()), 'kpx_jpeg_encode_u8')
    return scans, offsets


def jpeg_encode(canvas, quality, budget=JPEG_BUDGET):
    """canvas: contiguous uint8 [N,H,W,3] on the device -> a list of N ``bytes``, the scan of every frame (``jpeg_scans``).  The frames are
    coded in chunks whose workspace and scan buffer stay within ``budget`` bytes (at least one frame a chunk); per chunk one read of the
    offsets, then one copy of the bytes in use into pinned memory: nothing but compressed bytes crosses to the host."""
    import torch
    from ._args import scratch
    from ._lib import KpxError, lib
    dev, n, h, w = _jpeg_sizes('jpeg_encode', canvas)
    if isinstance(budget, bool) or not isinstance(budget, int) or budget < 1:
        raise KpxError('jpeg_encode: budget is a positive number of bytes (got %r)' % (budget,))
    bound = int(lib.kpx_jpeg_scan_bound(h, w))
    per = max(1, budget // (int(lib.kpx_jpeg_workspace_bytes(1, h, w)) + bound))
    out = []
    for lo in range(0, n, per):
        m = min(per, n - lo)
        buf = scratch.get('jpeg_scans', m * bound, dev)
        scans, offsets = jpeg_scans(canvas[lo:lo + m], quality, buf[:m * bound])
        off = offsets.cpu().numpy()               # synchronous: the one read of the chunk
        used = int(off[m])
        if _pinned[0] is None or _pinned[0].numel() < used:
            _pinned[0] = torch.empty(max(used, 1 << 20), dtype=torch.uint8, pin_memory=True)
        host = _pinned[0][:used]
        host.copy_(scans[:used])
        data = host.numpy().tobytes()
        out.extend(data[int(off[i]):int(off[i + 1])] for i in range(m))
    return out


# ------------------------------------------------------------------------------------------------------------------- the tools' writers
def canvas_avi(path, canvas, fps, quality):
    """canvas: uint8 [T, H, W, 3] on the device -> one AVI of its T frames, encoded by ``ops.jpeg_encode``; the file's size in bytes"""
    from . import ops
    h, w = int(canvas.shape[1]), int(canvas.shape[2])
    prefix = frame_prefix(h, w, quant_tables(quality))
    return write_avi(path, [frame_bytes(prefix, s) for s in ops.jpeg_encode(canvas, quality)], fps, h, w)


class RolloutVideos:
    """evaluate.py --video: per batch, the canvases of pred.avi and compare.avi composed (``gif.RolloutGifs._canvas``) and JPEG-coded on the
    device, so only the compressed scans reach the host; written per sample; video.json at the end."""

    def __init__(self, fps, quality):
        from .gif import RolloutGifs
        self.fps, self.quality = int(fps), int(quality)
        self.columns = self.frames = self.cell = None
        self.bytes = {'pred': [], 'compare': []}
        self._canvas = RolloutGifs(1, 0)._canvas

    def write_canvas(self, save_dir, first_sample, name, canvas, sizes):
        """canvas: uint8 [B, T, H, W, 3] on the device -> <save_dir>/<sample>/<name>.avi per sample, the sizes appended to ``sizes``"""
        from . import ops
        b, t, h, w = (int(v) for v in canvas.shape[:4])
        prefix = frame_prefix(h, w, quant_tables(self.quality))
        scans = ops.jpeg_encode(canvas.view(b * t, h, w, 3), self.quality)
        for i in range(b):
            d = os.path.join(save_dir, '%04d' % (first_sample + i))
            os.makedirs(d, exist_ok=True)
            sizes.append(write_avi(os.path.join(d, name + '.avi'), [frame_bytes(prefix, s) for s in scans[i * t:(i + 1) * t]], self.fps, h, w))

    def write(self, save_dir, first_sample, columns):
        """columns: [(name, first, seq, premap)] in the order of compare.avi; the column named 'pred' alone is pred.avi"""
        self.columns = [c[0] for c in columns]
        for kind, cols in (('pred', [c[1:] for c in columns if c[0] == 'pred']), ('compare', [c[1:] for c in columns])):
            canvas = self._canvas(cols)
            self.frames, self.cell = int(canvas.shape[1]), [int(canvas.shape[2]), int(canvas.shape[3]) // len(cols)]
            self.write_canvas(save_dir, first_sample, kind, canvas, self.bytes[kind])

    def write_json(self, save_dir):
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, 'video.json'), 'w') as f:
            json.dump({'columns': self.columns, 'fps': self.fps, 'quality': self.quality, 'frames': self.frames, 'cell': self.cell,
                       'bytes': self.bytes}, f, indent=1)


def main(argv=None):
    import argparse
    import io
    parser = argparse.ArgumentParser(prog='python -m kpx_amd.mjpeg', description='List the frames of a Motion-JPEG AVI, or unpack them to PNGs.')
    parser.add_argument('avi')
    parser.add_argument('--png', metavar='DIR', default=None, help='decode every frame (PIL) and write DIR/00000.png, DIR/00001.png, ...')
    args = parser.parse_args(argv)
    fps, h, w, frames = read_avi(args.avi)
    print('%s: %d frames of %d x %d at %d fps, %d bytes of JPEG' % (args.avi, len(frames), w, h, fps, sum(len(f) for f in frames)))
    if args.png is not None:
        from PIL import Image
        os.makedirs(args.png, exist_ok=True)
        for i, f in enumerate(frames):
            Image.open(io.BytesIO(f)).convert('RGB').save(os.path.join(args.png, '%05d.png' % i))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
