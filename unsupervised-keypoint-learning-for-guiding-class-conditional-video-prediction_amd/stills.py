"""Stills as inputs (animate.py): listing, decoding and fitting the user's own images on the host, the limits of an
animated grid, and the grids' way to GIF files.

A still is decoded with PIL (``ImageOps.exif_transpose``, then ``convert('RGB')``: L, P, RGBA and CMYK all arrive as RGB, and an alpha
channel is DROPPED as ``convert`` drops it, not composited), optionally cropped to a box given in pixels of the upright image, and then
fitted with the arithmetic the sequence loader applies to a start frame: ``center_crop_box(w, h)`` and ``image.resize(size).crop(box)``.
The networks therefore see a still exactly as they would see a Penn frame of the same pixels.  There is no device resize: the decode
dominates and PIL is the definition.
"""
import os
import os.path as osp

import numpy as np

from . import ops
from .data import IMAGE_SIZE, N_SEQUENCE_LEN, center_crop_box, check_image_size

IMAGE_EXTS = ('.jpg', '.jpeg', '.png', '.bmp')
HIST_MAX_PIXELS = ops.HIST_MAX_PIXELS          # pixels of one GIF: what the uint32 sums of kpx_color_hist_add_u32 hold
MAX_GRID = 64                                  # rows and columns of cells of a canvas (kpx_cell_frames_u8_f32)
MAX_RADIUS = ops.CELL_MAX_RADIUS
CANVAS_BYTES = 1 << 30             # the canvases of one batch stay under this


class StillsError(ValueError):
    pass


def parse_box(text, what):
    """'x0,y0,x1,y1' -> (x0, y0, x1, y1) integers; the sides are checked against an image by ``check_box``"""
    try:
        box = tuple(int(v) for v in text.split(','))
    except ValueError:
        raise StillsError('%s takes x0,y0,x1,y1 in whole pixels (got %r)' % (what, text))
    if len(box) != 4:
        raise StillsError('%s takes four integers x0,y0,x1,y1 (got %r)' % (what, text))
    return box


def check_box(box, w, h, what):
    x0, y0, x1, y1 = box
    if not (0 <= x0 and 0 <= y0 and x1 <= w and y1 <= h):
        raise StillsError('%s %s does not lie inside the %d x %d image' % (what, list(box), w, h))
    if x1 - x0 < 2 or y1 - y0 < 2:
        raise StillsError('%s %s needs both sides >= 2 pixels' % (what, list(box)))


def is_image(name):
    return name.lower().endswith(IMAGE_EXTS)


def list_images(paths, box=None, what='--images'):
    """paths: image files, directories (their image files in sorted name order) and .txt manifests (one ``path [x0,y0,x1,y1]`` per line,
    paths relative to the manifest; its box overrides ``box``) -> [(path, box or None)] in input order"""
    out = []
    for p in paths:
        before = len(out)
        if osp.isdir(p):
            out.extend((osp.join(p, n), box) for n in sorted(os.listdir(p)) if is_image(n) and osp.isfile(osp.join(p, n)))
        elif p.lower().endswith('.txt'):
            if not osp.isfile(p):
                raise StillsError('%s: no manifest at %s' % (what, p))
            with open(p, 'r') as f:
                lines = f.read().splitlines()
            for n, line in enumerate(lines):
                line = line.strip()
                if not line or line.startswith('#'):
                    continue
                name, own = line, None
                head, _, tail = line.rpartition(' ')
                if head and tail.count(',') == 3:
                    name, own = head.strip(), parse_box(tail, '%s: line %d of %s' % (what, n + 1, p))
                full = name if osp.isabs(name) else osp.join(osp.dirname(osp.abspath(p)), name)
                if not osp.isfile(full):
                    raise StillsError('%s: line %d of %s names %s, which is no file' % (what, n + 1, p, name))
                out.append((full, own if own is not None else box))
        elif osp.isfile(p):
            out.append((p, box))
        if len(out) == before:
            raise StillsError('%s: %s yields no image (files, directories of %s files, or .txt manifests)' % (what, p, ' '.join(IMAGE_EXTS)))
    return out


def decode(path):
    """-> the upright RGB image (PIL): EXIF orientation applied, then convert('RGB'); alpha is dropped"""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        return ImageOps.exif_transpose(im).convert('RGB')


def fit_image(image, box=None, what='--box', image_size=IMAGE_SIZE):
    """upright RGB PIL image -> (uint8 [S,S,3], {'decoded_size', 'box', 'resized_size', 'crop_box'}), S = image_size: the optional crop,
    then the sequence loader's start-frame arithmetic without randomness"""
    image_size = check_image_size(image_size, 'image_size')
    decoded = list(image.size)
    if box is not None:
        check_box(box, image.size[0], image.size[1], what)
        image = image.crop(tuple(box))
    w, h = image.size
    crop, ratio = center_crop_box(w, h, image_size)
    size = [int(w / ratio), int(h / ratio)]
    out = np.asarray(image.resize(size).crop(crop))
    assert out.shape == (image_size, image_size, 3) and out.dtype == np.uint8
    return out, {'decoded_size': decoded, 'box': None if box is None else list(box), 'resized_size': size, 'crop_box': list(crop)}


def fit(path, box=None, what='--box', image_size=IMAGE_SIZE):
    """an image file -> (uint8 [S,S,3], its record for animate.json), S = image_size"""
    try:
        image = decode(path)
    except (OSError, SyntaxError, ValueError) as e:
        raise StillsError('%s cannot be decoded as an image (%s)' % (path, e))
    u8, info = fit_image(image, box, what='%s of %s' % (what, path), image_size=image_size)
    return u8, dict(info, source=path)


def driver_frames(folder, what='--driver'):
    """a directory of N >= 33 frames in sorted order -> (the 33 paths used, their indices i * (N // 33), N): the sequence loader's rule at
    im_idx = 0"""
    if not osp.isdir(folder):
        raise StillsError('%s: %s is no directory' % (what, folder))
    names = [n for n in sorted(os.listdir(folder)) if is_image(n) and osp.isfile(osp.join(folder, n))]
    n = len(names)
    if n < N_SEQUENCE_LEN:
        raise StillsError('%s needs at least %d frames in %s (found %d)' % (what, N_SEQUENCE_LEN, folder, n))
    idx = [i * (n // N_SEQUENCE_LEN) for i in range(N_SEQUENCE_LEN)]
    return [osp.join(folder, names[i]) for i in idx], idx, n


def check_grid(samples, classes, h=IMAGE_SIZE, w=IMAGE_SIZE, frames=N_SEQUENCE_LEN):
    """the limits of classes.gif: a canvas grid holds at most 64 x 64 cells, and one palette is counted over ``frames`` S A H W pixels
    (33 frames unless animate.py --frames / --rate ask for more), which the uint32 histogram bounds by 2^24"""
    if not 1 <= samples <= MAX_GRID:
        raise StillsError('--samples: a grid has 1 to %d rows of draws (got %d)' % (MAX_GRID, samples))
    if not 1 <= classes <= MAX_GRID:
        raise StillsError('--actions: a grid has 1 to %d columns of classes (got %d)' % (MAX_GRID, classes))
    pixels = frames * samples * classes * h * w
    if pixels > HIST_MAX_PIXELS:
        raise StillsError('--samples x --actions: %d draws x %d classes x %d frames of %d x %d are %d pixels in one GIF, and the colour '
                          'histogram counts at most 2^24 = %d (%d cells of this size)'
                          % (samples, classes, frames, h, w, pixels, HIST_MAX_PIXELS, HIST_MAX_PIXELS // (frames * h * w)))


def batch_under(batch, bytes_per_still, limit=CANVAS_BYTES):
    """the largest batch <= ``batch`` whose canvases stay under ``limit`` bytes (at least 1)"""
    return max(1, min(int(batch), limit // max(1, int(bytes_per_still))))


def marker_colors(colors):
    """FinalModel.colors (floats in [0, 1], [K, 3]) -> the uint8 colours of the markers: trunc(c * 255)"""
    return np.trunc(np.asarray(colors, dtype=np.float64) * 255.0).astype(np.uint8)


def write_grid_gifs(gifs, canvas, paths):
    """canvas uint8 [B, T, H, Wc, 3] on the device -> one GIF per sample at paths[b], one global palette each (``ops.gif_indices``; only the
    indices cross to the host, through ``gifs``' pinned buffer) -> the palette sizes.  gifs: a ``kpx_amd.gif.RolloutGifs``."""
    from .gif import write_gif
    idx, palettes, sizes = ops.gif_indices(canvas, gifs.dither)
    host = gifs._host(idx)
    for i, path in enumerate(paths):
        write_gif(path, host[i], palettes[i, :sizes[i]], gifs.delay)
    return [int(s) for s in sizes]


def write_grid_videos(canvas, paths, fps, quality):
    """canvas uint8 [B, T, H, Wc, 3] on the device -> one Motion-JPEG AVI per sample at paths[b] (``kpx_amd.mjpeg.canvas_avi``: every frame
    JPEG-coded on the device, only the scans cross to the host) -> the file sizes in bytes"""
    from .mjpeg import canvas_avi
    return [canvas_avi(path, canvas[i], fps, quality) for i, path in enumerate(paths)]
