"""Helpers of the image-size tests (test_image_size_cpu.py, test_image_size_gpu.py): ``ImagePairDataLoader.render`` restated as the Pillow
calls it makes at a side S, the side-S version of resident_ref.render_row (the geometry kernel's decomposition in numpy, on the host tables
of kpx_amd.resident), and the enumerated decisions both tests run.  (Helper module, no tests.)"""
import numpy as np
from PIL import Image, ImageEnhance, ImageFilter

import resident_ref as ref

f32 = np.float32
SIDES = (32, 48, 256)
KERNEL_FILTERS = (ImageFilter.DETAIL, ImageFilter.EDGE_ENHANCE, ImageFilter.SMOOTH, ImageFilter.SMOOTH_MORE, ImageFilter.EDGE_ENHANCE_MORE,
                  ImageFilter.BLUR)                                   # utils/data.py:8-35, ids 0..5
ENHANCERS = {6: (ImageEnhance.Sharpness, 0, 50), 7: (ImageEnhance.Brightness, 7, 20), 8: (ImageEnhance.Color, 0, 50),
             9: (ImageEnhance.Contrast, 7, 30)}


# ---------------------------------------------------------------------------------------------- Pillow itself, at a side S
def pillow_tile(path, plan, side, randomness):
    """The frame at ``path`` up to and including the flip: rotate, resize to short side S with the loader's truncations, crop, flip."""
    im = Image.open(path)
    w, h = im.size
    if randomness:
        im = im.rotate(plan.angle)
    ratio = (h if w > h else w) / float(side)
    rw, rh = int(w / ratio), int(h / ratio)
    im = im.resize([rw, rh])
    if not randomness:
        ox = rw / 2.0                                                 # centred on the width in both orientations; the top S rows
        return im.crop((ox - side // 2, 0, ox + side // 2, side))
    c = plan.crop
    im = im.crop((c, 0, c + side, side) if w > h else (0, c, side, c + side))
    if plan.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return im


def pillow_filter(im, plan):
    if plan.filt < 6:
        return im.filter(KERNEL_FILTERS[plan.filt])
    return ENHANCERS[plan.filt][0](im).enhance(plan.filt_val * 0.1)


def pillow_render(path, plan, side, randomness):
    """-> uint8 [S, S, 3]: what ``ImagePairDataLoader(image_size=S).render`` gives for one of the plan's two frames"""
    im = pillow_tile(path, plan, side, randomness)
    return np.asarray(pillow_filter(im, plan) if randomness else im)


def band_luminance(tile, band=16):
    """uint8 [S, S, 3] -> int64 [S / 16]: per band of 16 rows the sum of Pillow's L of every pixel (what the geometry kernel leaves in lsum)"""
    grey = np.asarray(Image.fromarray(np.ascontiguousarray(tile)).convert('L')).astype(np.int64)
    return grey.reshape(tile.shape[0] // band, -1).sum(1)


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic at a side S
def contrast_grey(tile):
    """int(mean luminance + 0.5) over S * S pixels in the filter kernel's integers: (2 * sum + S^2) / (2 * S^2)"""
    area = tile.shape[0] * tile.shape[1]
    return (2 * int(ref.gray(tile).astype(np.int64).sum()) + area) // (2 * area)


def enhance(a, filt, f, identity, kernels):
    if filt == 9 and not identity:
        return ref.blend(np.full_like(a, contrast_grey(a)), a, f)
    return ref.enhance(a, filt, f, identity, kernels)                 # Sharpness, Brightness and Color do not look at the side


def render_row(frame, row, tabs, kernels, side, band=16):
    """resident_ref.render_row for a side x side tile: per band of 16 tile rows only the rows of the horizontally resized frame that the
    band's vertical taps read, and of those the ``side`` crop columns -> (filtered tile, tile before the filter)"""
    from kpx_amd import resident as R
    h, w, _ = frame.shape
    assert (w, h) == (row[R.R_W], row[R.R_H])
    x0, y0, flags = int(row[R.R_X0]), int(row[R.R_Y0]), int(row[R.R_FLAGS])
    rot = ref.rotate(frame, tuple(int(v) for v in row[R.R_A0:R.R_A5 + 1]) if flags & R.ROTATE else None)

    def table(off, stride, lo, n):
        t = tabs[off + lo * stride: off + (lo + n) * stride].reshape(n, stride)
        return t[:, 0].copy(), t[:, 1], t[:, 2:]
    hx, hc, hk = table(int(row[R.R_HTAB]), int(row[R.R_HSTRIDE]), x0, side)
    tile = np.empty((side, side, 3), np.uint8)
    for b in range(side // band):
        vx, vc, vk = table(int(row[R.R_VTAB]), int(row[R.R_VSTRIDE]), y0 + b * band, band)
        ir0, ir1 = int(vx[0]), int((vx + vc).max())
        inter = ref.apply_pass(rot[ir0:ir1], hx, hc, hk)                          # [rows, side, 3]
        tile[b * band:(b + 1) * band] = ref.apply_pass(inter.transpose(1, 0, 2), vx - ir0, vc, vk).transpose(1, 0, 2)
    if flags & R.FLIP:
        tile = tile[:, ::-1]
    plain = np.ascontiguousarray(tile)
    filt = int(row[R.R_FILT])
    if 0 <= filt < 6:
        tile = ref.kernel_filter(plain, kernels[filt])
    elif filt >= 6:
        tile = enhance(plain, filt, np.array([row[R.R_FVAL]], np.int32).view(f32)[0], flags & R.IDENTITY, kernels)
    return np.ascontiguousarray(tile), plain


# ---------------------------------------------------------------------------------------------- the decisions, enumerated
def enumerated_plans(video, w, h, side, n_frames=12):
    """PairPlans of one video at side S, written down and not drawn: every filter id 0..9 (the enhancers at both ends of their ranges and
    at 10, the identity), both flips, rotation on (several angles) and off (angle 0), the crop origins 0, max and between."""
    from kpx_amd.data import PairPlan
    ratio = (h if w > h else w) / float(side)
    cmax = int((int(w / ratio) if w > h else int(h / ratio)) - side)
    crops = [0, cmax, cmax // 2]
    angles = [-10, 0, 7, 3, 0, -4]
    filters = [(f, None) for f in range(6)] + [(f, v) for f, (_, lo, hi) in sorted(ENHANCERS.items()) for v in (lo, hi, 10)]
    return [PairPlan(video, k % n_frames, (k + 9) % n_frames, angles[k % len(angles)], crops[k % 3], (k // 2) % 2, f, v)
            for k, (f, v) in enumerate(filters)]


def coverage(rows):
    """What a set of table rows exercises -> (filter ids, flip states, rotation states, whether an identity enhancer occurs)"""
    from kpx_amd import resident as R
    rows = np.asarray(rows)
    return (set(rows[:, R.R_FILT].tolist()), set((rows[:, R.R_FLAGS] & R.FLIP != 0).tolist()),
            set((rows[:, R.R_FLAGS] & R.ROTATE != 0).tolist()), bool((rows[:, R.R_FLAGS] & R.IDENTITY).any()))


def assert_full_coverage(rows):
    filters, flips, rotations, identity = coverage(rows)
    assert filters == set(range(-1, 10)) and flips == {False, True} and rotations == {False, True} and identity, (filters, flips, rotations, identity)
