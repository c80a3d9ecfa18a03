"""numpy restatement of csrc/augment.hip for the resident-frame tests: the same integer / strictly ordered float32 arithmetic, driven by
the SAME host tables (kpx_amd.resident: resize_table, rotate_constants, filter_kernels, table rows).  tests/test_resident_cpu.py compares
it with PIL itself; it is the specification the kernels are written from.  (Helper module, no tests.)"""
import io
import os

import numpy as np
from PIL import Image

f32 = np.float32


def apply_pass(a, xmin, cnt, k):
    """One resize pass along axis 1 of uint8 [H, W, 3]: out[:, i] = clip((2^21 + sum_j k[i, j] * a[:, xmin[i] + j]) >> 22, 0, 255)."""
    out = np.empty((a.shape[0], len(xmin), 3), np.uint8)
    for i in range(len(xmin)):
        kk = k[i, :cnt[i]].astype(np.int64)
        s = (a[:, xmin[i]:xmin[i] + cnt[i]].astype(np.int64) * kk[None, :, None]).sum(1) + (1 << 21)
        out[:, i] = np.clip(s >> 22, 0, 255)
    return out


def resize(a, htable, vtable):
    return apply_pass(apply_pass(a, *htable).transpose(1, 0, 2), *vtable).transpose(1, 0, 2)


def rotate(a, consts):
    """NEAREST gather in 16.16 fixed point; consts = (a0..a5) or None for the identity."""
    if consts is None:
        return a
    a0, a1, a2, a3, a4, a5 = consts
    h, w, _ = a.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (a2 + a1 * ys + a0 * xs) >> 16
    yin = (a5 + a4 * ys + a3 * xs) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(a)
    out[ok] = a[yin[ok], xin[ok]]
    return out


def clip8(s):
    return np.where(s <= 0, 0, np.where(s >= 255, 255, np.trunc(s))).astype(np.uint8)


def kernel_filter(a, kern):
    """kern: one row of resident.filter_kernels() (size, float32(offset) + 0.5, coefficients).  Kernel rows from the bottom one up, each
    summed left to right on its own, every product and sum rounded to float32; the outer size // 2 rows and columns are copied."""
    size = int(kern[0])
    r = size // 2
    kf = kern[2:2 + size * size].reshape(size, size)
    hh, ww, _ = a.shape
    n, m = hh - 2 * r, ww - 2 * r
    s = np.full((n, m, 3), kern[1], f32)
    for ky in range(size - 1, -1, -1):
        row = None
        for kx in range(size):
            p = a[ky:ky + n, kx:kx + m].astype(f32) * kf[ky, kx]
            row = p if row is None else row + p
        s = s + row
    out = a.copy()
    out[r:-r, r:-r] = clip8(s)
    return out


def gray(a):
    return ((a[..., 0].astype(np.int64) * 19595 + a[..., 1].astype(np.int64) * 38470 + a[..., 2].astype(np.int64) * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, v, f):
    """f: the float32 factor the kernel gets."""
    t = d.astype(f32) + f32(f) * (v.astype(f32) - d.astype(f32))
    return clip8(t)


def enhance(a, filt, f, identity, kernels):
    if identity:
        return a
    if filt == 6:
        d = kernel_filter(a, kernels[2])
    elif filt == 7:
        d = np.zeros_like(a)
    elif filt == 8:
        d = np.repeat(gray(a)[..., None], 3, 2)
    else:
        d = np.full_like(a, (int(gray(a).astype(np.int64).sum()) + 8192) >> 14)
    return blend(d, a, f)


def render_row(frame, row, tabs, kernels, band=16):
    """One table row -> the uint8 128 x 128 x 3 tile, in the geometry kernel's decomposition: per band of 16 tile rows only the rows of
    the horizontally resized frame that the band's vertical taps read, and of those the 128 crop columns."""
    from kpx_amd import resident as R
    h, w, _ = frame.shape
    assert (w, h) == (row[R.R_W], row[R.R_H])
    x0, y0, flags = int(row[R.R_X0]), int(row[R.R_Y0]), int(row[R.R_FLAGS])
    rot = rotate(frame, tuple(int(v) for v in row[R.R_A0:R.R_A5 + 1]) if flags & R.ROTATE else None)

    def table(off, stride, lo, n):
        t = tabs[off + lo * stride: off + (lo + n) * stride].reshape(n, stride)
        return t[:, 0].copy(), t[:, 1], t[:, 2:]
    hx, hc, hk = table(int(row[R.R_HTAB]), int(row[R.R_HSTRIDE]), x0, 128)
    tile = np.empty((128, 128, 3), np.uint8)
    for b in range(128 // band):
        vx, vc, vk = table(int(row[R.R_VTAB]), int(row[R.R_VSTRIDE]), y0 + b * band, band)
        ir0, ir1 = int(vx[0]), int((vx + vc).max())
        inter = apply_pass(rot[ir0:ir1], hx, hc, hk)                              # [rows, 128, 3]
        tile[b * band:(b + 1) * band] = apply_pass(inter.transpose(1, 0, 2), vx - ir0, vc, vk).transpose(1, 0, 2)
    if flags & R.FLIP:
        tile = tile[:, ::-1]
    filt = int(row[R.R_FILT])
    if 0 <= filt < 6:
        tile = kernel_filter(tile, kernels[filt])
    elif filt >= 6:
        tile = enhance(tile, filt, np.array([row[R.R_FVAL]], np.int32).view(f32)[0], flags & R.IDENTITY, kernels)
    return np.ascontiguousarray(tile)


# ---------------------------------------------------------------------------------------------- synthetic JPEG frames for the tests
def jpeg_frame(w, h, seed):
    """A decoded JPEG frame with smooth structure, noise and saturated patches (0 and 255, so that the clipping branches run)."""
    rs = np.random.RandomState(seed)
    low = (rs.rand(h // 16 + 2, w // 16 + 2, 3) * 255).astype(np.uint8)
    img = np.asarray(Image.fromarray(low).resize((w, h), Image.BILINEAR)).astype(np.float32) + rs.randn(h, w, 3) * 12
    img[: h // 3, : w // 4] = 255
    img[h // 2: h // 2 + h // 4, w // 3: w // 3 + w // 4] = 0
    img[h - h // 5:, w - w // 5:] = rs.randint(0, 2, (h // 5, w // 5, 1)) * 255
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, format='JPEG', quality=90)
    return Image.open(io.BytesIO(buf.getvalue()))


def write_dataset(root, sizes, frames=12, subsets=('train',)):
    """One video of ``frames`` JPEG frames per size under root/NNNN/, listed in root/<subset>_set.txt -> the video names."""
    names = ['%04d' % v for v in range(len(sizes))]
    for v, (w, h) in enumerate(sizes):
        os.makedirs(os.path.join(root, names[v]))
        for i in range(frames):
            jpeg_frame(w, h, 100 * v + i).save(os.path.join(root, names[v], '%06d.jpg' % (i + 1)), format='JPEG', quality=90)
    for subset in subsets:
        with open(os.path.join(root, subset + '_set.txt'), 'w') as f:
            f.write(''.join('%s %d\n' % (n, v) for v, n in enumerate(names)))
    return names
