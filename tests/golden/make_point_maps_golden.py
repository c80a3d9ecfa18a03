#!/usr/bin/env python3
"""Generate tests/golden/point_maps_ref.npz.  Run in the build container only (needs /root/reference):

    python -B tests/golden/make_point_maps_golden.py

Executes the REFERENCE's own ``utils/model.py`` (get_n_colors and its helpers, colorize_point_maps, get_gaussian_maps; :13-60), unmodified,
against ``tf_standin`` (the lazy TF-1.12 stand-in of make_networks_golden.py: float64 numpy constants become fp32, as TF converts them to
the maps' dtype; ``reduce_max`` over the list of per-point maps; ``shape.as_list``) and stores:

* the palettes ``get_n_colors(K)`` draws after ``random.seed(s)`` for (s, K) in PALETTES, as float64 (Python floats);
* colourised maps ``colorize_point_maps(get_gaussian_maps(mu, [H, W]), colors)`` for seeded key-points in CASES -- coordinates in
  [-1.4, 1.4] (some outside the [-1, 1] grid), plus coordinates set exactly on grid lines of the fp32 ``tf.linspace``.  The reference renders
  every pixel; the file keeps the pixels listed in ``case_<tag>_index`` (flat indices into N*H*W): all of them for the small case, and for
  the two large ones the 5x5 neighbourhood of every key-point plus SAMPLES_PER_FRAME seeded pixels per frame (the whole maps would be 1 MB).

The stand-in's ``exp`` is torch-CPU's, not the MI355X's ``__expf``: tests compare at the Gaussian-map tolerance (atol 2e-6, rtol 2e-5).
Nothing from /root/reference is copied: only seeds, shapes and output arrays are stored.
"""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

PALETTES = ((0, 15), (1, 40), (2, 1), (3, 64))
# tag, points seed, palette seed, N, K, H, W
CASES = (('a', 21, 0, 2, 15, 128, 128), ('b', 22, 1, 1, 40, 256, 256), ('c', 23, 2, 3, 4, 40, 70))
FULL_MAX_PIXELS = 10000             # cases with at most this many pixels are stored whole
SAMPLES_PER_FRAME = 1536


def grid_line(i, n):
    """tf.linspace(-1, 1, n)[i] in fp32 ([TF-sem 4]: start + step * i)."""
    step = np.float32(np.float32(2.0) / np.float32(n - 1))
    return np.float32(np.float32(-1.0) + step * np.float32(i))


def case_points(seed, n, k, h, w):
    rs = np.random.RandomState(seed)
    mu = rs.uniform(-1.4, 1.4, size=(n, k, 2)).astype(np.float32)
    # every third point of frame 0 sits exactly on a grid line in x, every fourth of the last frame in y; one point on a grid crossing
    for i in range(0, k, 3):
        mu[0, i, 0] = grid_line(rs.randint(0, w), w)
    for i in range(0, k, 4):
        mu[-1, i, 1] = grid_line(rs.randint(0, h), h)
    mu[0, 0] = (grid_line(w // 2, w), grid_line(h // 3, h))
    return mu


def stored_pixels(mu, n, h, w, seed):
    """Flat pixel indices kept for a case: every pixel of a small case; else each key-point's 5x5 neighbourhood and seeded samples."""
    if n * h * w <= FULL_MAX_PIXELS:
        return np.arange(n * h * w, dtype=np.int32)
    rs = np.random.RandomState(1000 + seed)
    keep = [rs.randint(0, h * w, size=SAMPLES_PER_FRAME) + f * h * w for f in range(n)]
    for f in range(n):
        for x, y in mu[f]:
            cx, cy = int(round((x + 1) / 2 * (w - 1))), int(round((y + 1) / 2 * (h - 1)))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if 0 <= cy + dy < h and 0 <= cx + dx < w:
                        keep.append(np.array([f * h * w + (cy + dy) * w + cx + dx]))
    return np.unique(np.concatenate(keep)).astype(np.int32)


def main():
    import torch
    import tf_standin as S
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    S.reset(seed=0)
    tf = S.install()
    spec = importlib.util.spec_from_file_location('_ref_model_utils', os.path.join(REF, 'utils', 'model.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for s, k in PALETTES:
        random.seed(s)
        out['palette_s%d_k%d' % (s, k)] = np.array(ref.get_n_colors(k), np.float64)
    out['palettes'] = np.array(PALETTES, np.int64)
    for tag, pseed, cseed, n, k, h, w in CASES:
        random.seed(cseed)
        colors = ref.get_n_colors(k)
        mu = case_points(pseed, n, k, h, w)
        maps = ref.colorize_point_maps(ref.get_gaussian_maps(mu, [h, w]), colors)
        sess = tf.Session()
        val = np.asarray(sess.run(maps), np.float32)
        assert val.shape == (n, h, w, 3), val.shape
        out['case_%s_mu' % tag] = mu
        out['case_%s_colors' % tag] = np.array(colors, np.float64)
        idx = stored_pixels(mu, n, h, w, pseed)
        out['case_%s_index' % tag] = idx
        out['case_%s_maps' % tag] = val.reshape(-1, 3)[idx]
        out['case_%s_dims' % tag] = np.array([pseed, cseed, n, k, h, w], np.int64)
    out['cases'] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, 'point_maps_ref.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
