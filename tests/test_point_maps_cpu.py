"""CPU: the key-point palette against the reference's get_n_colors (tests/golden/point_maps_ref.npz), and argument checks of the fused
colourised-map entry that return before any device call."""
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def test_palette_equals_the_reference_after_random_seed():
    from kpx_amd import model_utils
    d = np.load(os.path.join(HERE, 'golden', 'point_maps_ref.npz'))
    for s, k in d['palettes']:
        got = np.array(model_utils.get_n_colors(int(k), rng=random.Random(int(s))), np.float64)
        assert np.array_equal(got, d['palette_s%d_k%d' % (s, k)]), (s, k)
    # pastel_factor is ignored, as in the reference, and rng=None draws from the module-level random
    assert model_utils.get_n_colors(5, pastel_factor=0.0, rng=random.Random(0)) == model_utils.get_n_colors(5, rng=random.Random(0))
    random.seed(1)
    assert np.array_equal(np.array(model_utils.get_n_colors(40), np.float64), d['palette_s1_k40'])


def test_point_maps_entry_rejects_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                  # an aligned fake address: never dereferenced on these paths
    ok = dict(mu=a, n=2, k=15, h=128, w=128, inv_std=14.3, colors=a, out=a)

    def call(**kw):
        p = {**ok, **kw}
        return lib.kpx_point_maps_rgb_f32(p['mu'], p['n'], p['k'], p['h'], p['w'], p['inv_std'], p['colors'], p['out'], None)
    assert call(mu=None) == -1
    assert call(colors=None) == -1 and call(out=None) == -1
    assert call(n=0) == -1
    assert call(k=0) == -1 and call(k=65) == -1
    assert call(h=1) == -1 and call(h=1025) == -1
    assert call(w=1) == -1 and call(w=1025) == -1
    assert call(inv_std=0.0) == -1 and call(inv_std=-1.0) == -1 and call(inv_std=float('nan')) == -1


def test_point_maps_op_refuses_cpu_tensors():
    import pytest
    import torch
    from kpx_amd import ops
    from kpx_amd._lib import KpxError
    with pytest.raises(KpxError):
        ops.point_maps_rgb(torch.zeros(1, 3, 2), 8, 8, torch.ones(3, 3))
