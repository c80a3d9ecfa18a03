"""GPU: colourised key-point maps (kpx_point_maps_rgb_f32) against the reference's colorize_point_maps(get_gaussian_maps(..)) fixture, bit
for bit against the unfused GPU composition, on a side stream, inside FinalModel (eager, captured, replayed, re-captured after a restore)
and in evaluate.py's artefacts."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import restatement as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device('cuda:0')


def _palette(k, seed):
    from kpx_amd import model_utils
    return torch.tensor(model_utils.get_n_colors(k, rng=random.Random(seed)), dtype=torch.float32, device=DEV)


def _unfused(mu, h, w, colors):
    """(gaussian_maps[..., None] * colors).amax(-2): the reference's two steps with the repo's Gaussian-map kernel, in frame chunks."""
    from kpx_amd import ops
    outs = []
    for s in range(0, mu.shape[0], 256):
        maps = ops.gaussian_maps(mu[s:s + 256], h, w)
        outs.append((maps[..., None] * colors).amax(dim=-2))
        del maps
    return torch.cat(outs, 0)


def _points(n, k, h, w, seed):
    rs = np.random.RandomState(seed)
    mu = rs.uniform(-1.5, 1.5, size=(n, k, 2)).astype(np.float32)
    far = rs.rand(n, k) < 0.15                                     # far outside the frame: culled rows, all-zero frames
    mu[far] = rs.uniform(-4, 4, size=(int(far.sum()), 2)).astype(np.float32)
    lin_w = (np.float32(-1) + np.float32(np.float32(2) / np.float32(w - 1)) * np.arange(w, dtype=np.float32)).astype(np.float32)
    lin_h = (np.float32(-1) + np.float32(np.float32(2) / np.float32(h - 1)) * np.arange(h, dtype=np.float32)).astype(np.float32)
    on = rs.rand(n, k) < 0.2                                       # exactly on grid lines
    mu[..., 0][on] = lin_w[rs.randint(0, w, size=int(on.sum()))]
    mu[..., 1][on] = lin_h[rs.randint(0, h, size=int(on.sum()))]
    return torch.from_numpy(mu).to(DEV)


def test_render_point_maps_matches_the_reference_fixture():
    from kpx_amd import model_utils
    d = np.load(os.path.join(HERE, 'golden', 'point_maps_ref.npz'))
    for tag in d['cases']:
        _, _, n, k, h, w = (int(v) for v in d['case_%s_dims' % tag])
        colors = torch.from_numpy(d['case_%s_colors' % tag].astype(np.float32)).to(DEV)
        got = model_utils.render_point_maps(torch.from_numpy(d['case_%s_mu' % tag]).to(DEV), (h, w), colors).cpu().numpy()
        assert got.shape == (n, h, w, 3)
        idx = d['case_%s_index' % tag]                 # the fixture keeps every pixel of the small case, a sample of the large ones
        np.testing.assert_allclose(got.reshape(-1, 3)[idx], d['case_%s_maps' % tag], atol=2e-6, rtol=2e-5, err_msg=str(tag))


@pytest.mark.parametrize('n,k,h,w', [(2048, 15, 128, 128), (1, 1, 128, 128), (37, 3, 40, 70), (5, 40, 64, 130), (3, 64, 256, 256),
                                     (37, 15, 2, 2), (2, 64, 70, 2), (1, 40, 130, 70)])
def test_fused_maps_are_bitwise_the_unfused_composition(n, k, h, w):
    from kpx_amd import ops
    mu = _points(n, k, h, w, seed=n * 1000 + k * 10 + w)
    colors = _palette(k, seed=k)
    got = ops.point_maps_rgb(mu, h, w, colors)
    want = _unfused(mu, h, w, colors)
    assert got.shape == want.shape == (n, h, w, 3)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert float(got.max()) > 0


def test_launch_on_a_side_stream_gives_the_same_bits():
    from kpx_amd import model_utils
    mu = _points(64, 15, 128, 128, seed=3)
    colors = _palette(15, seed=0)
    ref = model_utils.render_point_maps(mu, (128, 128), colors)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got = model_utils.render_point_maps(mu, (128, 128), colors)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert torch.equal(got, ref)


def _checkpoint(k, res, cells, vdim, seed):
    arrays = {**R.init_variables(k, res=res, seed=seed), **R.init_stage2_decoder(k, cell_info=cells, vae_dim=vdim, seed=seed + 1)}
    return {n: a for n, a in arrays.items() if not n.startswith('img_discr')}


def test_final_model_point_maps_eager_captured_replayed_and_after_restore(tmp_path):
    """Three runs (eager, capture, replay), then a restore (drops the graph), an eager run and a re-capture: the point maps equal
    render_point_maps of the returned key-points bit for bit, and every other output equals a point_maps=False model's with the same
    weights and latents."""
    import kpx_amd
    import kpx_amd.final_model as fmod
    from kpx_amd import model_utils
    assert fmod.GRAPH
    res, k, b, cells, vdim = 32, 3, 2, (64, 64), 8
    cfg = {'model': {'n_pts': k, 'cell_info': list(cells), 'vae_dim': vdim, 'n_action': 9}, 'paths': {'log_dir': str(tmp_path)}}
    second = tmp_path / 'second.npz'
    np.savez(str(second), **{n.replace('/', '|'): a for n, a in _checkpoint(k, res, cells, vdim, 177).items()})
    rs = np.random.RandomState(13)
    feeds = []
    for i in range(5):
        im, _ = R.synthetic_pair(b, res=res, seed0=80 + i, seed1=90 + i)
        feeds.append(({'image': torch.from_numpy(im).to(DEV),
                       'action_code': torch.from_numpy(np.eye(9, dtype=np.float32)[rs.randint(0, 9, size=b)]).to(DEV)},
                      torch.from_numpy(rs.randn(b, vdim).astype(np.float32)).to(DEV)))
    runs = {}
    for pm in (False, True):
        fm = kpx_amd.FinalModel(cfg, device=DEV, image_size=res, frames_per_launch=32, point_maps=pm, colors_seed=5)
        fm.build()
        fm.store.load_numpy(_checkpoint(k, res, cells, vdim, 77), strict=True)
        assert fm.colors == model_utils.get_n_colors(k, rng=random.Random(5))
        runs[pm] = []
        for i, (feed, z) in enumerate(feeds):
            if i == 3:
                assert len(fm._graphs) == 1 and not fm._graph_failed          # captured at run 1, replayed at run 2
                fm.restore(None, str(second))
            o = fm.run(None, feed, z=z)
            runs[pm].append({key: v.clone() for key, v in o.items() if isinstance(v, torch.Tensor)})
            if pm:
                colors = torch.tensor(fm.colors, dtype=torch.float32, device=DEV)
                cur = model_utils.render_point_maps(o['first_pt'].reshape(b, k, 2), (res, res), colors)
                fut = model_utils.render_point_maps(o['fut_pt_raw'].reshape(-1, k, 2), (res, res), colors).reshape(b, 32, res, res, 3)
                assert torch.equal(o['current_points'], cur), i
                assert torch.equal(o['future_points'], fut), i
                assert float(o['future_points'].max()) > 0
        assert len(fm._graphs) == 1 and not fm._graph_failed              # re-captured at run 4
    for i in range(5):
        off, on = runs[False][i], runs[True][i]
        assert set(on) == set(off) | {'current_points', 'future_points'} and 'current_points' not in off
        for key in off:
            assert torch.equal(off[key], on[key]), (i, key)


def test_evaluate_writes_point_map_images(tmp_path):
    import yaml
    from PIL import Image
    import kpx_amd
    import evaluate
    cfg = {'paths': {'data_dir': str(tmp_path / 'none'), 'vggnet': None, 'log_dir': str(tmp_path / 'results')},
           'model': {'n_pts': 5, 'n_action': 9, 'cell_info': [32, 32], 'vae_dim': 8}}
    cfg_path = tmp_path / 'cfg.yaml'
    cfg_path.write_text(yaml.safe_dump(cfg))
    fm = kpx_amd.FinalModel(cfg, device=DEV)
    fm.build(None)
    fm.initialize_loggers(str(tmp_path / 'ckpt'))
    ckpt = fm.save_checkpoint(None, 0)
    base = ['--config', str(cfg_path), '--checkpoint_stage1', ckpt, '--checkpoint_stage2', ckpt, '--synthetic', '2', '--batch', '2']
    evaluate.main(base + ['--save_dir', str(tmp_path / 'eval'), '--colors_seed', '3'])
    for s in ('0000', '0001'):
        d = tmp_path / 'eval' / s
        cur = np.asarray(Image.open(str(d / 'current_points.png')))
        assert cur.shape == (128, 128, 3) and cur.dtype == np.uint8 and cur.max() > 0
        names = sorted(os.listdir(str(d / 'pred_points')))
        assert names == ['%06d.png' % i for i in range(32)]
        for nm in names:
            im = np.asarray(Image.open(str(d / 'pred_points' / nm)))
            assert im.shape == (128, 128, 3) and im.max() > 0, nm
        assert len(os.listdir(str(d / 'pred_seq'))) == 32 and (d / 'input_im.png').exists()
    evaluate.main(base + ['--save_dir', str(tmp_path / 'nosave'), '--no-save'])
    assert not (tmp_path / 'nosave').exists()                                  # --no-save writes nothing, point maps included
