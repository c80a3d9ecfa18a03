#!/usr/bin/env python3
"""Measure the colourised key-point maps (kpx_point_maps_rgb_f32, FinalModel(point_maps=True)) on one MI355X.

1. The kernel alone at the BASELINE configs[4] shape (N = 64 * 32 frames, 128x128, K = 15): device-event time of each launch, writing
   into outputs rotated over more than the 256 MB Infinity Cache; median us per launch, GB/s of the 12 B written per pixel and the
   fraction of the 8 TB/s HBM spec.
2. The configs[4] rollout (B = 64, replayed HIP graph) with point maps off and on: two FinalModels in one process, timed alternately;
   median ms per rollout of each and the difference.

    python bench_point_maps.py [--launches 40] [--rollouts 10]

Prints one JSON line.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_FRAMES, RES, K, B = 64 * 32, 128, 15, 64
HBM_SPEC = 8.0e12


def kernel_leg(dev, launches):
    from kpx_amd import model_utils, ops
    rs = np.random.RandomState(1)
    mu = torch.from_numpy(rs.uniform(-0.8, 0.8, size=(N_FRAMES, K, 2)).astype(np.float32)).to(dev)
    colors = torch.tensor(model_utils.get_n_colors(K, rng=random.Random(0)), dtype=torch.float32, device=dev)
    nbytes = N_FRAMES * RES * RES * 3 * 4
    outs = [torch.empty((N_FRAMES, RES, RES, 3), dtype=torch.float32, device=dev) for _ in range(-(-768 * 2 ** 20 // nbytes))]
    for o in outs:                                        # warm-up (code object load) and first touch of every output
        ops.point_maps_rgb(mu, RES, RES, colors, out=o)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        ops.point_maps_rgb(mu, RES, RES, colors, out=outs[i % len(outs)])
        e1.record()
    torch.cuda.synchronize(dev)
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    med = statistics.median(us)
    return {'shape': [N_FRAMES, RES, RES, K], 'outputs_rotated': len(outs), 'output_mb': round(nbytes / 2 ** 20, 1), 'launches': launches,
            'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
            'gb_per_s': round(nbytes / (med * 1e-6) / 1e9, 1), 'frac_of_8tbs': round(nbytes / (med * 1e-6) / HBM_SPEC, 3)}


def rollout_leg(dev, rollouts):
    import kpx_amd
    cfg = {'model': {'n_pts': K, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    rs = np.random.RandomState(7)
    im = torch.from_numpy((rs.randint(0, 256, size=(B, RES, RES, 3)).astype(np.float32) / 255.0 * 2 - 1).astype(np.float32)).to(dev)
    act = torch.from_numpy(np.eye(9, dtype=np.float32)[rs.randint(0, 9, size=B)]).to(dev)
    z = torch.from_numpy(rs.randn(B, 64).astype(np.float32)).to(dev)
    feed = {'image': im, 'action_code': act}
    models = {}
    for pm in (False, True):
        fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256, point_maps=pm)
        fm.build()
        for _ in range(3):                                # eager, capture, one replay
            fm.run(None, feed, z=z)
        models[pm] = fm
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for pm in (False, True):
            t0 = time.perf_counter()
            out = models[pm].run(None, feed, z=z)
            torch.cuda.synchronize(dev)
            ms[pm].append((time.perf_counter() - t0) * 1e3)
    assert tuple(out['future_points'].shape) == (B, 32, RES, RES, 3) and bool(torch.isfinite(out['future_points']).all())
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'rollouts_each': rollouts, 'graph_replay': all(len(m._graphs) == 1 for m in models.values()),
            'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'delta_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rollouts', type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_point_maps.py needs the MI355X')
    dev = torch.device('cuda:0')
    res = {'kernel': kernel_leg(dev, args.launches)}
    torch.cuda.empty_cache()
    res['rollout_c4'] = rollout_leg(dev, args.rollouts)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
