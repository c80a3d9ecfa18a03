#!/usr/bin/env python3
"""Measure the frame metrics (kpx_frame_metrics_f32, evaluate.py --metrics) on one MI355X.

1. The kernel alone on the BASELINE configs[4] batch (2 048 frame pairs of 128x128x3, the png8 form evaluate.py runs, and the plain fp32
   form): device-event time of each launch after warm-up; median us, effective bytes/s of the two inputs (805 MB, more than the 256 MB
   Infinity Cache) read once, and its fraction of the 6.29 TB/s measured copy rate.
2. The configs[4] rollout (B = 64, replayed HIP graph) without and with scoring its 2 048 predicted frames against real frames, alternated in
   one process; median ms of each and the overhead in %.

    python bench_metrics.py [--launches 40] [--rollouts 10] [--vgg | --motion]

``--vgg`` measures the VGG feature-space metrics (kpx_feature_pair_metrics_f32, evaluate.py --vgg-metrics) instead:

3. The kernel alone on the five VGG19 feature shapes of 512 frame pairs at 128x128 (conv1_2 [512,128,128,64] ... conv5_4 [512,8,8,512]):
   device-event time of each call (its two launches) after warm-up; median us, bytes/s of the two inputs read once, and the fraction of the
   copy rate.
4. The configs[4] rollout without and with scoring its 2 048 predicted frames through vgg.FeatureScorer (He-normal VGG19 weights, the
   real frames' features computed once before the timed loop, as evaluate.py reuses them across draws), alternated in one process.

``--motion`` measures the motion metrics (evaluate.py --motion-metrics) instead:

5. The two pixel kernels alone at the configs[4] size (2 048 frames of 128x128x3 = 100.7 M values, D = 4): kpx_draw_moments_add_f32 (per
   value 4 bytes of the frame and two uint32 accumulators read and written: 20 bytes) and kpx_draw_diversity_f32 with the spread map (the two
   accumulators read: 8 bytes); device-event time of each launch after warm-up, median us, bytes/s and the fraction of the copy rate.
6. Four configs[4] rollouts (the draws of one batch) without and with what --motion-metrics adds -- per rollout the key-point copy and the
   accumulator update, per batch the zeroing, kpx_keypoint_draw_metrics_f32 and kpx_draw_diversity_f32 --, alternated in one process;
   median ms per rollout of each and the overhead in %.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_FRAMES, RES, B = 64 * 32, 128, 64
COPY_RATE = 6.29e12                  # measured float4 copy rate of the MI355X (MI355X_MICROARCH: HBM)


def kernel_leg(dev, launches, png8):
    from kpx_amd import ops
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.rand((N_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1
    b = torch.rand((N_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1
    out = torch.empty((N_FRAMES, 3), dtype=torch.float32, device=dev)
    for _ in range(3):
        ops.frame_metrics(a, b, png8=png8, out=out)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        ops.frame_metrics(a, b, png8=png8, out=out)
        e1.record()
    torch.cuda.synchronize(dev)
    us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    med = statistics.median(us)
    nbytes = 2 * a.numel() * 4
    assert bool(torch.isfinite(out).all())
    return {'shape': [N_FRAMES, RES, RES, 3], 'png8': png8, 'input_mb': round(nbytes / 1e6, 1), 'launches': launches,
            'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
            'gb_per_s': round(nbytes / (med * 1e-6) / 1e9, 1), 'frac_of_copy_rate': round(nbytes / (med * 1e-6) / COPY_RATE, 3)}


def rollout_leg(dev, rollouts):
    import kpx_amd
    from kpx_amd import ops
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    real = torch.rand((N_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1
    out = torch.empty((N_FRAMES, 3), dtype=torch.float32, device=dev)
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    for _ in range(3):                                    # eager, capture, one replay
        o = fm.run(None, feed, z=z)
    ops.frame_metrics(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), real, png8=True, out=out)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            o = fm.run(None, feed, z=z)
            if score:
                ops.frame_metrics(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), real, png8=True, out=out)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'frames': N_FRAMES, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 1,
            'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'overhead_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


VGG_PAIRS = 512
VGG_SHAPES = [('conv1_2', RES, 64), ('conv2_2', RES // 2, 128), ('conv3_4', RES // 4, 256), ('conv4_4', RES // 8, 512), ('conv5_4', RES // 16, 512)]


def vgg_kernel_leg(dev, launches):
    from kpx_amd import ops
    res = []
    for name, hw, c in VGG_SHAPES:
        g = torch.Generator(device=dev).manual_seed(2)
        a = torch.randn((VGG_PAIRS, hw, hw, c), generator=g, device=dev).relu_()
        b = torch.randn((VGG_PAIRS, hw, hw, c), generator=g, device=dev).relu_()
        out = torch.empty((VGG_PAIRS, 2), dtype=torch.float32, device=dev)
        for _ in range(3):
            ops.feature_pair_metrics(a, b, out=out)
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for e0, e1 in ev:
            e0.record()
            ops.feature_pair_metrics(a, b, out=out)
            e1.record()
        torch.cuda.synchronize(dev)
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        med = statistics.median(us)
        nbytes = 2 * a.numel() * 4
        assert bool(torch.isfinite(out).all())
        res.append({'layer': name, 'shape': [VGG_PAIRS, hw, hw, c], 'input_mb': round(nbytes / 1e6, 1), 'launches': launches,
                    'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                    'gb_per_s': round(nbytes / (med * 1e-6) / 1e9, 1), 'frac_of_copy_rate': round(nbytes / (med * 1e-6) / COPY_RATE, 3)})
        del a, b
        torch.cuda.empty_cache()
    return res


def vgg_rollout_leg(dev, rollouts):
    import kpx_amd
    from kpx_amd import vgg as V
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    real = torch.rand((N_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1
    out = torch.empty((N_FRAMES, len(V.FEATURE_LAYERS), 2), dtype=torch.float32, device=dev)
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    net = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(), device=dev)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    scorer = V.FeatureScorer(net, real)
    torch.cuda.synchronize(dev)
    real_ms = (time.perf_counter() - t0) * 1e3                # the first VGG forwards: includes what the first use of each kernel costs
    for _ in range(3):                                        # eager, capture, one replay
        o = fm.run(None, feed, z=z)
    scorer(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), out=out)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            o = fm.run(None, feed, z=z)
            if score:
                scorer(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), out=out)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(out).all())
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'frames': N_FRAMES, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 1, 'feature_chunk': scorer.chunk,
            'real_features_gb': round(sum(f.numel() * 4 for c in scorer.real for f in c) / 1e9, 2), 'real_features_first_ms': round(real_ms, 1),
            'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'overhead_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


MOTION_DRAWS = 4


def _event_times(fn, launches, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize(dev)
    return [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]


def motion_kernel_leg(dev, launches):
    from kpx_amd import ops
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.rand((N_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1
    acc = torch.zeros((2, x.numel()), dtype=torch.int32, device=dev)
    div_mse = torch.empty((N_FRAMES,), dtype=torch.float32, device=dev)
    std_map = torch.empty((N_FRAMES, RES, RES), dtype=torch.uint8, device=dev)
    res = {}
    draws = [torch.rand((N_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1 for _ in range(MOTION_DRAWS - 1)] + [x]

    def four_draws():                                     # the timed adds left 3 + launches draws behind (far below the 4096 that fit)
        ops.fill_raw_(acc, 0.0)
        for d in draws:
            ops.draw_moments_add(d, acc[0], acc[1])

    for name, per_value, setup, fn in (('draw_moments_add', 20, None, lambda: ops.draw_moments_add(x, acc[0], acc[1])),
                                       ('draw_diversity', 8, four_draws, lambda: ops.draw_diversity(acc[0], acc[1], MOTION_DRAWS, (RES, RES, 3),
                                                                                                    std_map=std_map, out=div_mse))):
        if setup is not None:
            setup()
        us = _event_times(fn, launches, dev)
        med = statistics.median(us)
        nbytes = per_value * x.numel()
        res[name] = {'shape': [N_FRAMES, RES, RES, 3], 'draws': MOTION_DRAWS, 'bytes_per_value': per_value, 'mb': round(nbytes / 1e6, 1),
                     'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                     'gb_per_s': round(nbytes / (med * 1e-6) / 1e9, 1), 'frac_of_copy_rate': round(nbytes / (med * 1e-6) / COPY_RATE, 3)}
    assert bool(torch.isfinite(div_mse).all()) and float(div_mse.min()) > 0
    return res


def motion_rollout_leg(dev, rollouts):
    import kpx_amd
    from kpx_amd import ops
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    zs = [torch.randn((B, 64), generator=g, device=dev) for _ in range(MOTION_DRAWS)]
    kp_real = torch.rand((B, 32, 15, 2), generator=g, device=dev) * 1.6 - 0.8
    kp_pred = torch.empty((MOTION_DRAWS, B, 32, 15, 2), dtype=torch.float32, device=dev)
    acc = torch.empty((2, N_FRAMES * RES * RES * 3), dtype=torch.int32, device=dev)
    kp_l2 = torch.empty((MOTION_DRAWS, B, 32), dtype=torch.float32, device=dev)
    kp_div = torch.empty((B, 32), dtype=torch.float32, device=dev)
    div_mse = torch.empty((N_FRAMES,), dtype=torch.float32, device=dev)
    std_map = torch.empty((N_FRAMES, RES, RES), dtype=torch.uint8, device=dev)
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()

    def batch(score):
        if score:
            ops.fill_raw_(acc, 0.0)
        for d, z in enumerate(zs):
            o = fm.run(None, feed, z=z)
            if score:
                ops.flat_copy_tensor(o['fut_pt_raw'].contiguous(), kp_pred[d].data_ptr())
                ops.draw_moments_add(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), acc[0], acc[1])
        if score:
            ops.keypoint_draw_metrics(kp_pred, kp_real, out=(kp_l2, kp_div))
            ops.draw_diversity(acc[0], acc[1], MOTION_DRAWS, (RES, RES, 3), std_map=std_map, out=div_mse)

    for _ in range(3):                                    # eager, capture, one replay
        fm.run(None, feed, z=zs[0])
    batch(True)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            batch(score)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3 / MOTION_DRAWS)
    assert bool(torch.isfinite(div_mse).all()) and bool(torch.isfinite(kp_l2).all()) and bool(torch.isfinite(kp_div).all())
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'frames': N_FRAMES, 'draws': MOTION_DRAWS, 'batches_each': rollouts, 'graph_replay': len(fm._graphs) == 1,
            'off_ms_per_rollout': round(off, 3), 'on_ms_per_rollout': round(on, 3), 'delta_ms_per_rollout': round(on - off, 3),
            'overhead_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rollouts', type=int, default=10)
    ap.add_argument('--vgg', action='store_true', help='measure the VGG feature-space metrics instead of the frame metrics')
    ap.add_argument('--motion', action='store_true', help='measure the motion metrics (draw diversity, key-point error) instead')
    args = ap.parse_args()
    if args.vgg and args.motion:
        ap.error('--vgg and --motion are two measurements: pass one')
    if not torch.cuda.is_available():
        raise SystemExit('bench_metrics.py needs the MI355X')
    dev = torch.device('cuda:0')
    if args.vgg:
        res = {'vgg_kernel': vgg_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['vgg_rollout_c4'] = vgg_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.motion:
        res = {'motion_kernels': motion_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['motion_rollout_c4'] = motion_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    res = {'kernel_png8': kernel_leg(dev, args.launches, True), 'kernel_f32': kernel_leg(dev, args.launches, False)}
    torch.cuda.empty_cache()
    res['rollout_c4'] = rollout_leg(dev, args.rollouts)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
