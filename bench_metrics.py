#!/usr/bin/env python3
"""Measure the frame metrics (kpx_frame_metrics_f32, evaluate.py --metrics) on one MI355X.

1. The kernel alone on the BASELINE configs[4] batch (2 048 frame pairs of 128x128x3, the png8 form evaluate.py runs, and the plain fp32
   form): device-event time of each launch after warm-up; median us, effective bytes/s of the two inputs (805 MB, more than the 256 MB
   Infinity Cache) read once, and its fraction of the 6.29 TB/s measured copy rate.
2. The configs[4] rollout (B = 64, replayed HIP graph) without and with scoring its 2 048 predicted frames against real frames, alternated in
   one process; median ms of each and the overhead in %.

    python bench_metrics.py [--launches 40] [--rollouts 10] [--vgg | --motion | --actions | --drive | --frechet | --classifier | --stability | --joints | --gif | --animate | --guard | --ema | --video]

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

``--actions`` measures the class sweep (evaluate.py --actions) instead:

7. kpx_sheet_paste_u8_f32 alone at the configs[4] size (B = 64 rollouts of 32 frames of 128x128x3, J = 8 frames into one row of a sheet of
   10 x 9 cells): per pixel 12 bytes read and 3 written; device-event time of each launch after warm-up, the launches walking over the four
   groups of 8 frames and the 10 rows (the 403 MB of frames and the 283 MB sheet do not stay in the 256 MB Infinity Cache); median us,
   bytes/s and the fraction of the copy rate, beside kpx_draw_moments_add_f32 (the sibling stream) measured in the same process.  Then the
   route the kernel replaces, in the same run: the same 8 frames of every sample gathered and copied to the host as fp32, quantised and
   pasted with numpy, against the paste on the device plus the copy of the strip's bytes; wall-clock ms of each, medians of 5.
8. A configs[4] sweep -- the batch's own rollout and one per class, 9 classes, at one z -- without what --actions adds, with its scores
   alone (--no-save: the key-point copies, accumulator updates and score launches) and with the sheets too: the pastes of both sheets and
   their two copies into page-locked host memory (not the PNG encoding, which is host work after the device is idle); the three alternated
   in one process; median ms per rollout of each and the overheads in %; the two copies alone, page-locked and pageable.

``--drive`` measures the driven rollout (FinalModel.run(drive=...), evaluate.py --drive) instead:

9. kpx_points_retarget_f32 alone at the configs[4] size (B = 64, T = 32, K = 15: 61 440 values, 240 KB out) in its four modes, shift 1:
   device-event time of each launch after warm-up; median, minimum and maximum us.  It is a launch-bound call: no rate is quoted.
10. The configs[4] rollout (B = 64, replayed HIP graphs) as the model's own rollout and as a driven rollout of each mode -- labels
   (absolute, shift 0), hold, transfer (relative, shift 1) and transfer scaled --, the five alternated in one process; median ms per rollout
   of each and the difference to the model's own in ms and %.

``--frechet`` measures the Fréchet distance's device passes (evaluate.py --frechet) instead:

11. kpx_feature_pool_f64 alone on the five VGG19 feature shapes of 512 frames at 128x128: device-event time of each call (its two launches)
   after warm-up; median us, bytes/s of the one input read once and the fraction of the copy rate, beside a float4 device copy of the same
   tensor (read + write bytes) and beside kpx_feature_pair_metrics_f32 on the same shape (two inputs), all in this process.
12. kpx_moments_add_f64 alone: M = 2 048 rows (the frames of a configs[4] rollout) at D = 64, 128, 256, 512 and M = 64 rows (its rollouts) at
   D = 1024; median, minimum and maximum us and the fp64 GFLOP/s (2 M D^2).
13. The configs[4] rollout scored through vgg.FeatureScorer without and with the accumulators (frechet=: pooling, both levels' moments, into
   the two accumulators of draw 0), alternated in one process beside the bare rollout; median ms of each, the cost of --frechet on top of
   --vgg-metrics in ms and %.

``--stability`` measures the detector's equivariance score (make_pseudo_labels.py --stability) instead:

14. kpx_affine_warp_f32 alone at [128 frames x 4 maps, 128, 128, 3] (per output row about a frame read and a frame written: 201 MB, which
   fits the 256 MB Infinity Cache) beside a float4 device copy of the same bytes in the same process; median us, bytes/s and the fraction
   of the copy.  kpx_equivariance_scores_f32 alone at K = 40 on the 1 326 rows of a 663-frame video at W = 2: a launch-bound call.
15. A 663-frame video through KeypointModel.run (K = 40) without and with stability() at W = 2, alternated in one process; the warp of its
   1 326 warped frames alone beside the detector on them.

``--joints`` measures the landmark regression (make_pseudo_labels.py --joints) instead:

16. kpx_joint_targets_f32, kpx_joint_moments_add_f64 and kpx_joint_scores_f32 alone on the F = 663 frames of a video with J = 13 joints,
   at K = 15 and at K = 40, each beside a device copy of the bytes the launch reads and writes in the same process; median, minimum and
   maximum us.  All three are launch-bound at these sizes: no rate is quoted.
17. A 663-frame video through KeypointModel.run (K = 40) without and with JointRegression.add for a train video (targets and moments, the
   labels already read), alternated in one process, and JointRegression.finish (the host solve and one scores launch per video) over the
   videos added, per video.

``--gif`` measures the animated GIFs of rollouts (evaluate.py --gif) instead:

18. kpx_color_hist_add_u32 and kpx_palette_map_u8 alone on the compare.gif canvases of a configs[4] batch (64 samples of 33 frames of
   128 x 384 pixels: 311 MB of RGB, 104 MB of indices; two smooth image columns and a mostly black key-point column), the histogram also on
   a canvas of uniform noise (no two neighbours share a cell), each beside a device copy of the canvas in the same process; device-event
   time of each launch after warm-up, median us and the ratio to the copy; the map kernel's candidate evaluations per second.  Then, for 4
   samples, the host route the kernels replace (the frames copied to the host as fp32, quantised there, PIL ``quantize`` per frame) against
   ``ops.gif_indices`` plus the copy of the indices, wall-clock ms per sample; and the LZW of one sample's 33 frames in the library's host
   code against the pure-Python encoder of tests/gif_ref.py.
19. The configs[4] rollout without and with what --gif adds (``kpx_amd.gif.RolloutGifs.write``: both canvases composed, quantised, copied
   and written as 128 GIF files), alternated in one process; ms per rollout of each, and the flag's cost split into the device part (through
   the copy of the indices) and the host part (median cut, LZW, files).

``--animate`` measures the animated grids of stills (animate.py) instead:

20. kpx_cell_frames_u8_f32 alone on a 64-still batch (frame 0 and 32 predicted frames of 128 x 128 x 3 into one cell: 415 MB of fp32 in,
   104 MB out) without markers and with 15 key points at radius 3, beside a device copy of the frames in the same process, and the route
   the kernel replaces without markers (``RolloutGifs._canvas``: a staging stack, two copies and kpx_sheet_paste_u8_f32); device-event
   time after warm-up, median us, GB/s of the bytes each moves and the kernel's rate as a fraction of the copy's.
21. animate.py's loop for 8 stills under 9 classes x 1 draw with --overlay 3 (random weights): the rollouts alone, with both grids
   composed, quantised and copied, and with the host GIF work (LZW, 16 files); ms per still of each part.

``--guard`` measures the step guard (train.py --guard) instead:

22. kpx_grad_health_f32 (its two launches), kpx_adam_tf_flat_guarded_f32 beside kpx_adam_tf_flat_dev_alpha_f32, and kpx_guard_restore_f32
   on a dirty record, on the two flat buckets of the configs[1] model (their real sizes, read from a built model), each beside a device copy
   of the same number of floats in the same process; device-event time of each call after warm-up, median us, bytes/s of what each moves
   (health 4n read; Adam 16n read + 12n written; copy and restore 4n + 4n) and the rate as a fraction of the copy's.
23. The configs[1] train step (128x128, K = 15, B = 32, replayed HIP graph) through the model API with guard off and on, two models in one
   process, alternated in blocks; median ms per step of each and the difference in ms and %.

``--ema`` measures the averaged generator (train.py --ema) instead:

24. kpx_ema_flat_f32 (without a health record and with a clean one) and kpx_swap_flat_f32 on the 'G' bucket of the configs[1] model (its real
   size, read from a built model), beside a device copy of the same number of floats in the same process; device-event time of each call
   after warm-up, median us, bytes/s of what each moves (the average 8n read + 4n written; the swap 8n + 8n; the copy 4n + 4n) and the rate
   as a fraction of the copy's.
25. The configs[1] train step through the model API with ema off and on (ema=0.999), two models in one process, alternated in blocks; median
   ms per step of each and the difference in ms and %.

``--novelty`` measures the nearest-motion search (evaluate.py --novelty) instead:

26. kpx_seq_nearest_f32 (its two launches) on a synthetic store of Penn's size -- 1 171 videos, lengths drawn from 18..663, K = 40, 9 classes,
   mirror images searched -- for Q = 64 and Q = 1 024 queries; device-event time of each call after warm-up, min / median / max ms, and the
   fp64 fmas per second of 4 fmas per point, candidate window and query.  Beside it, in the same process: (a) a device copy of the store's label
   buffer; (b) the route the kernel replaces on the same device: every window gathered with ``MotionStore.gather`` (kpx_keypoint_seq_augment_f32)
   and the distances formed in torch in fp64, in chunks, with a per-class ``amin`` (the distances alone: no argmin, no exclusion), whose
   result is compared with the kernel's.
27. The rollout of configs[4] (B = 64, replayed HIP graph) at n_pts = 40 without and with what --novelty adds per batch and draw (the copy of
   the draw's key points and one search of the 64 real futures and 64 rollouts), alternated; median ms of each and the difference.

``--long`` measures the longer and smoother rollouts (FinalModel.run(frames=, rate=), evaluate.py / animate.py --frames --rate) instead:

28. kpx_points_resample_f32 (linear and cubic) and kpx_points_speed_f64 at B = 64, N = 96, F = 4 for K = 15 and K = 40; device-event time of
   each launch after warm-up, min / median / max us, beside a device copy of the resampler's output (B x 384 x K x 2 floats) in the same process.
29. The rollout of configs[4] (B = 64, replayed HIP graphs) in one process, alternated: frames = 96 beside three 32-frame rollouts, and
   frames = 32, rate = 4 beside four 32-frame rollouts; median ms of each and the quotient.

``--prdc`` measures precision / recall / density / coverage (evaluate.py --prdc) instead:

30. ``ops.prdc`` (four calls of kpx_set_neighbours_f64, two launches each) on a synthetic store of Penn's test-set size -- n = 1 024 real rows,
   m = 4 096 generated rows (four draws), k = 5, clustered rows of D = 2 560 (key-point space at K = 40) and D = 256 (the recogniser's features)
   -- device-event time of the whole call and of each of its four searches after warm-up, min / median / max ms, and the fp64 fmas per second of
   one fma per value, query and reference (the subtractions are not counted).  Beside it, in the same process: (a) a device copy of the rows;
   (b) the route this replaces on the same device: ``torch.cdist`` in fp64 + ``topk`` + comparisons, once in cdist's default mode (which forms
   |a|^2 + |b|^2 - 2ab on the matrix pipe at these sizes) and once with ``donot_use_mm_for_euclid_dist`` (direct differences); whether the four
   scores of each route equal the kernel's is reported, not asserted.
31. The rollout of configs[4] (B = 64, replayed HIP graph) at n_pts = 40 without and with what --prdc adds per batch and draw (the float32 copy
   of the draw's key points; the scores are computed once, after the last batch: item 30), alternated; median ms of each and the difference.

``--video`` measures the Motion-JPEG AVIs of rollouts (evaluate.py --video) instead:

32. kpx_jpeg_encode_u8 alone on the pred and compare canvases of a configs[4] batch (64 samples of 33 frames of 128 x 128 and 128 x 384,
   quality 90), in the chunks ``ops.jpeg_encode`` uses: device-event time of all chunks after warm-up, min / median / max ms, beside a device
   copy of the same canvases; the compressed bytes against the 8-bit RGB bytes.  Then the two routes to JPEG bytes on the host for the same
   samples, wall-clock ms per sample: ``ops.jpeg_encode`` (kernels, one read of the offsets and one copy of the used bytes per chunk) against
   the uint8 canvas copied to the host and ``PIL.Image.save(..., 'JPEG', quality=90, subsampling=2)`` per frame on 16 threads.
33. The configs[4] rollout without anything, with what --gif adds and with what --video adds (``kpx_amd.mjpeg.RolloutVideos.write``: both
   canvases composed, coded, copied and written as 128 AVI files), alternated in one process; ms per rollout and per sample of each.

``--posterior`` measures the posterior tools (evaluate.py --posterior) instead:

34. kpx_latent_stats_add_f64 (B = 64, V = 64, nine groups, kl_rows), kpx_latent_sample_f32 and kpx_latent_path_f32 (eight slerp steps): device-event
   time of each launch after warm-up, min / median / max us, beside a device copy of the logit rows (32 KB) in the same process.  All three are
   launch-latency-bound at these sizes; the statistics launch is one workgroup by design (determinism).
35. ``FinalModel.encode`` at B = 64, K = 40 (replayed HIP graph), wall-clock ms, and the rollout of configs[4] at n_pts = 40 without and with what
   --posterior adds per batch (encode, latent_stats_add, the copy of the rows, z = mu, one more rollout), alternated; median ms of each and the
   quotient.  The flag adds one rollout: roughly 2 is expected, and there is no target.

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


def frechet_kernel_leg(dev, launches):
    from kpx_amd import ops
    pool, moments = [], []
    for name, hw, c in VGG_SHAPES:
        g = torch.Generator(device=dev).manual_seed(2)
        a = torch.randn((VGG_PAIRS, hw, hw, c), generator=g, device=dev).relu_()
        b = torch.randn((VGG_PAIRS, hw, hw, c), generator=g, device=dev).relu_()
        out = torch.empty((VGG_PAIRS, c), dtype=torch.float64, device=dev)
        pair_out = torch.empty((VGG_PAIRS, 2), dtype=torch.float32, device=dev)
        nbytes = a.numel() * 4
        row = {'layer': name, 'shape': [VGG_PAIRS, hw, hw, c], 'input_mb': round(nbytes / 1e6, 1), 'launches': launches,
               'workspace_mb': round(ops.lib.kpx_feature_pool_workspace_bytes(VGG_PAIRS, hw, hw, c) / 1e6, 2)}
        for key, moved, fn in (('pool', nbytes, lambda: ops.feature_pool(a, out=out)), ('copy', 2 * nbytes, lambda: b.copy_(a)),
                               ('pair', 2 * nbytes, lambda: ops.feature_pair_metrics(a, b, out=pair_out))):
            us = _event_times(fn, launches, dev)
            med = statistics.median(us)
            row[key] = {'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                        'gb_per_s': round(moved / (med * 1e-6) / 1e9, 1), 'frac_of_copy_rate': round(moved / (med * 1e-6) / COPY_RATE, 3)}
        assert bool(torch.isfinite(out).all())
        pool.append(row)
        del a, b
        torch.cuda.empty_cache()
    for m, d in ((N_FRAMES, 64), (N_FRAMES, 128), (N_FRAMES, 256), (N_FRAMES, 512), (B, 1024)):
        g = torch.Generator(device=dev).manual_seed(3)
        x = torch.randn((m, d), generator=g, device=dev, dtype=torch.float64)
        s, o = torch.zeros((d,), dtype=torch.float64, device=dev), torch.zeros((d, d), dtype=torch.float64, device=dev)
        us = _event_times(lambda: ops.moments_add(x, s, o), launches, dev)
        med = statistics.median(us)
        assert bool(torch.isfinite(o).all())
        moments.append({'M': m, 'D': d, 'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                        'fp64_gflops': round(2.0 * m * d * d / (med * 1e-6) / 1e9, 1)})
    return {'feature_pool': pool, 'moments_add': moments}


def frechet_rollout_leg(dev, rollouts):
    import kpx_amd
    from kpx_amd import frechet as K, vgg as V
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
    dims = [int(net.params[name][0].shape[3]) for name in V.FEATURE_LAYERS]
    accs = [K.FrechetAccumulator(dims, dev) for _ in range(4)]
    scorer = V.FeatureScorer(net, real, frechet=K.FrechetSplit(accs[:2]), frames_per_video=32)
    for _ in range(3):                                        # eager, capture, one replay
        o = fm.run(None, feed, z=z)
    scorer(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), out=out, frechet=accs[2:])
    torch.cuda.synchronize(dev)
    modes = ('rollout', 'vgg', 'vgg_frechet')
    ms = {m: [] for m in modes}
    for _ in range(rollouts):
        for m in modes:
            t0 = time.perf_counter()
            o = fm.run(None, feed, z=z)
            if m != 'rollout':
                scorer(o['pred_im_seq'].reshape(N_FRAMES, RES, RES, 3), out=out, frechet=accs[2:] if m == 'vgg_frechet' else None)
            torch.cuda.synchronize(dev)
            ms[m].append((time.perf_counter() - t0) * 1e3)
    stats = accs[2].stats()
    assert all(s['n'] == N_FRAMES * (1 + rollouts) for s in stats['frame']) and all(s['n'] == B * (1 + rollouts) for s in stats['video'])
    bare, vgg, both = (statistics.median(ms[m]) for m in modes)
    return {'batch': B, 'frames': N_FRAMES, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 1, 'accumulators_per_call': 2,
            'rollout_ms': round(bare, 3), 'vgg_ms': round(vgg, 3), 'vgg_frechet_ms': round(both, 3), 'delta_ms': round(both - vgg, 3),
            'overhead_on_vgg_pct': round(100 * (both - vgg) / vgg, 2), 'overhead_on_rollout_pct': round(100 * (both - vgg) / bare, 2),
            'rollout_ms_all': [round(v, 2) for v in ms['rollout']], 'vgg_ms_all': [round(v, 2) for v in ms['vgg']],
            'vgg_frechet_ms_all': [round(v, 2) for v in ms['vgg_frechet']]}


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


ACTION_CLASSES = 9
SHEET_FRAMES = [3, 7, 11, 15, 19, 23, 27, 31]


def actions_kernel_leg(dev, launches):
    import numpy as np
    from kpx_amd import ops
    g = torch.Generator(device=dev).manual_seed(4)
    j, rows, cols = len(SHEET_FRAMES), 1 + ACTION_CLASSES, 1 + len(SHEET_FRAMES)
    src = torch.rand((B, 32, RES, RES, 3), generator=g, device=dev) * 2 - 1
    canvas = torch.zeros((B, rows * RES, cols * RES, 3), dtype=torch.uint8, device=dev)
    turn = [0]

    def paste():                                          # another group of 8 frames and another row each launch: nothing stays cached
        t = turn[0] = turn[0] + 1
        ops.sheet_paste(canvas, src, list(range(8 * (t % 4), 8 * (t % 4) + j)), t % rows, 1, 'unit')

    us = _event_times(paste, launches, dev)
    med = statistics.median(us)
    pixels = B * j * RES * RES
    nbytes = pixels * (12 + 3)
    res = {'sheet_paste': {'src': list(src.shape), 'sheet_cells': [rows, cols], 'frames_per_launch': j, 'bytes_per_pixel': [12, 3],
                           'mb': round(nbytes / 1e6, 1), 'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1),
                           'max_us': round(max(us), 1), 'gb_per_s': round(nbytes / (med * 1e-6) / 1e9, 1),
                           'frac_of_copy_rate': round(nbytes / (med * 1e-6) / COPY_RATE, 3)}}
    # the route the kernel replaces: the same frames to the host as fp32, quantised and pasted there -- against paste + copy of the bytes
    strip = torch.zeros((B, RES, j * RES, 3), dtype=torch.uint8, device=dev)
    idx = torch.tensor(SHEET_FRAMES, device=dev)
    host_canvas = np.zeros((B, RES, j * RES, 3), np.uint8)

    def host_route():
        x = src.index_select(1, idx).cpu().numpy()
        for k in range(j):
            host_canvas[:, :, k * RES:(k + 1) * RES] = ((0.5 * (x[:, k] + 1.0)) * 255).astype(np.uint8)
        return host_canvas

    def device_route():
        ops.sheet_paste(strip, src, SHEET_FRAMES, 0, 0, 'unit')
        return strip.cpu().numpy()

    ms = {'host': [], 'device': []}
    same = None
    for _ in range(6):                                    # the first pair warms both routes up and is dropped
        for name, fn in (('host', host_route), ('device', device_route)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            if name == 'host':
                same = out.copy()
            else:
                same = bool((same == out).all())          # values in [-1, 1): the two routes write the same bytes
    host_ms, dev_ms = statistics.median(ms['host'][1:]), statistics.median(ms['device'][1:])
    res['route'] = {'frames': [B, j, RES, RES, 3], 'fp32_to_host_mb': round(pixels * 12 / 1e6, 1), 'bytes_to_host_mb': round(pixels * 3 / 1e6, 1),
                    'host_route_ms': round(host_ms, 2), 'device_route_ms': round(dev_ms, 2), 'host_over_device': round(host_ms / dev_ms, 2),
                    'same_bytes': same, 'host_ms_all': [round(v, 2) for v in ms['host'][1:]], 'device_ms_all': [round(v, 2) for v in ms['device'][1:]]}
    del src, canvas, strip
    torch.cuda.empty_cache()
    res['draw_moments_add'] = motion_kernel_leg(dev, launches)['draw_moments_add']
    return res


def actions_rollout_leg(dev, batches):
    import kpx_amd
    from kpx_amd import ops
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    a_n, cols = ACTION_CLASSES, 1 + len(SHEET_FRAMES)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    codes = [torch.eye(9, device=dev)[a:a + 1].expand(B, -1).contiguous() for a in range(a_n)]
    z = torch.randn((B, 64), generator=g, device=dev)
    real = torch.rand((B, 32, RES, RES, 3), generator=g, device=dev) * 2 - 1
    kp_real = torch.rand((B, 32, 15, 2), generator=g, device=dev) * 1.6 - 0.8
    kp = torch.empty((1, a_n, B, 32, 15, 2), dtype=torch.float32, device=dev)
    acc = torch.empty((2, N_FRAMES * RES * RES * 3), dtype=torch.int32, device=dev)
    classes = torch.empty((B, (1 + a_n) * RES, cols * RES, 3), dtype=torch.uint8, device=dev)
    points = torch.empty((B, a_n * RES, cols * RES, 3), dtype=torch.uint8, device=dev)
    kp_l2 = torch.empty((a_n, B, 32), dtype=torch.float32, device=dev)
    kp_div = torch.empty((B, 32), dtype=torch.float32, device=dev)
    div_mse = torch.empty((N_FRAMES,), dtype=torch.float32, device=dev)
    im1 = im.unsqueeze(1)
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256, point_maps=True)
    fm.build()

    pinned = [torch.empty(tuple(t.shape), dtype=torch.uint8, pin_memory=True) for t in (classes, points)]   # as evaluate.py keeps them

    def batch(mode):                                      # 'off': the rollouts alone; 'scores': --no-save; 'on': sheets and scores
        sheets, scores = mode == 'on', mode != 'off'
        fm.run(None, {'image': im, 'action_code': act}, z=z)
        if sheets:
            ops.sheet_paste(classes, im1, [0], 0, 0, 'unit')
            ops.sheet_paste(classes, real, SHEET_FRAMES, 0, 1, 'unit')
        if scores:
            ops.fill_raw_(acc, 0.0)
        for a in range(a_n):
            o = fm.run(None, {'image': im, 'action_code': codes[a]}, z=z)
            pred = o['pred_im_seq'].contiguous()
            if sheets:
                ops.sheet_paste(classes, im1, [0], 1 + a, 0, 'unit')
                ops.sheet_paste(classes, pred, SHEET_FRAMES, 1 + a, 1, 'unit')
                ops.sheet_paste(points, o['current_points'].contiguous().unsqueeze(1), [0], a, 0, 'raw')
                ops.sheet_paste(points, o['future_points'].contiguous(), SHEET_FRAMES, a, 1, 'raw')
            if scores:
                ops.flat_copy_tensor(o['fut_pt_raw'].contiguous(), kp[0, a].data_ptr())
                ops.draw_moments_add(pred.reshape(N_FRAMES, RES, RES, 3), acc[0], acc[1])
        if scores:
            ops.keypoint_draw_metrics(kp[0], kp_real, out=(kp_l2, kp_div))
            ops.draw_diversity(acc[0], acc[1], a_n, (RES, RES, 3), out=div_mse)
        if sheets:
            for host, t in zip(pinned, (classes, points)):
                host.copy_(t)

    for _ in range(3):                                    # eager, capture, one replay
        fm.run(None, {'image': im, 'action_code': act}, z=z)
    batch('on')
    torch.cuda.synchronize(dev)
    modes = ('off', 'scores', 'on')
    ms = {m: [] for m in modes}
    copy_ms = {'pinned': [], 'pageable': []}
    for _ in range(batches):
        for m in modes:
            t0 = time.perf_counter()
            batch(m)
            torch.cuda.synchronize(dev)
            ms[m].append((time.perf_counter() - t0) * 1e3 / (1 + a_n))
        for kind in copy_ms:                              # the two copies of a sweep alone, on an idle device
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if kind == 'pinned':
                for host, t in zip(pinned, (classes, points)):
                    host.copy_(t)
            else:
                classes.cpu(), points.cpu()
            copy_ms[kind].append((time.perf_counter() - t0) * 1e3 / (1 + a_n))
    assert bool(torch.isfinite(div_mse).all()) and bool(torch.isfinite(kp_l2).all()) and bool(torch.isfinite(kp_div).all())
    assert bool((pinned[0] == classes.cpu()).all()) and bool((pinned[1] == points.cpu()).all())
    off, scores, on = (statistics.median(ms[m]) for m in modes)
    return {'batch': B, 'frames': N_FRAMES, 'classes': a_n, 'rollouts_per_sweep': 1 + a_n, 'sweeps_each': batches,
            'graph_replay': len(fm._graphs) == 1, 'sheet_mb': [round(classes.numel() / 1e6, 1), round(points.numel() / 1e6, 1)],
            'off_ms_per_rollout': round(off, 3), 'scores_only_ms_per_rollout': round(scores, 3), 'on_ms_per_rollout': round(on, 3),
            'scores_only_delta_ms_per_rollout': round(scores - off, 3), 'scores_only_overhead_pct': round(100 * (scores - off) / off, 2),
            'delta_ms_per_rollout': round(on - off, 3), 'overhead_pct': round(100 * (on - off) / off, 2),
            'sheet_copies_alone_ms_per_rollout': {k: round(statistics.median(v), 3) for k, v in copy_ms.items()},
            'off_ms_all': [round(v, 2) for v in ms['off']], 'scores_only_ms_all': [round(v, 2) for v in ms['scores']],
            'on_ms_all': [round(v, 2) for v in ms['on']]}


DRIVES = (('labels', 'absolute', 0, False), ('hold', 'hold', 0, False), ('transfer', 'relative', 1, False),
          ('transfer_scaled', 'relative', 1, True))


def drive_kernel_leg(dev, launches):
    from kpx_amd import ops
    g = torch.Generator(device=dev).manual_seed(5)
    k, t = 15, 32
    src, first = (torch.rand((B, k, 2), generator=g, device=dev) * 1.6 - 0.8 for _ in range(2))
    seq = torch.rand((B, t, k, 2), generator=g, device=dev) * 1.6 - 0.8
    out = torch.empty((B, t, k, 2), dtype=torch.float32, device=dev)
    res = {'shape': [B, t, k, 2], 'out_kb': round(out.numel() * 4 / 1e3, 1), 'launches': launches}
    for name, mode, shift, scaled in (('hold', 'hold', 0, False), ('absolute', 'absolute', 1, False), ('relative', 'relative', 1, False),
                                      ('relative_scaled', 'relative', 1, True)):
        if mode == 'hold':
            fn = lambda: ops.points_retarget(src, 'hold', frames=t, out=out)
        else:
            fn = lambda: ops.points_retarget(src, mode, first, seq, shift=shift, scaled=scaled, out=out)
        us = _event_times(fn, launches, dev)
        assert bool(torch.isfinite(out).all())
        res[name] = {'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1)}
    return res


def drive_rollout_leg(dev, rollouts):
    import kpx_amd
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    first = torch.rand((B, 15, 2), generator=g, device=dev) * 1.6 - 0.8
    seq = torch.rand((B, 32, 15, 2), generator=g, device=dev) * 1.6 - 0.8
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    feed = {'image': im, 'action_code': act}
    runs = {'model': lambda: fm.run(None, feed, z=z)}
    for name, mode, shift, scaled in DRIVES:
        drive = {'mode': mode, 'shift': shift, 'scaled': scaled}
        if mode != 'hold':
            drive.update(first=first, seq=seq)
        runs[name] = (lambda d: lambda: fm.run(None, feed, drive=d))(drive)
    for fn in runs.values():
        for _ in range(3):                                # eager, capture, one replay
            out = fn()
        assert bool(torch.isfinite(out['pred_im_seq']).all())
    torch.cuda.synchronize(dev)
    ms = {name: [] for name in runs}
    for _ in range(rollouts):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    own = statistics.median(ms['model'])
    res = {'batch': B, 'frames': N_FRAMES, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == len(runs) and not fm._graph_failed}
    for name in runs:
        med = statistics.median(ms[name])
        res[name] = {'ms': round(med, 3), 'frames_per_s': round(N_FRAMES / (med * 1e-3), 1), 'ms_all': [round(v, 2) for v in ms[name]]}
        if name != 'model':
            res[name].update(delta_ms=round(med - own, 3), delta_pct=round(100 * (med - own) / own, 2))
    return res

CLASSIFIER_CELLS = [256, 256]                             # = kpx_amd.action_classifier_model.DEFAULT_CELLS


def classifier_kernel_leg(dev, launches):
    """The three launches of csrc/classify.hip alone, at the rows a configs[4] rollout scores (64) and at 1024 rows, A = 9."""
    from kpx_amd import ops
    from kpx_amd._lib import lib, check
    res = {}
    g = torch.Generator(device=dev).manual_seed(5)
    for rows in (B, 1024):
        a = ACTION_CLASSES
        x = torch.randn((rows, a), generator=g, device=dev)
        t = torch.randint(0, a, (rows,), generator=g, device=dev).to(torch.int32)
        y = torch.eye(a, device=dev)[t.long()].contiguous()
        loss, lse, dl = torch.empty(1, device=dev), torch.empty(rows, device=dev), torch.empty((rows, a), device=dev)
        conf = torch.zeros((a, a), dtype=torch.int32, device=dev)
        out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, device=dev))
        fns = {'softmax_xent_fwd': lambda: check(lib.kpx_softmax_xent_fwd_f32(x.data_ptr(), y.data_ptr(), rows, a, loss.data_ptr(), lse.data_ptr(),
                                                                               ops._stream()), 'fwd'),
               'softmax_xent_bwd': lambda: check(lib.kpx_softmax_xent_bwd_f32(x.data_ptr(), y.data_ptr(), lse.data_ptr(), rows, a, None, 1.0,
                                                                               dl.data_ptr(), ops._stream()), 'bwd'),
               'class_scores': lambda: ops.class_scores(x, t, conf, out=out, check_target=False)}
        row = {}
        for name, fn in fns.items():                      # launch-bound calls: no rate is quoted
            us = _event_times(fn, launches, dev)
            row[name] = {'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1)}
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all()) and int(conf.sum()) == rows * (3 + launches)
        res['rows_%d' % rows] = dict(row, classes=a, launches=launches)
    return res


def classifier_rollout_leg(dev, rollouts):
    """--action-accuracy beside a configs[4] rollout: classify + class_scores + the fp64 moments of the features of one draw (the two
    accumulators of draw 0), alternated with the bare rollout in one process.  The recogniser has its initial values: the time does not
    depend on them."""
    import kpx_amd
    from kpx_amd import ops
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9, 'classifier_cells': CLASSIFIER_CELLS},
           'training': {'batch_size': B, 'lr': None}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    target = torch.randint(0, 9, (B,), generator=g, device=dev).to(torch.int32)
    act = torch.eye(9, device=dev)[target.long()]
    z = torch.randn((B, 64), generator=g, device=dev)
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    cm = kpx_amd.ActionClassifierModel(cfg, is_training=False, device=dev)
    cm.build()
    u = CLASSIFIER_CELLS[-1]
    conf = torch.zeros((9, 9), dtype=torch.int32, device=dev)
    out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev))
    moments = [(torch.zeros(u, dtype=torch.float64, device=dev), torch.zeros((u, u), dtype=torch.float64, device=dev)) for _ in range(2)]

    def rollout(score):
        o = fm.run(None, feed, z=z)
        if score:
            logits, feats = cm.classify(o['fut_pt_raw'])
            ops.class_scores(logits, target, conf, out=out, check_target=False)
            feats = feats.double()
            for s_, o_ in moments:
                ops.moments_add(feats, s_, o_)

    for _ in range(3):                                    # eager, capture, one replay
        rollout(True)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            rollout(score)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(moments[0][1]).all())
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'frames': N_FRAMES, 'classifier_cells': CLASSIFIER_CELLS, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 1,
            'off_ms_per_rollout': round(off, 3), 'on_ms_per_rollout': round(on, 3), 'delta_ms_per_rollout': round(on - off, 3),
            'overhead_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


STAB_FRAMES, STAB_WARPS, STAB_POINTS, VIDEO_FRAMES = 128, 4, 40, 663


def stability_kernel_leg(dev, launches):
    """kpx_affine_warp_f32 at [128 frames x 4 maps, 128, 128, 3] beside a float4 device copy of the same bytes (every output row reads about a
    frame and writes one: 2 x the output), and kpx_equivariance_scores_f32 at K = 40 on the rows of a 663-frame video at W = 2."""
    from kpx_amd import ops, stability
    g = torch.Generator(device=dev).manual_seed(6)
    frames = torch.rand((STAB_FRAMES, RES, RES, 3), generator=g, device=dev) * 2 - 1
    coef, _ = stability.draw_warps(STAB_FRAMES, STAB_WARPS, seed=1, res=RES)
    r = STAB_FRAMES * STAB_WARPS
    rows = torch.arange(STAB_FRAMES, dtype=torch.int32, device=dev).repeat_interleave(STAB_WARPS).contiguous()
    coef = torch.from_numpy(coef.reshape(r, 6)).to(dev)
    out, other = torch.empty((r, RES, RES, 3), device=dev), torch.empty((r, RES, RES, 3), device=dev)
    nbytes = 2 * out.numel() * 4
    res = {'warp': {'shape': [r, RES, RES, 3], 'frames': STAB_FRAMES, 'maps_per_frame': STAB_WARPS, 'mb': round(nbytes / 1e6, 1),
                    'fits_infinity_cache': nbytes < 256e6, 'launches': launches}}
    for key, fn in (('warp', lambda: ops.affine_warp(frames, rows, coef, out=out, check_tables=False)), ('copy', lambda: other.copy_(out))):
        us = _event_times(fn, launches, dev)
        med = statistics.median(us)
        res['warp'][key] = {'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                            'gb_per_s': round(nbytes / (med * 1e-6) / 1e9, 1), 'frac_of_copy_rate': round(nbytes / (med * 1e-6) / COPY_RATE, 3)}
    res['warp']['frac_of_copy_in_this_process'] = round(res['warp']['copy']['median_us'] / res['warp']['warp']['median_us'], 3)
    assert bool(torch.isfinite(out).all())
    del out, other
    torch.cuda.empty_cache()
    n, w, k = VIDEO_FRAMES, 2, STAB_POINTS
    _, fwd = stability.draw_warps(n, w, seed=2, res=RES)
    pts = torch.rand((n, k, 2), generator=g, device=dev) * 1.6 - 0.8
    pts_w = torch.rand((n * w, k, 2), generator=g, device=dev) * 1.6 - 0.8
    rows = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(w).contiguous()
    fwd = torch.from_numpy(fwd.reshape(n * w, 6)).to(dev)
    outs = ops.equivariance_scores(pts, pts_w, rows, fwd)
    us = _event_times(lambda: ops.equivariance_scores(pts, pts_w, rows, fwd, out=outs, check_tables=False), launches, dev)
    assert int(outs[3].sum()) > 0                             # a launch-bound call: no rate is quoted
    res['scores'] = {'rows': n * w, 'points': k, 'launches': launches, 'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1),
                     'max_us': round(max(us), 1)}
    return res


def stability_video_leg(dev, rollouts):
    """A 663-frame video through KeypointModel.run (K = 40, 128 x 128) without and with stability() at W = 2 (the points of run() reused),
    alternated in one process; and the warp of those 2 x 663 frames alone beside the detector on them."""
    import kpx_amd
    from kpx_amd import ops, stability
    cfg = {'model': {'n_pts': STAB_POINTS}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(8)
    n, w = VIDEO_FRAMES, 2
    video = torch.rand((1, n, RES, RES, 3), generator=g, device=dev) * 2 - 1
    coef, fwd = stability.draw_warps(n, w, seed=3, res=RES)
    model = kpx_amd.KeypointModel(cfg, device=dev)
    model.build(None)

    def one(score):
        o = model.run(None, {'image': video})
        if score:
            return model.stability(video[0], coef, fwd, pts=o['pts'][0])

    for _ in range(2):
        last = one(True)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            one(score)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3)
    assert int(last['n_valid'].sum()) > 0
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    rows = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(w).contiguous()
    coef_dev = torch.from_numpy(coef.reshape(n * w, 6)).to(dev)
    warped = torch.empty((n * w, RES, RES, 3), device=dev)
    warp_us = statistics.median(_event_times(lambda: ops.affine_warp(video[0], rows, coef_dev, out=warped, check_tables=False), 10, dev))
    detect = []
    for _ in range(max(3, rollouts // 2)):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        model.run(None, {'image': warped[None]})
        torch.cuda.synchronize(dev)
        detect.append((time.perf_counter() - t0) * 1e3)
    det = statistics.median(detect)
    return {'frames': n, 'maps_per_frame': w, 'points': STAB_POINTS, 'frames_per_launch': model.frames_per_launch, 'runs_each': rollouts,
            'run_ms': round(off, 3), 'run_and_stability_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'delta_over_run': round((on - off) / off, 3),
            'warp_of_the_warped_frames_ms': round(warp_us / 1e3, 3), 'detector_on_the_warped_frames_ms': round(det, 3),
            'warp_over_detector': round(warp_us / 1e3 / det, 4),
            'run_ms_all': [round(v, 2) for v in ms[False]], 'run_and_stability_ms_all': [round(v, 2) for v in ms[True]]}


JOINT_COUNT = 13


def _joint_inputs(dev, f, k, j, seed):
    """Device inputs of the three joint launches for one video of f frames, from planted annotations of a 320 x 240 frame."""
    import numpy as np
    from kpx_amd import joints
    labels = joints.planted_labels([seed, 0], f, j, (320, 240))
    g = torch.Generator(device=dev).manual_seed(seed)
    pts = (torch.rand((f, k, 2), generator=g, device=dev) * 1.8 - 0.9).contiguous()
    xy = torch.from_numpy(np.stack([labels['x'], labels['y']], axis=-1).astype(np.float32)).to(dev)
    vis = torch.from_numpy(labels['visibility'].astype(np.uint8)).to(dev)
    bbox = torch.from_numpy(labels['bbox'].astype(np.float32)).to(dev)
    cmap = torch.from_numpy(joints.crop_map(320, 240)).to(dev)
    return labels, pts, xy, vis, bbox, cmap


def joints_kernel_leg(dev, launches):
    """The three launches alone at F = 663, J = 13 for K = 15 and K = 40, each beside a device copy of the bytes it reads and writes."""
    from kpx_amd import ops
    out = {}
    f, j = VIDEO_FRAMES, JOINT_COUNT
    for k in (15, 40):
        d = 2 * k + 1
        _, pts, xy, vis, bbox, cmap = _joint_inputs(dev, f, k, j, 20 + k)
        target, mask, norm = ops.joint_targets(xy, vis, bbox, cmap)
        gm, bm, n = (torch.zeros(s, dtype=t, device=dev) for s, t in (((j, d, d), torch.float64), ((j, d, 2), torch.float64), ((j,), torch.int64)))
        w = (torch.rand((j, d, 2), dtype=torch.float64, device=dev) - 0.5) / d
        alpha = torch.tensor([0.05, 0.1, 0.2], dtype=torch.float64, device=dev)
        nbytes = {'targets': xy.numel() * 4 + vis.numel() + bbox.numel() * 4 + target.numel() * 4 + mask.numel() + norm.numel() * 4,
                  'moments': pts.numel() * 4 + target.numel() * 4 + mask.numel() + 2 * (gm.numel() + bm.numel() + n.numel()) * 8,
                  'scores': pts.numel() * 4 + target.numel() * 4 + mask.numel() + norm.numel() * 4 + w.numel() * 8 + f * j * (8 + 4 + 1)}
        fns = {'targets': lambda: ops.joint_targets(xy, vis, bbox, cmap), 'moments': lambda: ops.joint_moments_add(pts, target, mask, gm, bm, n),
               'scores': lambda: ops.joint_scores(pts, target, mask, norm, w, alpha)}
        res = {'frames': f, 'points': k, 'joints': j, 'D': d, 'launches': launches}
        for key in ('targets', 'moments', 'scores'):
            us = _event_times(fns[key], launches, dev)
            src, dst = torch.empty(nbytes[key] // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes[key] // 2, dtype=torch.uint8, device=dev)
            cp = _event_times(lambda: dst.copy_(src), launches, dev)
            res[key] = {'bytes': nbytes[key], 'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                        'copy_median_us': round(statistics.median(cp), 1), 'copy_min_us': round(min(cp), 1)}
        assert int(n.sum()) > 0 and bool(torch.isfinite(gm).all())
        out['K%d' % k] = res
    return out


def joints_video_leg(dev, rollouts):
    """A 663-frame video through KeypointModel.run (K = 40) without and with JointRegression.add as a train video, alternated in one
    process; then finish() over the videos added, per video."""
    import kpx_amd
    from kpx_amd import joints
    cfg = {'model': {'n_pts': STAB_POINTS}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(9)
    n = VIDEO_FRAMES
    video = torch.rand((1, n, RES, RES, 3), generator=g, device=dev) * 2 - 1
    labels = joints.planted_labels([9, 0], n, JOINT_COUNT, (320, 240))
    model = kpx_amd.KeypointModel(cfg, device=dev)
    model.build(None)
    reg = joints.JointRegression(STAB_POINTS, JOINT_COUNT, device=dev)

    def one(score):
        o = model.run(None, {'image': video})
        if score:
            reg.add('train', len(reg.kept), o['pts'][0], labels, (320, 240))

    for _ in range(2):
        one(True)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            one(score)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = reg.finish()
    torch.cuda.synchronize(dev)
    fin = (time.perf_counter() - t0) * 1e3
    assert out['summary']['overall']['valid_entries'] > 0
    return {'frames': n, 'points': STAB_POINTS, 'joints': JOINT_COUNT, 'runs_each': rollouts, 'run_ms': round(off, 3), 'run_and_add_ms': round(on, 3),
            'delta_ms': round(on - off, 3), 'delta_over_run': round((on - off) / off, 4), 'videos_finished': len(reg.kept),
            'finish_ms': round(fin, 3), 'finish_ms_per_video': round(fin / len(reg.kept), 3),
            'run_ms_all': [round(v, 2) for v in ms[False]], 'run_and_add_ms_all': [round(v, 2) for v in ms[True]]}


def _gif_canvas(dev, g, samples=B):
    """compare.gif-like canvases uint8 [samples, 33, RES, 3 RES, 3]: two smooth image columns, one mostly black key-point column"""
    low = torch.rand((samples * 33, 3, 8, 16), generator=g, device=dev)
    smooth = torch.nn.functional.interpolate(low, size=(RES, 2 * RES), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    smooth = (smooth + 0.02 * torch.rand(smooth.shape, generator=g, device=dev)).clamp(0, 1)
    canvas = torch.zeros((samples, 33, RES, 3 * RES, 3), dtype=torch.uint8, device=dev)
    canvas[:, :, :, :2 * RES] = (smooth * 255).to(torch.uint8).view(samples, 33, RES, 2 * RES, 3)
    for k in range(15):                                   # 15 coloured key-point blobs
        y, x = 8 + 7 * k, 2 * RES + 10 + 7 * k
        canvas[:, :, y:y + 5, x:x + 5] = torch.tensor([(37 * k) % 256, (91 * k + 60) % 256, (53 * k + 120) % 256], dtype=torch.uint8, device=dev)
    return canvas


def gif_kernel_leg(dev, launches):
    import numpy as np
    from PIL import Image
    from kpx_amd import gif, ops
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tests'))
    import gif_ref
    g = torch.Generator(device=dev).manual_seed(20)
    canvas = _gif_canvas(dev, g)
    noise = torch.randint(0, 256, tuple(canvas.shape), generator=g, device=dev, dtype=torch.uint8)
    dst = torch.empty_like(canvas)
    hist = torch.zeros((B, 32768, 4), dtype=torch.int32, device=dev)
    idx, palettes, sizes = ops.gif_indices(canvas)
    pal_dev, sizes_dev = torch.from_numpy(palettes).to(dev), torch.from_numpy(sizes).to(dev)
    pixels = canvas.numel() // 3
    res = {'canvas': list(canvas.shape), 'rgb_mb': round(canvas.numel() / 1e6, 1), 'palette_sizes_min_max': [int(sizes.min()), int(sizes.max())]}
    legs = (('device_copy', lambda: dst.copy_(canvas)), ('color_hist', lambda: ops.color_hist_add(canvas.view(B, -1, 3), hist)),
            ('color_hist_noise', lambda: ops.color_hist_add(noise.view(B, -1, 3), hist)),
            ('palette_map', lambda: ops.palette_map(canvas, pal_dev, sizes_dev, 0, out=idx)),
            ('palette_map_dither8', lambda: ops.palette_map(canvas, pal_dev, sizes_dev, 8, out=idx)))
    for name, fn in legs:
        hist.zero_()                                      # (the repeated adds wrap modulo 2^32: a timing run, the sums are not read)
        us = _event_times(fn, launches, dev)
        res[name] = {'launches': launches, 'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1)}
    copy_us = res['device_copy']['median_us']
    for name, _ in legs[1:]:
        res[name]['over_device_copy'] = round(res[name]['median_us'] / copy_us, 2)
    evals = float(pixels) * float(sizes.astype(np.float64).mean())
    res['palette_map']['candidates_per_s'] = round(evals / (res['palette_map']['median_us'] * 1e-6), 0)
    res['device_copy']['gb_per_s'] = round(2 * canvas.numel() / (copy_us * 1e-6) / 1e9, 1)
    # the host route: fp32 frames to the host, quantised there, PIL's quantiser per frame -- against the device route and the index copy
    n = 4
    frames32 = (canvas[:n].float() / 255 * 2 - 1).contiguous()
    ms = {'host': [], 'device': []}
    for _ in range(3):                                    # the first pair warms both routes up and is dropped
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        x = frames32.cpu().numpy()
        q = ((0.5 * (x + 1.0)) * 255).astype(np.uint8)
        for s in range(n):
            for t in range(33):
                Image.fromarray(q[s, t]).quantize(256)
        ms['host'].append((time.perf_counter() - t0) * 1e3 / n)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        i4, _, _ = ops.gif_indices(canvas[:n])
        i4.cpu()
        ms['device'].append((time.perf_counter() - t0) * 1e3 / n)
    res['route_ms_per_sample'] = {'samples': n, 'host_fp32_copy_and_pil_quantize': round(statistics.median(ms['host'][1:]), 2),
                                  'device_gif_indices_and_copy': round(statistics.median(ms['device'][1:]), 2)}
    one = idx[0].cpu().numpy()
    t0 = time.perf_counter()
    c_bytes = sum(len(gif.lzw(one[t], 8)) for t in range(33))
    t1 = time.perf_counter()
    py_bytes = sum(len(gif_ref.lzw(one[t].reshape(-1), 8)) for t in range(33))
    t2 = time.perf_counter()
    assert c_bytes == py_bytes
    res['lzw_ms_per_sample'] = {'library_host_code': round((t1 - t0) * 1e3, 2), 'pure_python': round((t2 - t1) * 1e3, 2), 'bytes': c_bytes}
    return res


def gif_rollout_leg(dev, rollouts):
    import shutil
    import tempfile
    import kpx_amd
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    real = torch.rand((B, 32, RES, RES, 3), generator=g, device=dev) * 2 - 1
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256, point_maps=True)
    fm.build()
    gifs = kpx_amd.gif.RolloutGifs(10, 0)
    out_dir = tempfile.mkdtemp(prefix='kpx_gif_bench_')
    ops = kpx_amd.ops

    def run(mode):
        o = fm.run(None, {'image': im, 'action_code': act}, z=z)
        cols = [('real', im, real, 'unit'), ('pred', o['im'], o['pred_im_seq'], 'unit'), ('points', o['current_points'], o['future_points'], 'raw')]
        if mode == 'device':                              # what reaches the host: compose, histogram, median cut, map, the copy of the indices
            for sel in (cols[1:2], cols):
                canvas = gifs._canvas([c[1:] for c in sel])
                gifs._host(ops.gif_indices(canvas, 0)[0])
        elif mode == 'on':
            gifs.write(out_dir, 0, cols)

    try:
        for _ in range(3):                                # eager, capture, one replay
            run('off')
        run('on')
        torch.cuda.synchronize(dev)
        modes = ('off', 'device', 'on')
        ms = {m: [] for m in modes}
        for _ in range(max(1, min(rollouts, 3))):
            for m in modes:
                t0 = time.perf_counter()
                run(m)
                torch.cuda.synchronize(dev)
                ms[m].append((time.perf_counter() - t0) * 1e3)
        size = sum(os.path.getsize(os.path.join(d, n)) for d, _, names in os.walk(out_dir) for n in names)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    off, device, on = (statistics.median(ms[m]) for m in modes)
    return {'batch': B, 'frames': N_FRAMES, 'graph_replay': len(fm._graphs) == 1, 'gif_files': 2 * B, 'gif_mb': round(size / 1e6, 1),
            'off_ms_per_rollout': round(off, 2), 'on_ms_per_rollout': round(on, 2), 'flag_ms_per_rollout': round(on - off, 2),
            'device_part_with_median_cut_ms': round(device - off, 2), 'lzw_and_files_ms': round(on - device, 2),
            'flag_ms_per_sample': round((on - off) / B, 2), 'off_ms_all': [round(v, 1) for v in ms['off']],
            'device_ms_all': [round(v, 1) for v in ms['device']], 'on_ms_all': [round(v, 1) for v in ms['on']]}


def video_kernel_leg(dev, launches, quality=90):
    import io
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from kpx_amd import mjpeg, ops
    from kpx_amd._lib import lib
    g = torch.Generator(device=dev).manual_seed(20)
    compare = _gif_canvas(dev, g)
    canvases = {'pred': compare[:, :, :, :RES].contiguous(), 'compare': compare}
    res = {'quality': quality, 'budget_mb': ops.JPEG_BUDGET >> 20}
    for name, canvas in canvases.items():
        flat = canvas.view((-1,) + tuple(canvas.shape[2:]))
        n, h, w = (int(v) for v in flat.shape[:3])
        bound = int(lib.kpx_jpeg_scan_bound(h, w))
        per = max(1, ops.JPEG_BUDGET // (int(lib.kpx_jpeg_workspace_bytes(1, h, w)) + bound))
        scans = torch.empty(min(per, n) * bound, dtype=torch.uint8, device=dev)
        offsets = torch.empty(min(per, n) + 1, dtype=torch.int64, device=dev)
        dst = torch.empty_like(canvas)

        def encode_all():
            for lo in range(0, n, per):
                m = min(per, n - lo)
                ops.jpeg_scans(flat[lo:lo + m], quality, scans[:m * bound], offsets[:m + 1])

        leg = {'canvas': list(canvas.shape), 'rgb_mb': round(canvas.numel() / 1e6, 1), 'frames_per_chunk': min(per, n), 'chunks': -(-n // per)}
        for key, fn in (('device_copy', lambda: dst.copy_(canvas)), ('jpeg_scans', encode_all)):
            us = _event_times(fn, launches, dev)
            leg[key] = {'launches': launches, 'median_ms': round(statistics.median(us) / 1e3, 3), 'min_ms': round(min(us) / 1e3, 3),
                        'max_ms': round(max(us) / 1e3, 3)}
        leg['jpeg_scans']['over_device_copy'] = round(leg['jpeg_scans']['median_ms'] / leg['device_copy']['median_ms'], 1)
        leg['jpeg_scans']['rgb_gb_per_s'] = round(canvas.numel() / (leg['jpeg_scans']['median_ms'] * 1e-3) / 1e9, 1)
        del dst
        ms = {'device': [], 'host': []}
        samples = int(canvas.shape[0])
        for _ in range(3):                                    # the first pair warms both routes up and is dropped
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            mine = ops.jpeg_encode(flat, quality)
            ms['device'].append((time.perf_counter() - t0) * 1e3 / samples)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            host = flat.cpu().numpy()

            def save(i):
                buf = io.BytesIO()
                Image.fromarray(host[i]).save(buf, 'JPEG', quality=quality, subsampling=2)
                return buf.tell()
            with ThreadPoolExecutor(16) as pool:
                pil_bytes = sum(pool.map(save, range(n)))
            ms['host'].append((time.perf_counter() - t0) * 1e3 / samples)
        prefix = len(mjpeg.frame_prefix(h, w, mjpeg.quant_tables(quality))) + 2
        leg['jpeg_mb'] = round((sum(len(s) for s in mine) + n * prefix) / 1e6, 2)
        leg['pil_jpeg_mb'] = round(pil_bytes / 1e6, 2)
        leg['bytes_to_host_over_rgb'] = round(sum(len(s) for s in mine) / canvas.numel(), 4)
        leg['route_ms_per_sample'] = {'samples': samples, 'device_jpeg_encode_and_copy': round(statistics.median(ms['device'][1:]), 2),
                                      'host_u8_copy_and_pil_save_16_threads': round(statistics.median(ms['host'][1:]), 2)}
        res[name] = leg
    return res


def video_rollout_leg(dev, rollouts):
    import shutil
    import tempfile
    import kpx_amd
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    real = torch.rand((B, 32, RES, RES, 3), generator=g, device=dev) * 2 - 1
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256, point_maps=True)
    fm.build()
    writers = {'gif': kpx_amd.gif.RolloutGifs(10, 0), 'video': kpx_amd.mjpeg.RolloutVideos(10, 90)}
    out_dir = tempfile.mkdtemp(prefix='kpx_video_bench_')

    def run(mode):
        o = fm.run(None, {'image': im, 'action_code': act}, z=z)
        cols = [('real', im, real, 'unit'), ('pred', o['im'], o['pred_im_seq'], 'unit'), ('points', o['current_points'], o['future_points'], 'raw')]
        if mode != 'off':
            writers[mode].write(out_dir, 0, cols)

    try:
        for _ in range(3):                                # eager, capture, one replay
            run('off')
        run('gif')
        run('video')
        torch.cuda.synchronize(dev)
        modes = ('off', 'gif', 'video')
        ms = {m: [] for m in modes}
        for _ in range(max(1, min(rollouts, 3))):
            for m in modes:
                t0 = time.perf_counter()
                run(m)
                torch.cuda.synchronize(dev)
                ms[m].append((time.perf_counter() - t0) * 1e3)
        size = {ext: sum(os.path.getsize(os.path.join(d, n)) for d, _, names in os.walk(out_dir) for n in names if n.endswith(ext))
                for ext in ('.gif', '.avi')}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    off, gif, video = (statistics.median(ms[m]) for m in modes)
    return {'batch': B, 'frames': N_FRAMES, 'graph_replay': len(fm._graphs) == 1, 'files_each': 2 * B, 'gif_mb': round(size['.gif'] / 1e6, 1),
            'avi_mb': round(size['.avi'] / 1e6, 1), 'off_ms_per_rollout': round(off, 2), 'gif_ms_per_rollout': round(gif, 2),
            'video_ms_per_rollout': round(video, 2), 'gif_flag_ms_per_rollout': round(gif - off, 2),
            'video_flag_ms_per_rollout': round(video - off, 2), 'gif_flag_ms_per_sample': round((gif - off) / B, 2),
            'video_flag_ms_per_sample': round((video - off) / B, 2), 'off_ms_all': [round(v, 1) for v in ms['off']],
            'gif_ms_all': [round(v, 1) for v in ms['gif']], 'video_ms_all': [round(v, 1) for v in ms['video']]}


def animate_kernel_leg(dev, launches):
    from kpx_amd import gif, ops
    t, k = 32, 15
    g = torch.Generator(device=dev).manual_seed(21)
    first = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    seq = torch.rand((B, t, RES, RES, 3), generator=g, device=dev) * 2 - 1
    pts_first = torch.rand((B, k, 2), generator=g, device=dev) * 1.8 - 0.9
    pts_seq = torch.rand((B, t, k, 2), generator=g, device=dev) * 1.8 - 0.9
    colors = torch.randint(0, 256, (k, 3), generator=g, device=dev, dtype=torch.uint8)
    canvas = torch.empty((B, t + 1, RES, RES, 3), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(seq)
    gifs = gif.RolloutGifs(10, 0)
    legs = (('device_copy', lambda: dst.copy_(seq)),
            ('cell_frames_r0', lambda: ops.cell_frames(canvas, first, seq, 0, 0, 'unit')),
            ('cell_frames_r3', lambda: ops.cell_frames(canvas, first, seq, 0, 0, 'unit', pts_first, pts_seq, colors, 3)),
            ('stack_copies_sheet_paste', lambda: gifs._canvas([(first, seq, 'unit')])))
    values = first.numel() + seq.numel()
    moved = {'device_copy': 8 * seq.numel(), 'cell_frames_r0': 5 * values, 'cell_frames_r3': 5 * values,
             'stack_copies_sheet_paste': 8 * values + 5 * values}           # the staging stack is written and read again
    res = {'first': list(first.shape), 'seq': list(seq.shape), 'canvas': list(canvas.shape), 'key_points': k}
    for name, fn in legs:
        us = _event_times(fn, launches, dev)
        med = statistics.median(us)
        res[name] = {'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                     'mb_moved': round(moved[name] / 1e6, 1), 'gb_per_s': round(moved[name] / (med * 1e-6) / 1e9, 1)}
    copy = res['device_copy']['gb_per_s']
    for name, _ in legs[1:3]:
        res[name]['fraction_of_copy_rate'] = round(res[name]['gb_per_s'] / copy, 3)
    res['cell_frames_r0']['over_existing_route'] = round(res['cell_frames_r0']['median_us'] / res['stack_copies_sheet_paste']['median_us'], 3)
    res['cell_frames_r3']['over_r0'] = round(res['cell_frames_r3']['median_us'] / res['cell_frames_r0']['median_us'], 3)
    return res


def animate_stills_leg(dev, rollouts):
    """animate.py's loop for a batch of 8 stills, 9 classes x 1 draw, overlay radius 3: the rollouts alone, with the canvases (both grids
    composed, quantised, the indices copied), and with the host GIF work (LZW, files); ms per still"""
    import shutil
    import tempfile
    import kpx_amd
    from kpx_amd import stills
    n, classes, radius = 8, 9, 3
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': classes}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(8)
    low = torch.rand((n, 3, 8, 8), generator=g, device=dev)
    im = (torch.nn.functional.interpolate(low, size=(RES, RES), mode='bilinear', align_corners=False).permute(0, 2, 3, 1) * 2 - 1).contiguous()
    codes = torch.eye(classes, device=dev)
    z = torch.randn((1, 64), generator=g, device=dev).expand(n, -1).contiguous()
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256, point_maps=True)
    fm.build()
    ops = kpx_amd.ops
    colors = torch.from_numpy(stills.marker_colors(fm.colors)).to(dev)
    gifs = kpx_amd.gif.RolloutGifs(10, 0)
    grid = torch.empty((n, 33, RES, classes * RES, 3), dtype=torch.uint8, device=dev)
    over = torch.empty_like(grid)
    out_dir = tempfile.mkdtemp(prefix='kpx_animate_bench_')
    paths = {name: [os.path.join(out_dir, '%s_%d.gif' % (name, i)) for i in range(n)] for name in ('classes', 'overlay')}

    def run(mode):
        for a in range(classes):
            o = fm.run(None, {'image': im, 'action_code': codes[a:a + 1].expand(n, -1).contiguous()}, z=z)
            if mode != 'off':
                pred = o['pred_im_seq'].contiguous()
                ops.cell_frames(grid, im, pred, 0, a, 'unit')
                ops.cell_frames(over, im, pred, 0, a, 'unit', o['first_pt'].reshape(n, 15, 2).contiguous(), o['fut_pt_raw'].contiguous(), colors, radius)
        if mode == 'device':
            for canvas in (grid, over):
                gifs._host(ops.gif_indices(canvas, 0)[0])
        elif mode == 'on':
            stills.write_grid_gifs(gifs, grid, paths['classes'])
            stills.write_grid_gifs(gifs, over, paths['overlay'])

    try:
        for _ in range(3):                                # eager, capture, one replay
            run('off')
        run('on')
        torch.cuda.synchronize(dev)
        modes = ('off', 'device', 'on')
        ms = {m: [] for m in modes}
        for _ in range(max(1, min(rollouts, 3))):
            for m in modes:
                t0 = time.perf_counter()
                run(m)
                torch.cuda.synchronize(dev)
                ms[m].append((time.perf_counter() - t0) * 1e3)
        size = sum(os.path.getsize(os.path.join(d, f)) for d, _, names in os.walk(out_dir) for f in names)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    off, device, on = (statistics.median(ms[m]) for m in modes)
    return {'stills': n, 'classes': classes, 'draws': 1, 'overlay_radius': radius, 'grid': list(grid.shape), 'gif_files': 2 * n,
            'gif_mb': round(size / 1e6, 1), 'rollouts_ms_per_still': round(off / n, 2),
            'canvases_quantised_and_copied_ms_per_still': round((device - off) / n, 2), 'host_lzw_and_files_ms_per_still': round((on - device) / n, 2),
            'total_ms_per_still': round(on / n, 2), 'off_ms_all': [round(v, 1) for v in ms['off']],
            'device_ms_all': [round(v, 1) for v in ms['device']], 'on_ms_all': [round(v, 1) for v in ms['on']]}


def _c1_model(dev, guard, **kw):
    import kpx_amd
    cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': 32},
           'model': {'n_pts': 15}, 'paths': {'log_dir': '/tmp/kpx_bench', 'vggnet': None}}
    vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(seed=19), device=dev)
    model = kpx_amd.DetectorTranslatorModel(cfg, device=dev, vgg=vgg, image_size=RES, **({'guard': True} if guard else {}), **kw)
    model.build()
    return model


def guard_kernel_leg(dev, launches, sizes):
    from kpx_amd import ops
    res = {}
    for which, n in sizes.items():
        g = torch.randn(n, device=dev) * 1e-3
        p, m, v, dst = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, device=dev)
        clean, dirty = ops.new_guard_health(dev), ops.new_guard_health(dev)
        work = ops.grad_health_workspace(n, dev)
        ops.grad_health(torch.full((4,), float('inf'), device=dev), dirty)
        alpha = torch.full((1,), 1e-4, device=dev)
        legs = (('device_copy', lambda: dst.copy_(g), 8 * n),
                ('grad_health', lambda: ops.grad_health(g, clean, work), 4 * n),
                ('adam_dev_alpha', lambda: ops.adam_tf_flat_dev_alpha_(p, g, m, v, alpha, 0.5, 0.999, 1e-8), 28 * n),
                ('adam_guarded_clean', lambda: ops.adam_tf_flat_guarded_(p, g, m, v, alpha, 0.5, 0.999, 1e-8, clean), 28 * n),
                ('adam_guarded_skipped', lambda: ops.adam_tf_flat_guarded_(p, g, m, v, alpha, 0.5, 0.999, 1e-8, dirty), 0),
                ('guard_restore_dirty', lambda: ops.guard_restore_(dst, g, dirty), 8 * n))
        out = {'floats': n, 'mb': round(4 * n / 1e6, 1)}
        for name, fn, moved in legs:
            us = _event_times(fn, launches, dev)
            med = statistics.median(us)
            out[name] = {'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                         'gb_per_s': round(moved / (med * 1e-6) / 1e9, 1)}
        copy = out['device_copy']['gb_per_s']
        for name in ('grad_health', 'adam_dev_alpha', 'adam_guarded_clean', 'guard_restore_dirty'):
            out[name]['fraction_of_copy_rate'] = round(out[name]['gb_per_s'] / copy, 3)
        assert ops.read_guard_health(clean)['nonfinite'] == 0 and ops.read_guard_health(dirty)['skipped_total'] >= launches
        res[which] = out
        del g, p, m, v, dst
        torch.cuda.empty_cache()
    return res


def guard_step_leg(dev, steps):
    """The configs[1] train step with guard off and on: two models, blocks of ``steps`` replayed steps each, alternated three times."""
    from kpx_amd.synthetic import synthetic_pair
    models = {'off': _c1_model(dev, False), 'on': _c1_model(dev, True)}
    feed = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_pair(32, res=RES, seed0=0, seed1=1).items()}
    for m in models.values():
        for i in range(4):                                # eager, capture, replays
            m.train_step(None, feed, i, 32)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in models}
    for _ in range(3):
        for k, m in models.items():
            t0 = time.perf_counter()
            for i in range(steps):
                m.train_step(None, feed, 4 + i, 32)
            torch.cuda.synchronize(dev)
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    off, on = statistics.median(ms['off']), statistics.median(ms['on'])
    rep = models['on'].guard_report()
    return {'batch': 32, 'steps_per_block': steps, 'graph_replay': all(len(m._graphs) == 1 and not m._graph_failed for m in models.values()),
            'off_ms_per_step': round(off, 3), 'on_ms_per_step': round(on, 3), 'guard_ms_per_step': round(on - off, 3),
            'guard_percent': round(100.0 * (on - off) / off, 2), 'off_ms_all': [round(v, 3) for v in ms['off']],
            'on_ms_all': [round(v, 3) for v in ms['on']], 'moving_statistics_floats': {k: v.numel() for k, v in models['on'].store.moving.items()},
            'skipped': {k: r['skipped_total'] for k, r in rep.items()}}, {k: b.grads.numel() for k, b in models['on'].store.buckets.items()}


def ema_kernel_leg(dev, launches, n):
    from kpx_amd import ops
    p, e, dst = torch.randn(n, device=dev), torch.randn(n, device=dev), torch.empty(n, device=dev)
    rate, clean = torch.full((1,), 1e-3, device=dev), ops.new_guard_health(dev)
    legs = (('device_copy', lambda: dst.copy_(p), 8 * n),
            ('ema_flat', lambda: ops.ema_flat_(e, p, rate), 12 * n),
            ('ema_flat_clean_health', lambda: ops.ema_flat_(e, p, rate, clean), 12 * n),
            ('swap_flat', lambda: ops.swap_flat_(e, dst), 16 * n))
    out = {'floats': n, 'mb': round(4 * n / 1e6, 1)}
    for name, fn, moved in legs:
        us = _event_times(fn, launches, dev)
        med = statistics.median(us)
        out[name] = {'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                     'gb_per_s': round(moved / (med * 1e-6) / 1e9, 1)}
    for name in ('ema_flat', 'ema_flat_clean_health', 'swap_flat'):
        out[name]['fraction_of_copy_rate'] = round(out[name]['gb_per_s'] / out['device_copy']['gb_per_s'], 3)
    return {'G': out}


def ema_step_leg(dev, steps):
    """The configs[1] train step with ema off and on: two models, blocks of ``steps`` replayed steps each, alternated three times."""
    from kpx_amd.synthetic import synthetic_pair
    models = {'off': _c1_model(dev, False), 'on': _c1_model(dev, False, ema=0.999)}
    feed = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_pair(32, res=RES, seed0=0, seed1=1).items()}
    for m in models.values():
        for i in range(4):                                # eager, capture, replays
            m.train_step(None, feed, i, 32)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in models}
    for _ in range(3):
        for k, m in models.items():
            t0 = time.perf_counter()
            for i in range(steps):
                m.train_step(None, feed, 4 + i, 32)
            torch.cuda.synchronize(dev)
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    off, on = statistics.median(ms['off']), statistics.median(ms['on'])
    return {'batch': 32, 'steps_per_block': steps, 'decay': 0.999,
            'graph_replay': all(len(m._graphs) == 1 and not m._graph_failed for m in models.values()),
            'off_ms_per_step': round(off, 3), 'on_ms_per_step': round(on, 3), 'ema_ms_per_step': round(on - off, 3),
            'ema_percent': round(100.0 * (on - off) / off, 2), 'off_ms_all': [round(v, 3) for v in ms['off']],
            'on_ms_all': [round(v, 3) for v in ms['on']]}, models['on'].store.buckets['G'].ema.numel()


def clip_kernel_leg(dev, launches, model):
    """The clipped update beside the guarded update and a device copy, and the per-variable statistics beside the copy, on the two real
    buckets (the sizes and the segment tables of ``model``)."""
    from kpx_amd import ops
    res = {}
    for which, bucket in model.store.buckets.items():
        n = bucket.grads.numel()
        g = torch.randn(n, device=dev) * 1e-3
        p, m, v, dst = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.empty(n, device=dev)
        health, clip = ops.new_guard_health(dev), ops.new_clip_state(dev)
        ops.grad_health(g, health)
        norm = float(ops.read_guard_health(health)['sumsq']) ** 0.5
        alpha = torch.full((1,), 1e-4, device=dev)
        table = ops.grad_segment_table(bucket, dev)
        work, out = ops.grad_segment_workspace(table, dev)
        legs = (('device_copy', lambda: dst.copy_(g), 8 * n),
                ('adam_guarded_clean', lambda: ops.adam_tf_flat_guarded_(p, g, m, v, alpha, 0.5, 0.999, 1e-8, health), 28 * n),
                ('adam_clipped_below_bound', lambda: ops.adam_tf_flat_clipped_(p, g, m, v, alpha, 0.5, 0.999, 1e-8, health, clip, 4 * norm), 28 * n),
                ('adam_clipped_above_bound', lambda: ops.adam_tf_flat_clipped_(p, g, m, v, alpha, 0.5, 0.999, 1e-8, health, clip, norm / 4), 28 * n),
                ('segment_stats_g', lambda: ops.grad_segment_stats(g, None, table, work, out), 4 * table.size),
                ('segment_stats_g_and_p', lambda: ops.grad_segment_stats(g, p, table, work, out), 8 * table.size))
        o = {'floats': n, 'mb': round(4 * n / 1e6, 1), 'variables': table.n_segs, 'chunks': table.n_chunks}
        for name, fn, moved in legs:
            us = _event_times(fn, launches, dev)
            med = statistics.median(us)
            o[name] = {'launches': launches, 'median_us': round(med, 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1),
                       'gb_per_s': round(moved / (med * 1e-6) / 1e9, 1)}
        for name, _, _ in legs[1:]:
            o[name]['fraction_of_copy_rate'] = round(o[name]['gb_per_s'] / o['device_copy']['gb_per_s'], 3)
        o['clipped_over_guarded'] = round(o['adam_clipped_above_bound']['median_us'] / o['adam_guarded_clean']['median_us'], 3)
        assert ops.read_clip_state(clip)['clipped_total'] >= launches and ops.read_guard_health(health)['skipped_total'] == 0
        res[which] = o
        del g, p, m, v, dst
        torch.cuda.empty_cache()
    return res


def clip_step_leg(dev, steps):
    """The configs[1] train step guarded, and guarded with clip_norm (a bound every step exceeds): two models in one process, blocks of
    ``steps`` replayed steps each, alternated three times."""
    from kpx_amd.synthetic import synthetic_pair
    models = {'off': _c1_model(dev, True), 'on': _c1_model(dev, True, clip_norm=1e-3, grad_stats=True)}
    feed = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_pair(32, res=RES, seed0=0, seed1=1).items()}
    for m in models.values():
        for i in range(4):                                # eager, capture, replays
            m.train_step(None, feed, i, 32)
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in models}
    for _ in range(3):
        for k, m in models.items():
            t0 = time.perf_counter()
            for i in range(steps):
                m.train_step(None, feed, 4 + i, 32)
            torch.cuda.synchronize(dev)
            ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    off, on = statistics.median(ms['off']), statistics.median(ms['on'])
    t0 = time.perf_counter()
    models['on'].grad_stats()
    stats_ms = (time.perf_counter() - t0) * 1e3
    return {'batch': 32, 'steps_per_block': steps, 'clip_norm': 1e-3,
            'graph_replay': all(len(m._graphs) == 1 and not m._graph_failed for m in models.values()),
            'guarded_ms_per_step': round(off, 3), 'clipped_ms_per_step': round(on, 3), 'clip_ms_per_step': round(on - off, 3),
            'clip_percent': round(100.0 * (on - off) / off, 2), 'guarded_ms_all': [round(v, 3) for v in ms['off']],
            'clipped_ms_all': [round(v, 3) for v in ms['on']], 'grad_stats_call_ms': round(stats_ms, 2),
            'clip_report': models['on'].clip_report()}, models['on']

NOVELTY_VIDEOS, NOVELTY_K, NOVELTY_CLASSES = 1171, 40, 9


def _novelty_store(dev):
    import numpy as np
    from kpx_amd import novelty, resident
    rs = np.random.RandomState(5)
    counts = [int(v) for v in rs.randint(18, 664, size=NOVELTY_VIDEOS)]
    names = ['frames/%04d' % (v + 1) for v in range(NOVELTY_VIDEOS)]
    arrays = [(rs.rand(n, NOVELTY_K, 2) * 2.0 - 1.0).astype(np.float32) for n in counts]
    listing = ['%s %d' % (name, rs.randint(NOVELTY_CLASSES)) for name in names]
    idx = resident.LabelIndex(names, counts, arrays, [line.split()[1] for line in listing], NOVELTY_K)
    return novelty.MotionStore(None, listing, NOVELTY_K, NOVELTY_CLASSES, dev, index=idx)


def _novelty_torch_route(store, queries, window_chunk=1024, query_chunk=16):
    """The distances of the search by the route it replaces: gather every window, fp64 differences in torch, per-class amin.  -> d2 [Q, A]"""
    import numpy as np
    q, a, w = queries.shape[0], store.n_action, len(store.windows)
    action = store.table[:, 3].long()
    best = torch.full((q, a), float('inf'), dtype=torch.float64, device=queries.device)
    q64 = queries.double().reshape(q, -1, 2)
    n = q64.shape[1]
    for lo in range(0, w, window_chunk):
        hi = min(w, lo + window_chunk)
        v = store.gather(2 * np.arange(lo, hi)).double().reshape(hi - lo, -1, 2)
        cls = action[lo:hi]
        for qlo in range(0, q, query_chunk):
            qq = q64[qlo:qlo + query_chunk, None]
            ey2 = (qq[..., 1] - v[None, ..., 1]) ** 2
            d = torch.minimum(((qq[..., 0] - v[None, ..., 0]) ** 2 + ey2).sum(-1), ((qq[..., 0] + v[None, ..., 0]) ** 2 + ey2).sum(-1)) / n
            best[qlo:qlo + query_chunk].scatter_reduce_(1, cls[None].expand(d.shape[0], -1), d, 'amin')
    return best


def novelty_kernel_leg(dev, launches):
    store = _novelty_store(dev)
    w, n = len(store.windows), 32 * NOVELTY_K
    labels = store.labels.labels
    copy = torch.empty_like(labels)
    us = _event_times(lambda: copy.copy_(labels), launches, dev)
    spread = lambda ms: {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}
    res = {'videos': NOVELTY_VIDEOS, 'n_points': NOVELTY_K, 'classes': NOVELTY_CLASSES, 'windows': w, 'candidates': 2 * w,
           'label_rows': int(store.labels.index.label_rows.sum()), 'store_mb': round(labels.numel() * 4 / 1e6, 1),
           'blocks_of_64': int(store.order.numel() // 64),
           'device_copy_of_store': dict(spread([v / 1e3 for v in us]), launches=launches,
                                        gb_per_s=round(2 * labels.numel() * 4 / (statistics.median(us) * 1e-6) / 1e9, 1))}
    g = torch.Generator(device=dev).manual_seed(9)
    for q, reps, torch_reps in ((64, launches, 3), (1024, max(3, launches // 4), 1)):
        queries = torch.rand((q, 32, NOVELTY_K, 2), generator=g, device=dev) * 2 - 1
        d2 = torch.empty((q, NOVELTY_CLASSES), dtype=torch.float64, device=dev)
        code = torch.empty((q, NOVELTY_CLASSES), dtype=torch.int32, device=dev)
        from kpx_amd import ops
        search = lambda: ops.seq_nearest(labels, store.labels.label_off, store.table, store.order, store.group_first, queries, out=(d2, code))
        ms = [v / 1e3 for v in _event_times(search, reps, dev)]
        fmas = 4.0 * n * 2 * w * q / 2                   # per point, window and query: ex^2, ey^2 plain and mirrored
        entry = {'queries': q, 'kernel': dict(spread(ms), launches=reps, fp64_tfma_per_s=round(fmas / (statistics.median(ms) * 1e-3) / 1e12, 2))}
        _novelty_torch_route(store, queries[:16])
        torch.cuda.synchronize(dev)
        tms = []
        for _ in range(torch_reps):
            t0 = time.perf_counter()
            ref = _novelty_torch_route(store, queries)
            torch.cuda.synchronize(dev)
            tms.append((time.perf_counter() - t0) * 1e3)
        rel = float(((d2 - ref).abs() / ref).max())
        assert rel <= 1e-12 and bool((code >= 0).all()), rel
        entry['gather_and_torch_fp64'] = dict(spread(tms), runs=torch_reps, max_rel_difference_to_kernel=rel)
        entry['torch_over_kernel'] = round(statistics.median(tms) / statistics.median(ms), 1)
        res['q%d' % q] = entry
    return res, store


def novelty_rollout_leg(dev, rollouts, store):
    import kpx_amd
    from kpx_amd import ops
    cfg = {'model': {'n_pts': NOVELTY_K, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    queries = torch.rand((2, B, 32, NOVELTY_K, 2), generator=g, device=dev) * 2 - 1          # slot 0: the real futures
    exclude = torch.randint(0, NOVELTY_VIDEOS, (2 * B,), generator=g, device=dev).to(torch.int32)
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    for _ in range(3):                                    # eager, capture, one replay
        o = fm.run(None, feed, z=z)
    store.nearest(queries.view(2 * B, 32, NOVELTY_K, 2), True, exclude)
    torch.cuda.synchronize(dev)
    ms = {False: [], True: []}
    for _ in range(rollouts):
        for score in (False, True):
            t0 = time.perf_counter()
            o = fm.run(None, feed, z=z)
            if score:
                ops.flat_copy_tensor(o['fut_pt_raw'].contiguous(), queries[1].data_ptr())
                d2, code = store.nearest(queries.view(2 * B, 32, NOVELTY_K, 2), True, exclude)
            torch.cuda.synchronize(dev)
            ms[score].append((time.perf_counter() - t0) * 1e3)
    assert bool((code >= 0).all())
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'n_points': NOVELTY_K, 'queries_per_rollout': 2 * B, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 1,
            'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'overhead_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


PRDC_REAL, PRDC_FAKE, PRDC_K, PRDC_DIMS = 1024, 4096, 5, (2560, 256)


def _prdc_rows(dev, n, m, d, seed):
    """clustered rows (a 2-d latent of four unit Gaussians through a random map, plus noise), float32 values held in fp64: real rows from
    three of the centres, generated rows from three, two shared"""
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.tensor([[0.0, 0.0], [6.0, 0.0], [0.0, 6.0], [6.0, 6.0]], device=dev)
    proj = torch.randn((2, d), generator=g, device=dev) / 2 ** 0.5

    def draw(count, allowed):
        c = torch.tensor(allowed, device=dev)[torch.randint(0, len(allowed), (count,), generator=g, device=dev)]
        z = centres[c] + torch.randn((count, 2), generator=g, device=dev)
        return (z @ proj + 0.01 * torch.randn((count, d), generator=g, device=dev)).float().double().contiguous()
    return draw(n, (0, 1, 2)), draw(m, (0, 1, 3))


def _prdc_torch_route(real, fake, k, mode):
    """The four scores by the route the kernel replaces: torch.cdist in fp64, topk, comparisons (distances, not squares: the same order)"""
    def cdist(a, b):                                      # 1 024 rows a call: the direct mode's launch takes fewer than 2^24 pairs
        return torch.cat([torch.cdist(a[lo:lo + 1024], b, compute_mode=mode) for lo in range(0, a.shape[0], 1024)])

    def radius(x):
        d = cdist(x, x)
        d.fill_diagonal_(float('inf'))
        return d.topk(k, dim=1, largest=False).values[:, k - 1]
    rr, fr = radius(real), radius(fake)
    d = cdist(fake, real)                                                            # [m, n]
    fake_inside = (d <= rr[None, :]).sum(dim=1)
    real_inside = (d <= fr[:, None]).sum(dim=0)
    return {'precision': (fake_inside > 0).double().mean(), 'recall': (real_inside > 0).double().mean(),
            'density': fake_inside.sum().double() / torch.tensor(float(k * fake.shape[0]), dtype=torch.float64, device=d.device),   # a tensor: a true division, not a multiplication by 1 / (k m)
            'coverage': (d.min(dim=0).values <= rr).double().mean()}


def prdc_kernel_leg(dev, launches):
    from kpx_amd import ops
    spread = lambda ms: {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}
    n, m, k = PRDC_REAL, PRDC_FAKE, PRDC_K
    res = {'n_real': n, 'n_fake': m, 'k': k}
    for d in PRDC_DIMS:
        real, fake = _prdc_rows(dev, n, m, d, 17 + d)
        copy_r, copy_f = torch.empty_like(real), torch.empty_like(fake)
        us = _event_times(lambda: (copy_r.copy_(real), copy_f.copy_(fake)), launches, dev)
        entry = {'dim': d, 'rows_mb': round((n + m) * d * 8 / 1e6, 1),
                 'device_copy_of_rows': dict(spread([v / 1e3 for v in us]), launches=launches,
                                             gb_per_s=round(2 * (n + m) * d * 8 / (statistics.median(us) * 1e-6) / 1e9, 1))}
        ms = [v / 1e3 for v in _event_times(lambda: ops.prdc(real, fake, k), launches, dev)]
        fmas = float(d) * (n * n + m * m + 2 * n * m)
        entry['prdc'] = dict(spread(ms), launches=launches, fp64_tfma_per_s=round(fmas / (statistics.median(ms) * 1e-3) / 1e12, 2))
        got = ops.prdc(real, fake, k)
        skip_r, skip_f = (torch.arange(c, dtype=torch.int32, device=dev) for c in (n, m))
        searches = (('real_radii', real, real, k, skip_r, None), ('fake_radii', fake, fake, k, skip_f, None),
                    ('fake_in_real_balls', fake, real, 1, None, got['real_radius2']), ('real_in_fake_balls', real, fake, 1, None, got['fake_radius2']))
        entry['searches'] = {}
        for name, q, r, kk, skip, rad in searches:
            one = [v / 1e3 for v in _event_times(lambda: ops.set_neighbours(q, r, kk, q_skip=skip, r_radius2=rad), launches, dev)]
            pairs = float(d) * q.shape[0] * r.shape[0]
            entry['searches'][name] = dict(spread(one), queries=q.shape[0], refs=r.shape[0], k=kk,
                                           fp64_tfma_per_s=round(pairs / (statistics.median(one) * 1e-3) / 1e12, 2))
        scores = {s: float(got[s]) for s in ('precision', 'recall', 'density', 'coverage')}
        entry['scores'] = scores
        for label, mode in (('torch_cdist_default', 'use_mm_for_euclid_dist_if_necessary'), ('torch_cdist_direct', 'donot_use_mm_for_euclid_dist')):
            tms = [v / 1e3 for v in _event_times(lambda: _prdc_torch_route(real, fake, k, mode), max(3, launches // 4), dev)]
            ref = {s: float(v) for s, v in _prdc_torch_route(real, fake, k, mode).items()}
            entry[label] = dict(spread(tms), launches=max(3, launches // 4), scores_equal_kernel=ref == scores, scores=ref,
                                kernel_over_torch=round(statistics.median(ms) / statistics.median(tms), 2))
        res['d%d' % d] = entry
    return res


def prdc_rollout_leg(dev, rollouts):
    import kpx_amd
    cfg = {'model': {'n_pts': NOVELTY_K, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    for _ in range(3):                                    # eager, capture, one replay
        o = fm.run(None, feed, z=z)
    torch.cuda.synchronize(dev)
    ms, kept = {False: [], True: []}, []
    for _ in range(rollouts):
        for on in (False, True):
            t0 = time.perf_counter()
            o = fm.run(None, feed, z=z)
            if on:                                        # evaluate._Prdc._rows: the draw's key points as float32 rows, kept until the end
                kept.append(o['fut_pt_raw'].reshape(B, -1).to(torch.float32).clone())
            torch.cuda.synchronize(dev)
            ms[on].append((time.perf_counter() - t0) * 1e3)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'n_points': NOVELTY_K, 'row_values': int(kept[0].shape[1]), 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 1,
            'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'overhead_pct': round(100 * (on - off) / off, 2),
            'off_ms_all': [round(v, 2) for v in ms[False]], 'on_ms_all': [round(v, 2) for v in ms[True]]}


def long_kernel_leg(dev, launches):
    from kpx_amd import ops
    g = torch.Generator(device=dev).manual_seed(9)
    n, f = 96, 4
    res = {'batch': B, 'knots': n, 'rate': f, 'launches': launches}
    stats = lambda us: {'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1)}
    for k in (15, 40):
        first = torch.rand((B, k, 2), generator=g, device=dev) * 1.6 - 0.8
        seq = torch.rand((B, n, k, 2), generator=g, device=dev) * 1.6 - 0.8
        out = torch.empty((B, n * f, k, 2), dtype=torch.float32, device=dev)
        dst = torch.empty_like(out)
        leg = {'out_shape': [B, n * f, k, 2], 'out_kb': round(out.numel() * 4 / 1e3, 1)}
        for mode in ('linear', 'cubic'):
            leg['resample_' + mode] = stats(_event_times(lambda: ops.points_resample(first, seq, f, mode, out=out), launches, dev))
            assert bool(torch.isfinite(out).all())
        leg['speed'] = stats(_event_times(lambda: ops.points_speed(first, out, float(f)), launches, dev))
        leg['device_copy_of_out'] = stats(_event_times(lambda: dst.copy_(out), launches, dev))
        res['k%d' % k] = leg
    return res


def long_rollout_leg(dev, rollouts):
    import kpx_amd
    cfg = {'model': {'n_pts': 15, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((3, B, 64), generator=g, device=dev)
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256)
    fm.build()
    feed = {'image': im, 'action_code': act}
    plain = lambda: fm.run(None, feed, z=z[0])
    runs = {'plain_x3': lambda: [plain() for _ in range(3)][-1], 'frames_96': lambda: fm.run(None, feed, z=z, frames=96),
            'plain_x4': lambda: [plain() for _ in range(4)][-1], 'rate_4': lambda: fm.run(None, feed, z=z[0], rate=4)}
    for fn in (plain, runs['frames_96'], runs['rate_4']):
        for _ in range(3):                                # eager, capture, one replay
            out = fn()
        assert bool(torch.isfinite(out['pred_im_seq']).all())
    torch.cuda.synchronize(dev)
    ms = {name: [] for name in runs}
    for _ in range(rollouts):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    med = {name: statistics.median(v) for name, v in ms.items()}
    res = {'batch': B, 'n_points': 15, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 3 and not fm._graph_failed}
    for name in runs:
        res[name] = {'ms': round(med[name], 3), 'ms_all': [round(v, 2) for v in ms[name]]}
    res['frames_96_over_plain_x3'] = round(med['frames_96'] / med['plain_x3'], 4)
    res['rate_4_over_plain_x4'] = round(med['rate_4'] / med['plain_x4'], 4)
    return res


def posterior_kernel_leg(dev, launches):
    from kpx_amd import ops, posterior
    g = torch.Generator(device=dev).manual_seed(11)
    v, groups, steps = 64, 9, 8
    logit = torch.rand((B, 2 * v), generator=g, device=dev)
    eps = torch.randn((B, v), generator=g, device=dev)
    group = torch.randint(0, groups, (B,), generator=g, device=dev).to(torch.int32)
    state, counts = posterior.new_state(groups, v, dev)
    rows, z = torch.empty(B, dtype=torch.float64, device=dev), torch.empty((B, v), device=dev)
    path, dst = torch.empty((steps, B, v), device=dev), torch.empty_like(logit)
    stats = lambda us: {'median_us': round(statistics.median(us), 1), 'min_us': round(min(us), 1), 'max_us': round(max(us), 1)}
    res = {'batch': B, 'vae_dim': v, 'groups': groups, 'path_steps': steps, 'launches': launches, 'logit_kb': round(logit.numel() * 4 / 1e3, 1)}
    res['stats_add'] = stats(_event_times(lambda: ops.latent_stats_add(logit, state, counts, group, kl_rows=rows), launches, dev))
    res['sample'] = stats(_event_times(lambda: ops.latent_sample(logit, eps, 1.0, out=z), launches, dev))
    res['path_slerp'] = stats(_event_times(lambda: ops.latent_path(z, eps, steps, 'slerp', out=path), launches, dev))
    res['device_copy_of_logit'] = stats(_event_times(lambda: dst.copy_(logit), launches, dev))
    assert bool(torch.isfinite(state).all()) and bool(torch.isfinite(path).all()) and int(counts[:, 0].sum()) > 0
    return res


def posterior_rollout_leg(dev, rollouts):
    """encode at B = 64, K = 40, and the configs[4] rollout without and with what --posterior adds per batch: one encode, one
    latent_stats_add, the copy of the logit rows, z = mu and one more rollout"""
    import kpx_amd
    from kpx_amd import ops, posterior
    k = NOVELTY_K
    cfg = {'model': {'n_pts': k, 'cell_info': [1024, 1024], 'vae_dim': 64, 'n_action': 9}, 'paths': {'log_dir': '/tmp/kpx_bench'}}
    g = torch.Generator(device=dev).manual_seed(7)
    im = torch.rand((B, RES, RES, 3), generator=g, device=dev) * 2 - 1
    act = torch.eye(9, device=dev)[torch.randint(0, 9, (B,), generator=g, device=dev)]
    z = torch.randn((B, 64), generator=g, device=dev)
    kp = torch.rand((B, k, 2), generator=g, device=dev) * 1.6 - 0.8
    seq = torch.rand((B, 32, k, 2), generator=g, device=dev) * 1.6 - 0.8
    feed = {'image': im, 'action_code': act}
    fm = kpx_amd.FinalModel(cfg, device=dev, image_size=RES, frames_per_launch=256, posterior=True)
    fm.build()
    state, counts = posterior.new_state(9, 64, dev)
    group = act.argmax(dim=1).to(torch.int32)
    for _ in range(3):                                    # eager, capture, one replay
        fm.run(None, feed, z=z)
        fm.encode(kp, seq, act)
    torch.cuda.synchronize(dev)
    enc = []
    for _ in range(max(rollouts, 10)):
        t0 = time.perf_counter()
        fm.encode(kp, seq, act)
        torch.cuda.synchronize(dev)
        enc.append((time.perf_counter() - t0) * 1e3)
    ms, kept = {False: [], True: []}, []
    for _ in range(rollouts):
        for on in (False, True):
            t0 = time.perf_counter()
            fm.run(None, feed, z=z)
            if on:                                        # evaluate._Posterior.end_batch without the files
                logit = fm.encode(kp, seq, act)
                ops.latent_stats_add(logit, state, counts, group)
                kept.append(logit.clone())
                fm.run(None, feed, z=ops.latent_sample(logit, None, 0.0))
            torch.cuda.synchronize(dev)
            ms[on].append((time.perf_counter() - t0) * 1e3)
    off, on = statistics.median(ms[False]), statistics.median(ms[True])
    return {'batch': B, 'n_points': k, 'rollouts_each': rollouts, 'graph_replay': len(fm._graphs) == 2 and not fm._graph_failed,
            'encode_ms': round(statistics.median(enc), 3), 'encode_ms_all': [round(x, 3) for x in enc],
            'off_ms': round(off, 3), 'on_ms': round(on, 3), 'delta_ms': round(on - off, 3), 'on_over_off': round(on / off, 4),
            'off_ms_all': [round(x, 2) for x in ms[False]], 'on_ms_all': [round(x, 2) for x in ms[True]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rollouts', type=int, default=10)
    ap.add_argument('--vgg', action='store_true', help='measure the VGG feature-space metrics instead of the frame metrics')
    ap.add_argument('--motion', action='store_true', help='measure the motion metrics (draw diversity, key-point error) instead')
    ap.add_argument('--actions', action='store_true', help='measure the class sweep (contact-sheet paste, sheets and class scores) instead')
    ap.add_argument('--drive', action='store_true', help='measure the driven rollout (key-point retargeting, every drive mode) instead')
    ap.add_argument('--frechet', action='store_true', help="measure the Fréchet distance's pooling and moment kernels and its cost per rollout instead")
    ap.add_argument('--classifier', action='store_true',
                    help="measure the action classifier's loss and score launches and the cost of --action-accuracy per rollout instead")
    ap.add_argument('--stability', action='store_true',
                    help="measure the detector's equivariance score (the affine warp, the score launch, the cost of stability() per video) instead")
    ap.add_argument('--joints', action='store_true',
                    help='measure the landmark regression (its three launches, the cost of JointRegression per video) instead')
    ap.add_argument('--gif', action='store_true',
                    help='measure the animated GIFs (the colour histogram and palette-map kernels, the host route, the cost of --gif per rollout) instead')
    ap.add_argument('--animate', action='store_true',
                    help="measure animate.py's grids (the cell kernel without and with markers, the route it replaces, the cost per still) instead")
    ap.add_argument('--guard', action='store_true',
                    help="measure the step guard (the health pass, the guarded update and the restore on the two real buckets, the configs[1] train "
                         'step with guard off and on) instead')
    ap.add_argument('--ema', action='store_true',
                    help="measure the averaged generator (the update and the swap on the real 'G' bucket beside a device copy, the configs[1] "
                         'train step with ema off and on) instead')
    ap.add_argument('--clip', action='store_true',
                    help='measure gradient clipping (the clipped update beside the guarded update and a device copy, the per-variable statistics '
                         'on the two real buckets, the configs[1] train step guarded without and with clip_norm, all in this process) instead')
    ap.add_argument('--novelty', action='store_true',
                    help='measure the nearest-motion search (the kernel on a Penn-sized synthetic store beside a device copy and the gather + torch '
                         'fp64 route, the cost of --novelty per configs[4] rollout, all in this process) instead')
    ap.add_argument('--long', action='store_true',
                    help='measure the longer and smoother rollouts (the resample and speed launches beside a device copy, a 96-frame rollout beside '
                         'three 32-frame ones and a rate-4 rollout beside four, all in this process) instead')
    ap.add_argument('--prdc', action='store_true',
                    help='measure precision / recall / density / coverage (ops.prdc and its four searches at Penn\'s test-set size beside a device '
                         'copy and the torch.cdist fp64 route, the cost of --prdc per configs[4] rollout, all in this process) instead')
    ap.add_argument('--video', action='store_true',
                    help='measure the Motion-JPEG AVIs of rollouts (the JPEG coder beside a device copy and the host PIL route, the cost of '
                         '--video per configs[4] rollout beside --gif, all in this process) instead')
    ap.add_argument('--posterior', action='store_true',
                    help='measure the posterior tools (the three latent launches beside a device copy, FinalModel.encode at B = 64, K = 40, the cost '
                         'of --posterior per configs[4] rollout, all in this process) instead')
    args = ap.parse_args()
    if args.posterior:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        kernels = posterior_kernel_leg(dev, args.launches)
        print(json.dumps({'posterior_kernels': kernels, 'posterior_rollout_c4': posterior_rollout_leg(dev, args.rollouts)}))
        return
    if args.video:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        kernels = video_kernel_leg(dev, min(args.launches, 10))
        torch.cuda.empty_cache()
        print(json.dumps({'video_kernels': kernels, 'video_rollout_c4': video_rollout_leg(dev, args.rollouts)}))
        return
    if args.prdc:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        kernels = prdc_kernel_leg(dev, args.launches)
        torch.cuda.empty_cache()
        print(json.dumps({'prdc_kernels': kernels, 'prdc_rollout_c4': prdc_rollout_leg(dev, args.rollouts)}))
        return
    if args.long:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        kernels = long_kernel_leg(dev, args.launches)
        print(json.dumps({'long_kernels': kernels, 'long_rollout_c4': long_rollout_leg(dev, args.rollouts)}))
        return
    if args.novelty:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        kernels, store = novelty_kernel_leg(dev, args.launches)
        torch.cuda.empty_cache()
        print(json.dumps({'novelty_kernels': kernels, 'novelty_rollout_c4': novelty_rollout_leg(dev, args.rollouts, store)}))
        return
    if args.clip:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        step, model = clip_step_leg(dev, max(args.rollouts, 10))
        torch.cuda.empty_cache()
        print(json.dumps({'clip_kernels': clip_kernel_leg(dev, args.launches, model), 'clip_step_c1': step}))
        return
    if args.ema:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        step, n = ema_step_leg(dev, max(args.rollouts, 10))
        torch.cuda.empty_cache()
        print(json.dumps({'ema_kernels': ema_kernel_leg(dev, args.launches, n), 'ema_step_c1': step}))
        return
    if args.guard:
        if not torch.cuda.is_available():
            raise SystemExit('bench_metrics.py needs the MI355X')
        dev = torch.device('cuda:0')
        step, sizes = guard_step_leg(dev, max(args.rollouts, 10))
        torch.cuda.empty_cache()
        print(json.dumps({'guard_kernels': guard_kernel_leg(dev, args.launches, sizes), 'guard_step_c1': step}))
        return
    if (args.vgg + args.motion + args.actions + args.drive + args.frechet + args.classifier + args.stability + args.joints + args.gif
            + args.animate > 1):
        ap.error('--vgg, --motion, --actions, --drive, --frechet, --classifier, --stability, --joints, --gif and --animate are ten '
                 'measurements: pass one')
    if not torch.cuda.is_available():
        raise SystemExit('bench_metrics.py needs the MI355X')
    dev = torch.device('cuda:0')
    if args.animate:
        res = {'animate_kernels': animate_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['animate_stills'] = animate_stills_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.gif:
        res = {'gif_kernels': gif_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['gif_rollout_c4'] = gif_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.vgg:
        res = {'vgg_kernel': vgg_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['vgg_rollout_c4'] = vgg_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.stability:
        res = {'stability_kernels': stability_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['stability_video'] = stability_video_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.joints:
        res = {'joints_kernels': joints_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['joints_video'] = joints_video_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.classifier:
        res = {'classifier_kernels': classifier_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['classifier_rollout_c4'] = classifier_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.frechet:
        res = {'frechet_kernels': frechet_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['frechet_rollout_c4'] = frechet_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.actions:
        res = {'actions_kernels': actions_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['actions_rollout_c4'] = actions_rollout_leg(dev, args.rollouts)
        print(json.dumps(res))
        return
    if args.drive:
        res = {'drive_kernel': drive_kernel_leg(dev, args.launches)}
        torch.cuda.empty_cache()
        res['drive_rollout_c4'] = drive_rollout_leg(dev, args.rollouts)
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
