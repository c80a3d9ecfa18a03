"""Throughput of the image-pair input pipeline (kpx_amd.data) on Penn-Action-sized synthetic JPEG frames (480x270):
pairs/s of the threaded decode + augment + pinned H2D + on-device conversion -- or, with --resident, of the HIP augmentation on frames
kept in HBM -- alone and feeding the train step, next to the same train-step loop on ONE fixed device batch of the same process.
Every window is warmed up and at least a second long.  KPX_DTYPE=bf16 selects the bf16 configuration as everywhere.

--motion measures stage 2 instead (kpx_amd.data.SequenceDataLoader, K = 40 pseudo labels on 480x270 videos of 40 / 70 / 100 frames, the
motion generator at the reference's size): sequences/s at batch 16 and 64 of the loader alone -- the host threads, or with --resident
the key-point kernel on labels kept in HBM -- of the train step on one fixed device batch, and of the train step fed by the loader.
Run it once without and once with --resident in the same session to compare the two loaders.

--image-size S runs everything at S x S frames (default 128; --points K sets the model's key points, so --image-size 256 --points 40
--batch 16 is the shape of bench.py --config c3).  --resident --launches times the two augmentation launches of one fixed batch by
themselves, in alternating blocks: the entries that take the side as an argument, at 128 the compile-time entries of the same process
beside them, and a device copy of their output for scale."""
import argparse, io, os, sys, tempfile, time
import numpy as np
import torch
from PIL import Image
ROOT = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, ROOT)


def make_dataset(root, videos=8, frames=40, w=480, h=270):
    rs = np.random.RandomState(0)
    for v in range(videos):
        os.makedirs(os.path.join(root, '%04d' % v))
        low = rs.rand(h // 16 + 2, w // 16 + 2, 3)
        bg = np.asarray(Image.fromarray((low * 255).astype(np.uint8)).resize((w, h), Image.BILINEAR)).astype(np.float32)
        for i in range(frames):
            img = np.clip(bg + rs.randn(h, w, 3) * 6 + i, 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, '%04d' % v, '%06d.jpg' % (i + 1)), format='JPEG', quality=90)
    with open(os.path.join(root, 'train_set.txt'), 'w') as f:
        f.write(''.join('%04d 0\n' % v for v in range(videos)))


def make_motion_dataset(root, videos=12, lengths=(40, 70, 100), k=40, n_action=9, w=480, h=270):
    """Penn-shaped stage-2 data: frames/NNNN/*.jpg (eight distinct pictures per video, repeated), pseudo_labels/NNNN.npy float32 [len, k, 2];
    40 / 70 / 100 frames give SequenceDataLoader's gap 1 / 2 / 3."""
    rs = np.random.RandomState(0)
    os.makedirs(os.path.join(root, 'pseudo_labels'))
    lines = []
    for v in range(videos):
        n, name = lengths[v % len(lengths)], 'frames/%04d' % (v + 1)
        os.makedirs(os.path.join(root, name))
        low = rs.rand(h // 16 + 2, w // 16 + 2, 3)
        bg = np.asarray(Image.fromarray((low * 255).astype(np.uint8)).resize((w, h), Image.BILINEAR)).astype(np.float32)
        jpegs = []
        for i in range(8):
            buf = io.BytesIO()
            Image.fromarray(np.clip(bg + rs.randn(h, w, 3) * 6 + 4 * i, 0, 255).astype(np.uint8)).save(buf, format='JPEG', quality=90)
            jpegs.append(buf.getvalue())
        for i in range(n):
            with open(os.path.join(root, name, '%06d.jpg' % (i + 1)), 'wb') as f:
                f.write(jpegs[i % 8])
        np.save(os.path.join(root, 'pseudo_labels', '%04d.npy' % (v + 1)), (rs.rand(n, k, 2) * 1.6 - 0.8).astype(np.float32))
        lines.append('%s %d\n' % (name, v % n_action))
    with open(os.path.join(root, 'train_set.txt'), 'w') as f:
        f.write(''.join(lines))


def motion(a):
    """The --motion mode: every figure in sequences/s, batch 16 then 64."""
    import kpx_amd
    dev = torch.device('cuda', 0)
    k, n_action = 40, 9
    what = 'resident labels' if a.resident else 'CPU pipeline, %d threads' % a.threads
    with tempfile.TemporaryDirectory() as root:
        make_motion_dataset(root, k=k, n_action=n_action)
        for b in (16, 64):
            loader = kpx_amd.SequenceDataLoader(root, 'train', n_points=k, n_action=n_action, random_order=True, randomness=True)
            if a.resident:
                t0 = time.perf_counter()
                store = loader.resident_labels(dev)
                torch.cuda.synchronize()
                print('resident label store: %d videos, %d bytes read and copied in %.3f s'
                      % (len(store.index.names), store.index.labels.nbytes, time.perf_counter() - t0))
            it = iter(loader.batches(b, dev, repeat=True, num_preprocess_threads=a.threads, resident=a.resident))
            for _ in range(3): next(it)
            print('stage-2 loader alone (%s): %.0f sequences/s (batch %d)' % (what, timed(lambda i: next(it), b, a.batches), b))
            cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': b},
                   'model': {'n_pts': k, 'n_action': n_action, 'cell_info': [1024, 1024], 'vae_dim': 64}, 'paths': {'log_dir': '/tmp/kpx_motion'}}
            model = kpx_amd.MotionGeneratorModel(cfg, device=dev); model.build()
            fixed = {key: v.clone() for key, v in next(it).items() if key != 'image'}
            steps = [0]

            def fed(i):
                model.train_step(None, next(it), steps[0], b); steps[0] += 1

            def on_fixed(i):
                model.train_step(None, fixed, steps[0], b); steps[0] += 1
            for i in range(3): fed(i)
            for rep in range(2):                       # alternated: the spread between the repetitions is the noise of this session
                for i in range(3): on_fixed(i)
                print('stage-2 train step on one fixed device batch [%d]: %.0f sequences/s (batch %d)' % (rep, timed(on_fixed, b, a.batches), b))
                for i in range(3): fed(i)
                print('stage-2 train step fed by the loader (%s) [%d]: %.0f sequences/s (batch %d)' % (what, rep, timed(fed, b, a.batches), b))


def launches(a, loader, store, dev, blocks=5):
    """--resident --launches: microseconds per batch of the geometry + filter launches on one fixed row table, per block."""
    from kpx_amd import resident as R
    from kpx_amd._lib import lib, check
    s, n = store.image_size, 2 * a.batch
    plans = [p for _ in range(a.batch // max(1, loader.length()) + 1) for p in loader.plans()][:a.batch]
    rows_dev = torch.from_numpy(store.check_rows(store.rows_for_plans(plans, True))).to(dev)
    out, out2 = (torch.empty((n, s, s, 3), dtype=torch.float32, device=dev) for _ in range(2))
    tiles = torch.empty((n, s, s, 3), dtype=torch.uint8, device=dev)
    lsum = torch.empty((n, R.BANDS), dtype=torch.int32, device=dev)

    def by_argument(i):
        store.augment(rows_dev, n, out=out)

    def compile_time(i):                           # kpx_augment_geometry_u8 / kpx_augment_filter_f32: side 128 only
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib.kpx_augment_geometry_u8(store.frames.data_ptr(), store.frame_off.data_ptr(), rows_dev.data_ptr(), n, store.resize_tabs.data_ptr(),
                                          store.band_rows_cap, tiles.data_ptr(), lsum.data_ptr(), stream), 'kpx_augment_geometry_u8')
        check(lib.kpx_augment_filter_f32(tiles.data_ptr(), lsum.data_ptr(), rows_dev.data_ptr(), n, store.kernels.data_ptr(), out2.data_ptr(), stream),
              'kpx_augment_filter_f32')

    def copy(i):
        out2.copy_(out)
    forms = [('side as an argument', by_argument)] + ([('side 128 at compile time', compile_time)] if s == 128 else []) + [('device copy of the output', copy)]
    for _, f in forms:
        for i in range(20): f(i)
    if s == 128:
        torch.cuda.synchronize()
        assert torch.equal(out, out2), 'the two forms of the launches disagree'
    for block in range(blocks):
        for name, f in forms:
            print('launches of one batch of %d pairs at %d x %d, %s [%d]: %.1f us'
                  % (a.batch, s, s, name, block, 1e6 * a.batch / timed(f, a.batch, 200, min_seconds=0.5)))


def timed(step, batch, batches, min_seconds=1.0):
    """pairs/s of ``step(i)`` over a window of at least ``batches`` calls and ``min_seconds`` (the caller has warmed up)."""
    n = 0
    torch.cuda.synchronize(); t0 = time.perf_counter()
    while True:
        for _ in range(batches): step(n); n += 1
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if dt >= min_seconds: return batch * n / dt


def main():
    ap = argparse.ArgumentParser(); ap.add_argument('--batch', type=int, default=32); ap.add_argument('--batches', type=int, default=40)
    ap.add_argument('--threads', type=int, default=12); ap.add_argument('--train', action='store_true')
    ap.add_argument('--resident', action='store_true', help='frames decoded once into HBM, augmentation in HIP (batches(resident=True))')
    ap.add_argument('--frames', type=int, default=40, help='frames per synthetic video (8 videos)')
    ap.add_argument('--motion', action='store_true', help='stage 2: the sequence loader and the motion generator step (batch 16 and 64); '
                                                          'with --resident the key-point labels are kept in HBM')
    ap.add_argument('--image-size', type=int, default=128, metavar='S', help='side of the frames (a multiple of 16 in [32, 256], default 128)')
    ap.add_argument('--points', type=int, default=15, metavar='K', help='key points of the --train model (default 15; bench.py --config c3 has 40)')
    ap.add_argument('--launches', action='store_true', help='with --resident: time the two augmentation launches of one fixed batch alone')
    a = ap.parse_args()
    if a.motion:
        return motion(a)
    import kpx_amd
    dev = torch.device('cuda', 0)
    with tempfile.TemporaryDirectory() as root:
        make_dataset(root, frames=a.frames)
        loader = kpx_amd.ImagePairDataLoader(root, 'train', random_order=True, randomness=True, image_size=a.image_size)
        if a.resident:
            store = loader.resident_frames(dev)
            print('resident store: %d frames, %d bytes (%.1f MiB) ingested in %.2f s (%.0f frames/s, header scan + decode + copy)'
                  % (len(store.index.offsets), store.index.total_bytes, store.index.total_bytes / 2.0 ** 20, store.ingest_seconds,
                     len(store.index.offsets) / store.ingest_seconds))
            what = 'resident path'
            if a.launches:
                launches(a, loader, store, dev)
        else:
            what = 'CPU pipeline, %d threads' % a.threads
        it = iter(loader.batches(a.batch, dev, num_preprocess_threads=a.threads, resident=a.resident))
        for _ in range(3): next(it)
        print('input pipeline alone (%s): %.0f pairs/s (batch %d, %d x %d)'
              % (what, timed(lambda i: next(it), a.batch, a.batches), a.batch, a.image_size, a.image_size))
        if a.train:
            cfg = {'training': {'lr': {'start_val': 1e-4, 'step': 20000, 'decay': 0.95}, 'batch_size': a.batch}, 'model': {'n_pts': a.points},
                   'paths': {'log_dir': '/tmp/kpx_bench', 'vggnet': None}}
            vgg = kpx_amd.Vgg19(weights=kpx_amd.synthetic_vgg19_weights(seed=19), device=dev)
            model = kpx_amd.DetectorTranslatorModel(cfg, device=dev, vgg=vgg, image_size=a.image_size); model.build()
            fixed = {k: v.clone() for k, v in next(it).items()}
            steps = [0]

            def fed(i):
                model.train_step(None, next(it), steps[0], a.batch); steps[0] += 1

            def on_fixed(i):
                model.train_step(None, fixed, steps[0], a.batch); steps[0] += 1
            for i in range(3): fed(i)
            for rep in range(2):                       # alternated: the spread between the repetitions is the noise of this session
                for i in range(3): on_fixed(i)
                print('train step on one fixed device batch [%d]: %.0f pairs/s' % (rep, timed(on_fixed, a.batch, a.batches)))
                for i in range(3): fed(i)
                print('train step fed by the pipeline (%s) [%d]: %.0f pairs/s' % (what, rep, timed(fed, a.batch, a.batches)))


if __name__ == '__main__':
    main()
