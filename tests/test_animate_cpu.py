"""CPU: animate.py without a GPU -- the fit of a still against the sequence loader's start frame byte for byte (sizes, modes, EXIF
orientation, a box), the listing of files, directories and manifests, the marker restatement (cells_ref.py) against a float64 evaluation of
its inequality and its rules, every refusal of animate.py's parser, and the argument checks of kpx_cell_frames_u8_f32."""
import ctypes
import os

import numpy as np
import pytest

import cells_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stills():
    from kpx_amd import stills
    return stills


def _picture(w, h, seed):
    """a smooth picture with detail: gradients, a few blocks, mild noise (JPEG keeps it near)"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([255.0 * x / max(1, w - 1), 255.0 * y / max(1, h - 1), 127.0 + 127.0 * np.sin(x / 9.0) * np.cos(y / 7.0)], axis=-1)
    a[h // 4:h // 2, w // 3:w // 2] = rs.randint(0, 256, size=3)
    return np.clip(a + rs.normal(0, 6, size=a.shape), 0, 255).astype(np.uint8)


def _loader_start_image(tmp_path, name, upright_rgb):
    """what SequenceDataLoader.render_start_image gives for a one-video dataset whose only frame holds exactly ``upright_rgb`` (a PIL
    image, or the path of a JPEG to take as it is)"""
    import shutil
    from kpx_amd.data import SequenceDataLoader
    data = tmp_path / ('data_' + name)
    video = data / 'frames' / '0001'
    video.mkdir(parents=True)
    target = str(video / '000001.jpg')
    if isinstance(upright_rgb, str):
        shutil.copyfile(upright_rgb, target)
    else:
        upright_rgb.save(target, format='PNG')                    # PIL opens by content: the loader reads these pixels without loss
    (data / 'test_set.txt').write_text('frames/0001 0\n')
    loader = SequenceDataLoader(str(data), 'test', n_points=5, n_action=3, random_order=False, randomness=False)
    return loader.render_start_image(loader.plan(0))


@pytest.mark.parametrize('w,h', [(128, 128), (129, 128), (128, 300), (301, 200), (1600, 1200)])
def test_fit_of_a_jpeg_is_the_loaders_start_frame(tmp_path, w, h):
    from PIL import Image
    S = _stills()
    path = str(tmp_path / 'still.jpg')
    Image.fromarray(_picture(w, h, w + h)).save(path, quality=92)
    got, info = S.fit(path)
    want = _loader_start_image(tmp_path, 'jpeg', path)
    assert got.dtype == np.uint8 and got.shape == (128, 128, 3) and np.array_equal(got, want)
    assert info['source'] == path and info['decoded_size'] == [w, h] and info['box'] is None
    assert min(info['resized_size']) == 128 and len(info['crop_box']) == 4


@pytest.mark.parametrize('mode', ['L', 'P', 'RGBA'])
def test_fit_of_other_modes_is_the_fit_of_their_rgb_conversion(tmp_path, mode):
    from PIL import Image
    S = _stills()
    rgb = Image.fromarray(_picture(150, 131, 7))
    if mode == 'RGBA':
        alpha = Image.fromarray((np.arange(150 * 131).reshape(131, 150) % 256).astype(np.uint8))
        im = rgb.copy()
        im.putalpha(alpha)
    elif mode == 'P':
        im = rgb.convert('P', palette=Image.ADAPTIVE, colors=64)
    else:
        im = rgb.convert('L')
    assert im.mode == mode
    path = str(tmp_path / 'still.png')
    im.save(path)
    got, _ = S.fit(path)
    want = _loader_start_image(tmp_path, mode, Image.open(path).convert('RGB'))            # alpha is dropped as convert drops it
    assert np.array_equal(got, want)
    if mode == 'RGBA':
        assert np.array_equal(got, S.fit_image(rgb)[0])


def test_fit_applies_exif_orientation_6(tmp_path):
    from PIL import Image
    S = _stills()
    stored = Image.fromarray(_picture(200, 150, 3))
    exif = Image.Exif()
    exif[0x0112] = 6                                                   # the stored rows are the upright image's columns: show rotated 90 degrees clockwise
    path = str(tmp_path / 'phone.jpg')
    stored.save(path, quality=95, exif=exif)
    decoded = np.asarray(Image.open(path))                             # the JPEG's own pixels, orientation ignored
    assert decoded.shape == (150, 200, 3)
    upright = Image.fromarray(np.ascontiguousarray(np.rot90(decoded, k=-1)))
    got, info = S.fit(path)
    assert info['decoded_size'] == [150, 200]
    assert np.array_equal(got, _loader_start_image(tmp_path, 'exif', upright))


def test_fit_with_a_box_is_the_fit_of_the_cropped_image(tmp_path):
    from PIL import Image
    S = _stills()
    path = str(tmp_path / 'wide.png')
    Image.fromarray(_picture(400, 260, 5)).save(path)
    box = (37, 11, 301, 250)
    got, info = S.fit(path, box)
    assert info['box'] == list(box) and info['decoded_size'] == [400, 260]
    assert np.array_equal(got, _loader_start_image(tmp_path, 'box', Image.open(path).convert('RGB').crop(box)))
    for bad in ((-1, 0, 10, 10), (0, 0, 401, 10), (0, 0, 10, 261), (5, 5, 6, 50), (5, 5, 50, 6), (50, 5, 5, 50)):
        with pytest.raises(S.StillsError):
            S.fit(path, bad)
    S.fit(path, (0, 0, 400, 260))
    S.fit(path, (398, 258, 400, 260))                                  # both sides exactly 2


def test_listing_files_directories_and_manifests(tmp_path):
    from PIL import Image
    S = _stills()
    folder = tmp_path / 'pics'
    (folder / 'sub').mkdir(parents=True)
    small = Image.fromarray(_picture(8, 8, 1))
    for name in ('b.PNG', 'a.jpg', 'c.jpeg', 'd.BmP', 'notes.txt', 'e.gif', 'sub/z.png'):
        p = folder / name
        if name.endswith('.txt'):
            p.write_text('x')
        else:
            small.save(str(p), format='PNG' if name.endswith('.gif') else None)
    got = S.list_images([str(folder)], box=(0, 0, 4, 4))
    assert [os.path.basename(p) for p, _ in got] == ['a.jpg', 'b.PNG', 'c.jpeg', 'd.BmP'] and all(b == (0, 0, 4, 4) for _, b in got)
    manifest = tmp_path / 'pics' / 'list.txt'
    manifest.write_text('# comment\nb.PNG 1,2,7,8\n\nsub/z.png\na.jpg\n')
    got = S.list_images([str(manifest), str(folder / 'c.jpeg')], box=(0, 0, 4, 4))
    assert [os.path.relpath(p, str(folder)) for p, _ in got] == ['b.PNG', os.path.join('sub', 'z.png'), 'a.jpg', 'c.jpeg']
    assert [b for _, b in got] == [(1, 2, 7, 8), (0, 0, 4, 4), (0, 0, 4, 4), (0, 0, 4, 4)]            # a manifest box overrides the flag
    assert S.list_images([str(manifest)])[1][1] is None
    empty = tmp_path / 'empty'
    empty.mkdir()
    for bad in ([str(empty)], [str(tmp_path / 'missing.jpg')], [str(folder), str(empty)]):
        with pytest.raises(S.StillsError):
            S.list_images(bad)
    (tmp_path / 'bad.txt').write_text('nowhere.jpg\n')
    with pytest.raises(S.StillsError):
        S.list_images([str(tmp_path / 'bad.txt')])
    (tmp_path / 'badbox.txt').write_text('pics/a.jpg 1,2,x,4\n')
    with pytest.raises(S.StillsError):
        S.list_images([str(tmp_path / 'badbox.txt')])


def test_driver_frames_follow_the_loaders_rule(tmp_path):
    S = _stills()
    folder = tmp_path / 'video'
    folder.mkdir()
    for i in range(70):
        (folder / ('%04d.png' % i)).write_bytes(b'')
    paths, idx, n = S.driver_frames(str(folder))
    assert n == 70 and idx == list(range(0, 66, 2)) and [os.path.basename(p) for p in paths] == ['%04d.png' % i for i in idx]
    os.remove(str(folder / '0069.png'))
    for i in range(33, 69):
        os.remove(str(folder / ('%04d.png' % i)))
    assert S.driver_frames(str(folder))[1] == list(range(33))
    os.remove(str(folder / '0000.png'))
    with pytest.raises(S.StillsError):
        S.driver_frames(str(folder))


def test_grid_limits_and_batch():
    S = _stills()
    S.check_grid(1, 31)
    S.check_grid(31, 1)
    S.check_grid(5, 6)
    for s, a in ((1, 32), (4, 8), (65, 1), (1, 65), (0, 1), (1, 0)):
        with pytest.raises(S.StillsError):
            S.check_grid(s, a)
    with pytest.raises(S.StillsError, match='2\\^24'):
        S.check_grid(2, 16)
    per_still = 33 * 128 * 128 * 3 * 2 * 9
    assert S.batch_under(8, per_still) == 8 and S.batch_under(64, per_still) == (1 << 30) // per_still and S.batch_under(8, 1 << 31) == 1
    assert S.batch_under(64, per_still) * per_still <= 1 << 30
    assert np.array_equal(S.marker_colors([[0.0, 1.0, 0.5], [0.999, 0.2, 1 / 255.0]]), [[0, 255, 127], [254, 51, 1]])
    assert np.array_equal(S.marker_colors([[0.3, 0.7, 0.11]]), R.quantise_colors([[0.3, 0.7, 0.11]]))


# ------------------------------------------------------------------------------------------------ the marker restatement
def test_the_restatements_disc_is_the_float64_inequality_away_from_ties():
    rs = np.random.RandomState(11)
    checked = 0
    while checked < 2000:
        h, w, r = int(rs.randint(1, 40)), int(rs.randint(1, 40)), int(rs.randint(1, 17))
        p = rs.uniform(-1.6, 1.6, size=2).astype(np.float32)
        exact = [(float(p[0]) + 1.0) * 0.5 * (16 * (w - 1)), (float(p[1]) + 1.0) * 0.5 * (16 * (h - 1))]
        if any(abs(abs(v - np.floor(v)) - 0.5) < 1e-3 for v in exact):
            continue                                                   # within float32 rounding of a tie: the float32 steps decide, not this test
        cx, cy = np.rint(exact[0]), np.rint(exact[1])
        assert R.centre16(p[0], w) == int(cx) and R.centre16(p[1], h) == int(cy)
        py, px = np.mgrid[0:h, 0:w].astype(np.float64)
        d2 = (16.0 * px - cx) ** 2 + (16.0 * py - cy) ** 2
        covered, who, inner = R.marker_layers(p[None], h, w, r)
        assert np.array_equal(covered, d2 <= (16.0 * r) ** 2) and np.array_equal(inner, d2 <= (16.0 * (r - 1)) ** 2)
        checked += 1


def test_the_restatements_ties_round_to_even():
    n = np.arange(0, 40)
    x = ((n + 0.5) / 128.0 - 1.0).astype(np.float32)                   # W = 17: exactly n + 0.5 sixteenths
    assert np.array_equal(R.centre16(x, 17), n + (n % 2))


def test_the_restatements_rules():
    colors = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    base = np.full((17, 17, 3), 99, np.uint8)
    f = R.draw_markers(base.copy(), np.array([(0.0, 0.0), (0.0, 0.0), (0.25, 0.0)], np.float32), colors, 3)
    assert tuple(f[8, 8]) == (10, 20, 30) and tuple(f[8, 11]) == (0, 0, 0) and tuple(f[8, 12]) == (70, 80, 90)      # the lowest k on top
    assert not (f == colors[1]).all(axis=-1).any() and tuple(f[8, 14]) == (99, 99, 99)
    f = R.draw_markers(base.copy(), np.array([(1.25, 0.0)], np.float32), colors[:1], 3)                             # centre at column 18: clipped
    assert tuple(f[8, 16]) == (10, 20, 30) and tuple(f[8, 15]) == (0, 0, 0) and tuple(f[8, 14]) == (99, 99, 99) and f.shape == base.shape
    f = R.draw_markers(base.copy(), np.array([(0.0, 0.0)], np.float32), colors[:1], 1)                              # r = 1: one pixel in colour
    assert tuple(f[8, 8]) == (10, 20, 30) and tuple(f[8, 9]) == (0, 0, 0) and tuple(f[9, 9]) == (99, 99, 99)
    beyond = np.nextafter(np.float32(4), np.float32(5))
    for gone in ((np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0), (beyond, 0.0), (0.0, -beyond)):
        assert np.array_equal(R.draw_markers(base.copy(), np.array([gone], np.float32), colors[:1], 16), base)
    small = np.full((5, 5, 3), 99, np.uint8)                                                                        # |x| = 4 itself still draws
    assert (R.draw_markers(small.copy(), np.array([(4.0, 0.0)], np.float32), colors[:1], 16) != 99).any()
    assert np.array_equal(R.draw_markers(base.copy(), np.array([(0.0, 0.0)], np.float32), colors[:1], 0), base)     # r = 0 draws nothing
    canvas = np.full((1, 2, 2 * 4, 3 * 4, 3), 0xA5, np.uint8)
    R.cell_frames(canvas, np.zeros((1, 4, 4, 1), np.float32), np.ones((1, 1, 4, 4, 1), np.float32), 1, 2, 'unit')
    assert (canvas[0, 0, 4:, 8:] == 127).all() and (canvas[0, 1, 4:, 8:] == 255).all()
    assert (canvas[:, :, :4] == 0xA5).all() and (canvas[:, :, :, :8] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ animate.py's parser
def test_animate_refuses_bad_arguments_before_the_device_is_touched(tmp_path, capsys):
    import torch
    from PIL import Image
    import animate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    still = tmp_path / 'still.png'
    Image.fromarray(_picture(60, 40, 2)).save(str(still))
    empty = tmp_path / 'empty'
    empty.mkdir()
    short = tmp_path / 'short'
    short.mkdir()
    for i in range(32):
        Image.fromarray(_picture(16, 16, i)).save(str(short / ('%03d.png' % i)))
    cfg = os.path.join(REPO, 'configs', 'penn.yaml')                   # n_action = 9
    head = ['--config', cfg, '--checkpoint_stage1', str(ck), '--save_dir', str(tmp_path / 'out')]
    two = head + ['--checkpoint_stage2', str(ck), '--images', str(still)]
    cases = [(head + ['--images', str(still)], '--checkpoint_stage2'),                                  # neither stage 2 nor a driver
             (two + ['--samples', '4', '--actions', '0,1,2,3,4,5,6,7'], '2^24'),                        # 32 cells of 128 x 128
             (two + ['--samples', '65', '--actions', '0'], '--samples'),
             (two + ['--samples', '0'], '--samples'),
             (two + ['--actions', '9'], '--actions'), (two + ['--actions', '0,-1'], '--actions'), (two + ['--actions', '1,1'], '--actions'),
             (two + ['--actions', ''], '--actions'),
             (two + ['--box', '0,0,61,40'], '--box'), (two + ['--box', '0,0,1,40'], '--box'), (two + ['--box', '0,0,60'], '--box'),
             (two + ['--box', 'a,b,c,d'], '--box'), (two + ['--box', '30,0,10,40'], '--box'),
             (head + ['--checkpoint_stage2', str(ck), '--images', str(empty)], '--images'),
             (head + ['--checkpoint_stage2', str(ck), '--images', str(tmp_path / 'nothing.jpg')], '--images'),
             (two + ['--driver', str(short)], '--driver'), (two + ['--driver', str(tmp_path / 'nodir')], '--driver'),
             (two + ['--driver-mode', 'absolute'], '--driver-mode'), (two + ['--driver-scaled'], '--driver-scaled'),
             (two + ['--driver-box', '0,0,8,8'], '--driver-box'),
             (two + ['--driver', str(short), '--driver-mode', 'hold'], '--driver-mode'),
             (two + ['--driver', str(short), '--driver-mode', 'absolute', '--driver-scaled'], '--driver-scaled'),
             (two + ['--gif-fps', '0'], '--gif-fps'), (two + ['--gif-fps', '51'], '--gif-fps'),
             (two + ['--gif-dither', '-1'], '--gif-dither'), (two + ['--gif-dither', '65'], '--gif-dither'),
             (two + ['--overlay', '17'], '--overlay'), (two + ['--overlay', '-1'], '--overlay'),
             (two + ['--batch', '0'], '--batch'), (two + ['--sheet-frames', '32'], '--sheet-frames')]
    for argv, text in cases:
        with pytest.raises(SystemExit) as e:
            animate.main(argv)
        assert e.value.code == 2, argv
        assert text in capsys.readouterr().err, argv
    assert not (tmp_path / 'out').exists() and not torch.cuda.is_initialized()


# ------------------------------------------------------------------------------------------------ the ABI
def test_cell_frames_entry_refuses_bad_arguments_without_a_gpu():
    import kpx_amd  # noqa: F401
    from kpx_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'kpx_cell_frames_u8_f32') and 'kpx_cell_frames_u8_f32' in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 21 and _lib.lib.kpx_abi_version() == _lib.ABI_VERSION
    a = 1 << 20                                                        # an aligned fake address: never touched

    def cells(first=a, seq=a, b=2, t=3, h=8, w=8, c=3, pf=a, ps=a, k=5, colors=a + 1, r=2, canvas=a + 1, rows=2, cols=3, row=1, col=2, premap=0):
        return _lib.lib.kpx_cell_frames_u8_f32(first, seq, b, t, h, w, c, pf, ps, k, colors, r, canvas, rows, cols, row, col, premap, None)

    bad = [dict(first=None), dict(seq=None), dict(canvas=None), dict(first=a + 2), dict(seq=a + 1),
           dict(pf=None), dict(ps=None), dict(colors=None), dict(pf=a + 2), dict(ps=a + 3),
           dict(c=2), dict(c=0), dict(c=4), dict(b=0), dict(t=0), dict(h=0), dict(h=1025), dict(w=0), dict(w=1025),
           dict(rows=0), dict(rows=65), dict(cols=0), dict(cols=65), dict(row=2), dict(row=-1), dict(col=3), dict(col=-1),
           dict(k=0), dict(k=65), dict(k=-1), dict(r=17), dict(r=-1), dict(premap=2), dict(premap=-1),
           dict(r=0, first=None), dict(r=0, w=1025), dict(b=1 << 30, t=1)]
    for kw in bad:
        assert cells(**kw) == -1, kw
