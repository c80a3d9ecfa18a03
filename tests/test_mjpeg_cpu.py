"""CPU: evaluate.py --video -- the restatement's streams decode in PIL and match PIL's own encoder in quality, the frame headers, the AVI
container field by field, the command-line unpacker, the argument rules of both tools and the entry's KPX_EINVAL table."""
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import mjpeg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FIXTURES = R.fixtures()
CASES = [(name, q) for name, (_, qs) in FIXTURES.items() for q in qs]
STRUCTURAL = ('flat', 'two_tone', 'cells', 'checker', 'grey_checker')


def _mjpeg():
    from kpx_amd import mjpeg
    return mjpeg


def _jpeg(img, q):
    m = _mjpeg()
    return m.frame_bytes(m.frame_prefix(img.shape[0], img.shape[1], m.quant_tables(q)), R.encode(img, q))


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()                                                          # the whole scan: a bad restart marker or code fails here
    return im


def _pil(img, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=q, subsampling=2, optimize=False)
    return buf.getvalue()


def _psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


def test_tables_are_the_restatements_and_pils():
    m = _mjpeg()
    for mine, ref in zip(m.HUFFMAN, (R.DC_LUMA, R.AC_LUMA, R.DC_CHROMA, R.AC_CHROMA)):
        assert mine[1] == tuple(ref[0]) and mine[2] == tuple(ref[1])
    assert m.ZIGZAG == tuple(R.ZIGZAG) and sorted(m.ZIGZAG) == list(range(64)) and m.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2)
    t = [[np.rint(8192 * (np.sqrt(1 / 8) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)) for x in range(8)] for u in range(8)]
    assert np.array_equal(np.array(t), R.DCT)
    for q in (1, 10, 25, 49, 50, 75, 90, 100):
        assert np.array_equal(m.quant_tables(q), R.quant_tables(q)) and m.quant_tables(q).dtype == np.uint8
        theirs = _decode(_pil(FIXTURES['noise'][0], q)).quantization
        assert [list(theirs[i]) for i in (0, 1)] == m.quant_tables(q).tolist(), q
    for bad in (0, 101, 7.5, True, None):
        with pytest.raises(ValueError):
            m.quant_tables(bad)


def test_fixtures_reach_their_branches():
    want = {('flat', 75): {}, ('two_tone', 100): {'dc_cat': 11}, ('cells', 100): {'dc_cat': 11}, ('checker', 100): {'ac_cat': 10},
            ('grey_checker', 50): {'zrl': 72}}
    for (name, q), need in want.items():
        stats = {}
        scan = R.encode(FIXTURES[name][0], q, stats)
        for key, value in need.items():
            assert stats.get(key) == value, (name, stats)
        if name == 'flat':
            assert set(stats) <= {'dc_cat', 'stuffed'} and b'\xff' not in scan.replace(b'\xff\x00', b'')       # EOB only, no RST
        if name == 'cells':                                            # nine MCU rows: RST0..RST7 in order, m wraps after 7 (only 8 markers)
            marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xff and scan[i + 1] != 0]
            assert marks == [0xd0 + (r & 7) for r in range(8)]
        if name == 'checker':
            assert stats['no_eob'] == 24 and stats['stuffed'] >= 100
    marks = R.encode(FIXTURES['smooth'][0], 90)
    marks = [marks[i + 1] for i in range(len(marks) - 1) if marks[i] == 0xff and marks[i + 1] != 0]
    assert marks == [0xd0 + (r & 7) for r in range(9)] and marks[8] == 0xd0                       # ten MCU rows: the ninth marker is RST0 again


@pytest.mark.parametrize('name,q', CASES)
def test_pil_decodes_every_stream(name, q):
    m = _mjpeg()
    img = FIXTURES[name][0]
    im = _decode(_jpeg(img, q))
    assert im.size == (img.shape[1], img.shape[0]) and im.mode == 'RGB'
    assert [list(im.quantization[i]) for i in (0, 1)] == m.quant_tables(q).tolist()


def test_quality_is_pils_on_photographic_content(capsys):
    """the decoded PSNR of the restatement's stream is at least PIL's own minus 0.05 dB (measured: see the printed gaps; the largest
    shortfall is recorded in DESIGN.md section 2)"""
    worst = -1e9
    for name in ('noise', 'smooth', 'smooth_wide'):
        img = FIXTURES[name][0]
        for q in (25, 75, 90, 100):
            mine, theirs = _psnr(_decode(_jpeg(img, q)).convert('RGB'), img), _psnr(_decode(_pil(img, q)).convert('RGB'), img)
            print('%-12s q%-3d ours %.4f dB  PIL %.4f dB  shortfall %+.4f dB' % (name, q, mine, theirs, theirs - mine))
            worst = max(worst, theirs - mine)
            assert mine >= theirs - 0.05, (name, q, mine, theirs)
    print('largest shortfall %.4f dB' % worst)


def test_structural_fixtures_decode_like_pils(capsys):
    """flat and two-level images: both encoders' decodes are compared sample by sample.  Measured: 0 on all five (both pipelines quantise
    these few large coefficients to the same integers, so the one decoder sees the same data).  Asserted: at most 1 of 255, the decoder's
    own rounding unit -- a wrong table, sign or zig-zag position moves these images by tens of levels."""
    worst = 0
    for name in STRUCTURAL:
        img, qs = FIXTURES[name]
        for q in qs:
            mine, theirs = np.asarray(_decode(_jpeg(img, q)).convert('RGB'), np.int64), np.asarray(_decode(_pil(img, q)).convert('RGB'), np.int64)
            diff = int(np.abs(mine - theirs).max())
            print('%-12s q%-3d largest |ours - PIL| = %d' % (name, q, diff))
            worst = max(worst, diff)
    print('largest difference %d' % worst)
    assert worst <= 1


def test_frame_prefix_segments():
    m = _mjpeg()
    qt = m.quant_tables(75)
    p = m.frame_prefix(48, 160, qt)
    assert p[:2] == b'\xff\xd8' and p == m.frame_prefix(48, 160, qt.astype(np.int64))
    segs, pos = [], 2
    while pos < len(p):
        assert p[pos] == 0xff
        size = struct.unpack_from('>H', p, pos + 2)[0]
        segs.append((p[pos + 1], p[pos + 4:pos + 2 + size]))
        pos += 2 + size
    assert pos == len(p) and [s[0] for s in segs] == [0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
    assert segs[0][1] == b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'
    assert segs[1][1] == bytes([0]) + bytes(int(qt[0][z]) for z in m.ZIGZAG) and segs[2][1][0] == 1
    assert segs[3][1] == struct.pack('>BHHB', 8, 48, 160, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [s[1][0] for s in segs[4:8]] == [0x00, 0x10, 0x01, 0x11] and [len(s[1]) for s in segs[4:8]] == [29, 179, 29, 179]
    assert segs[8][1] == struct.pack('>H', 10) and segs[9][1] == bytes([3, 1, 0, 2, 0x11, 3, 0x11, 0, 63, 0])
    for h, w in ((24, 32), (32, 8), (4112, 16), (0, 16)):
        with pytest.raises(ValueError):
            m.frame_prefix(h, w, qt)
    bad = qt.copy()
    bad[1, 5] = 0
    with pytest.raises(ValueError):
        m.frame_prefix(16, 16, bad)


def test_avi_layout_field_by_field(tmp_path):
    m = _mjpeg()
    frames = [b'\xff\xd8' + bytes(range(7)), b'\xff\xd8' + bytes(range(10)), b'\xff\xd8\x01']       # 9 (odd), 12, 3 (odd) bytes
    path = str(tmp_path / 'a.avi')
    size = m.write_avi(path, frames, 24, 48, 160)
    data = open(path, 'rb').read()
    assert size == len(data) and m.read_avi(path) == (24, 48, 160, frames)
    u32 = lambda at: struct.unpack_from('<I', data, at)[0]
    assert data[:4] == b'RIFF' and u32(4) == len(data) - 8 and data[8:12] == b'AVI '
    assert data[12:16] == b'LIST' and u32(16) == 4 + 64 + 8 + 4 + 64 + 48 and data[20:24] == b'hdrl'
    assert data[24:28] == b'avih' and u32(28) == 56
    assert struct.unpack_from('<14I', data, 32) == (1000000 // 24, 12 * 24, 0, 0x10, 3, 0, 1, 12, 160, 48, 0, 0, 0, 0)
    assert data[88:92] == b'LIST' and u32(92) == 4 + 64 + 48 and data[96:100] == b'strl'
    assert data[100:104] == b'strh' and u32(104) == 56
    assert struct.unpack_from('<4s4sIHHIIIIIIiI4h', data, 108) == (b'vids', b'MJPG', 0, 0, 0, 0, 1, 24, 0, 3, 12, -1, 0, 0, 0, 160, 48)
    assert data[164:168] == b'strf' and u32(168) == 40
    assert struct.unpack_from('<IiiHH4sIiiII', data, 172) == (40, 160, 48, 1, 24, b'MJPG', 160 * 48 * 3, 0, 0, 0, 0)
    movi = 212
    assert data[movi:movi + 4] == b'LIST' and data[movi + 8:movi + 12] == b'movi'
    assert u32(movi + 4) == 4 + (8 + 9 + 1) + (8 + 12) + (8 + 3 + 1)
    at, offsets = movi + 12, []
    for f in frames:
        assert data[at:at + 4] == b'00dc' and u32(at + 4) == len(f) and data[at + 8:at + 8 + len(f)] == f
        offsets.append(at - (movi + 8))                                # from the 'movi' fourcc
        at += 8 + len(f)
        if len(f) & 1:
            assert data[at] == 0                                       # the pad byte is outside the chunk's size
            at += 1
    assert offsets == [4, 22, 42]
    assert data[at:at + 4] == b'idx1' and u32(at + 4) == 48 and at + 8 + 48 == len(data)
    for i, f in enumerate(frames):
        assert struct.unpack_from('<4sIII', data, at + 8 + 16 * i) == (b'00dc', 0x10, offsets[i], len(f))
    for fps in (0, 241, 2.5):
        with pytest.raises(ValueError):
            m.write_avi(path, frames, fps, 48, 160)
    with pytest.raises(ValueError):
        m.write_avi(path, [], 10, 48, 160)
    open(str(tmp_path / 'cut.avi'), 'wb').write(data[:-5])
    with pytest.raises(ValueError):
        m.read_avi(str(tmp_path / 'cut.avi'))


def test_avi_of_two_gigabytes_is_refused(tmp_path, monkeypatch):
    m = _mjpeg()
    monkeypatch.setattr(m, 'MAX_FILE_BYTES', 400)
    with pytest.raises(ValueError, match='2\\^31'):
        m.write_avi(str(tmp_path / 'big.avi'), [bytes(200)], 10, 16, 16)
    assert not os.path.exists(str(tmp_path / 'big.avi'))
    assert _mjpeg().write_avi(str(tmp_path / 'ok.avi'), [bytes(100)], 10, 16, 16) == 12 + (8 + 192) + (8 + 4 + 108) + (8 + 16)


def test_real_frames_round_trip_and_the_command_line_unpacks_them(tmp_path):
    from PIL import Image
    m = _mjpeg()
    batch = R.mixed_batch()
    jpegs = [_jpeg(f, 90) for f in batch]
    path = str(tmp_path / 'b.avi')
    m.write_avi(path, jpegs, 30, 32, 48)
    assert m.read_avi(path) == (30, 32, 48, jpegs)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([sys.executable, '-m', 'kpx_amd.mjpeg', path, '--png', str(tmp_path / 'png')], env=env, cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert '5 frames of 48 x 32 at 30 fps' in out.stdout
    assert sorted(os.listdir(str(tmp_path / 'png'))) == ['%05d.png' % i for i in range(5)]
    for i, j in enumerate(jpegs):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'png' / ('%05d.png' % i)))), np.asarray(_decode(j).convert('RGB')))


def test_evaluate_argument_rules(tmp_path, capsys):
    import evaluate
    base = ['--config', str(tmp_path / 'none.yaml'), '--checkpoint_stage1', 'a', '--checkpoint_stage2', 'b']
    for extra, word in ((['--video', '--no-save'], '--no-save'), (['--video-fps', '5'], 'need it'), (['--video-quality', '50'], 'need it'),
                        (['--video', '--video-fps', '0'], '1..240'), (['--video', '--video-fps', '241'], '1..240'),
                        (['--video', '--video-quality', '0'], '1..100'), (['--video', '--video-quality', '101'], '1..100'),
                        (['--frames', '64'], '--frames and --rate write long.gif beside the files of --gif and need it'),
                        (['--rate', '2'], '--frames and --rate write long.gif beside the files of --gif and need it'),
                        (['--video', '--rate', '25'], 'plays at most 240'),
                        (['--video', '--gif', '--rate', '6'], 'a GIF plays at most 50'),
                        (['--video', '--gif', '--frames', '2048', '--rate', '4'], '2^24')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    # accepted: the parser lets these through and the run stops at the configuration file that is not there
    for extra in (['--video', '--frames', '64'], ['--video', '--rate', '24'], ['--video', '--frames', '2048', '--rate', '4'],
                  ['--video', '--video-fps', '240', '--video-quality', '1'], ['--video', '--gif', '--rate', '5']):
        with pytest.raises(FileNotFoundError):
            evaluate.main(base + extra)
        assert 'error' not in capsys.readouterr().err, extra


def test_animate_argument_rules(tmp_path, capsys):
    import torch
    from PIL import Image
    import animate
    ck = tmp_path / 'ck.npz'
    ck.write_bytes(b'')
    still = tmp_path / 'still.png'
    Image.fromarray(FIXTURES['smooth'][0]).save(str(still))
    two = ['--config', os.path.join(REPO, 'configs', 'penn.yaml'), '--checkpoint_stage1', str(ck), '--save_dir', str(tmp_path / 'out'),
           '--checkpoint_stage2', str(ck), '--images', str(still)]
    for extra, word in ((['--video-fps', '5'], 'need it'), (['--video-quality', '50'], 'need it'), (['--video', '--video-fps', '0'], '1..240'),
                        (['--video', '--video-fps', '241'], '1..240'), (['--video', '--video-quality', '0'], '1..100'),
                        (['--video', '--video-quality', '101'], '1..100'),
                        (['--video', '--video-fps', '100', '--gif-fps', '1', '--rate', '3'], 'play at most 240')):
        with pytest.raises(SystemExit) as e:
            animate.main(two + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    assert not (tmp_path / 'out').exists() and not torch.cuda.is_initialized()


def test_entry_refuses_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                        # an aligned fake address
    qt = np.ascontiguousarray(_mjpeg().quant_tables(75))
    assert lib.kpx_jpeg_scan_bound(16, 16) == 6 * 416 and lib.kpx_jpeg_scan_bound(128, 384) == 8 * 24 * 6 * 416 + 2 * 7
    assert lib.kpx_jpeg_scan_bound(4096, 4096) == 256 * 256 * 6 * 416 + 2 * 255
    for h, w in ((8, 16), (16, 24), (4112, 16), (16, 4112), (0, 0), (-16, 16)):
        assert lib.kpx_jpeg_scan_bound(h, w) == 0 and lib.kpx_jpeg_workspace_bytes(1, h, w) == 0
    assert lib.kpx_jpeg_workspace_bytes(0, 16, 16) == 0 and lib.kpx_jpeg_workspace_bytes(-1, 16, 16) == 0
    assert lib.kpx_jpeg_workspace_bytes(128, 4096, 4096) == 0 and lib.kpx_jpeg_workspace_bytes(127, 4096, 4096) > 0      # N H W < 2^31
    ws = lib.kpx_jpeg_workspace_bytes(2, 32, 48)
    assert ws >= 2 * 6 * (768 + 6 * 416) and ws % 8 == 0

    def enc(rgb=a, n=2, h=32, w=48, q=qt.ctypes.data, scans=a, offsets=a, work=a, nbytes=ws):
        return lib.kpx_jpeg_encode_u8(rgb, n, h, w, q, scans, offsets, work, nbytes, None)
    assert enc(rgb=None) == -1 and enc(q=None) == -1 and enc(scans=None) == -1 and enc(offsets=None) == -1 and enc(work=None) == -1
    assert enc(offsets=a + 4) == -1 and enc(work=a + 4) == -1 and enc(nbytes=ws - 1) == -1 and enc(nbytes=0) == -1
    assert enc(n=0) == -1 and enc(h=24) == -1 and enc(w=40) == -1 and enc(h=0) == -1 and enc(h=4112) == -1 and enc(n=1 << 21) == -1
    zero = qt.copy()
    zero[1, 63] = 0
    assert enc(q=zero.ctypes.data) == -1
    zero = qt.copy()
    zero[0, 0] = 0
    assert enc(q=zero.ctypes.data) == -1
