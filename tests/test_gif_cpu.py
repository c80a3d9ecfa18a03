"""CPU: the host half of evaluate.py --gif -- the GIF89a container and the library's LZW encoder against the restatement and PIL, the median
cut, and the argument checks of the new entries (DESIGN.md sections 2 and 4.4)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gif_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'unsupervised-keypoint-learning-for-guiding-class-conditional-video-prediction_amd', 'csrc')


def _indices(t, h, w, p, seed=0):
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, p, size=(t, h, w)).astype(np.uint8)
    if (h, w) == (128, 384):                     # one smooth frame, one noise frame: the noise fills the 4096-entry table more than once
        idx[0] = (np.arange(h)[:, None] // 4 + np.arange(w)[None, :] // 8) % p
    return idx, rs.randint(0, 256, size=(p, 3)).astype(np.uint8)


@pytest.mark.parametrize('t,h,w,p', [(3, 5, 7, 2), (1, 1, 1, 1), (4, 33, 17, 5), (3, 9, 11, 17), (2, 16, 16, 256), (2, 128, 384, 256)])
def test_write_gif_is_the_restatement_and_pil_decodes_it(tmp_path, t, h, w, p):
    from kpx_amd import gif
    idx, pal = _indices(t, h, w, p)
    path = str(tmp_path / 'a.gif')
    gif.write_gif(path, idx, pal, 7)
    data = open(path, 'rb').read()
    assert data == R.gif_bytes(idx, pal, 7)
    if (h, w) == (128, 384):                     # the table did reset: more than 4096 - 258 codes in the noise frame
        assert len(R.lzw(idx[1].reshape(-1), 8)) * 8 // 12 > 2 * 3838
    frames, durations, loop = R.decode_gif(path)
    assert frames.shape == (t, h, w, 3) and np.array_equal(frames, pal[idx])
    assert durations == [70] * t and loop == 0


def _c_lzw(idx, code, short=0):
    from kpx_amd._lib import lib
    idx = np.ascontiguousarray(idx, np.uint8)
    bound = int(lib.kpx_gif_lzw_bound(idx.size))
    want = R.lzw(idx, code)
    assert len(want) <= bound
    out = np.zeros(len(want) - short + 8, np.uint8)
    n = lib.kpx_gif_lzw_u8(idx.ctypes.data, idx.size, code, out.ctypes.data, len(want) - short)
    return n, out, want


def test_lzw_entry_is_the_restatement():
    rs = np.random.RandomState(3)
    cases = [(np.zeros(1, np.uint8), 2), (np.full(70000, 3, np.uint8), 2), (rs.randint(0, 2, 5000), 2), (rs.randint(0, 256, 20000), 8),
             (np.full(70000, 200, np.uint8), 8)]
    for idx, code in cases:
        n, out, want = _c_lzw(idx, code)
        assert n == len(want) and out[:n].tobytes() == want and not out[n:].any(), (idx.size, code)
        n, out, _ = _c_lzw(idx, code, short=1)                       # a buffer one byte short: refused, and nothing written past it
        assert n == -1 and not out[len(want) - 1:].any()


def test_lzw_entry_refuses_bad_arguments():
    from kpx_amd._lib import lib
    buf = np.zeros(64, np.uint8)
    idx = np.array([0, 1, 5], np.uint8)
    assert lib.kpx_gif_lzw_u8(idx.ctypes.data, 3, 2, buf.ctypes.data, 64) == -1       # index 5 outside a 4-entry table
    assert lib.kpx_gif_lzw_u8(idx.ctypes.data, 3, 3, buf.ctypes.data, 64) > 0
    assert lib.kpx_gif_lzw_u8(idx.ctypes.data, 3, 1, buf.ctypes.data, 64) == -1 and lib.kpx_gif_lzw_u8(idx.ctypes.data, 3, 9, buf.ctypes.data, 64) == -1
    assert lib.kpx_gif_lzw_u8(None, 3, 3, buf.ctypes.data, 64) == -1 and lib.kpx_gif_lzw_u8(idx.ctypes.data, 3, 3, None, 64) == -1


def _hist(img):
    return R.hist_add(np.zeros((1, 32768, 4), np.uint32), np.ascontiguousarray(img).reshape(1, -1, 3))[0]


def test_median_cut_is_lossless_on_few_colours():
    from kpx_amd import gif
    rs = np.random.RandomState(5)
    cells = rs.choice(32768, size=200, replace=False)
    colours = np.stack([(cells >> 10) * 8, ((cells >> 5) & 31) * 8, (cells & 31) * 8], axis=1) + rs.randint(0, 8, size=(200, 3))
    img = colours[rs.randint(0, 200, size=(40, 40))].astype(np.uint8)
    img.reshape(-1, 3)[:200] = colours                                 # every colour occurs
    h = _hist(img)
    pal, boxes = gif.median_cut(h, return_boxes=True)
    assert pal.shape == (200, 3) and all(b.size == 1 for b in boxes)
    idx = R.palette_map(img[None], pal)[0]
    assert np.array_equal(pal[idx], img)
    assert np.array_equal(pal, gif.median_cut(h))                      # deterministic
    want, _ = R.median_cut(h)
    assert np.array_equal(pal, want)
    assert gif.median_cut(h, P=7).shape == (7, 3)


def _ramp(noise):
    x, y = np.arange(64)[None, :], np.arange(64)[:, None]
    img = np.stack([4 * x + 0 * y, 4 * y + 0 * x, 2 * x + 2 * y], axis=2).astype(np.int64)
    if noise:
        img = np.clip(img + np.random.RandomState(0).randint(-6, 7, size=img.shape), 0, 255)
    return img.astype(np.uint8)


@pytest.mark.parametrize('noise', [False, True])
def test_median_cut_on_a_ramp(noise):
    from kpx_amd import gif
    img = _ramp(noise)
    h = _hist(img)
    pal, boxes = gif.median_cut(h, return_boxes=True)
    want, want_boxes = R.median_cut(h)
    assert np.array_equal(pal, want) and [sorted(b.tolist()) for b in boxes] == [sorted(b) for b in want_boxes]
    # every occupied cell in exactly one box; the counts conserved
    members = np.concatenate(boxes)
    assert np.array_equal(np.sort(members), np.nonzero(h[:, 0])[0])
    assert sum(int(h[b, 0].sum()) for b in boxes) == 64 * 64
    assert pal.shape == (256, 3)
    mse = lambda p: float(((p[R.palette_map(img[None], p)[0]].astype(np.int64) - img) ** 2).mean())
    levels = lambda n: [(2 * i + 1) * 255 // (2 * n) for i in range(n)]
    p332 = np.array([[r, g, b] for r in levels(8) for g in levels(8) for b in levels(4)], np.uint8)
    got, fixed = mse(pal), mse(p332)
    print('ramp noise=%s: median cut MSE %.2f, 3-3-2 MSE %.2f' % (noise, got, fixed))
    assert got < fixed


def test_median_cut_edge_cases():
    from kpx_amd import gif
    assert np.array_equal(gif.median_cut(np.zeros((32768, 4), np.uint32)), np.zeros((1, 3), np.uint8))
    h = _hist(np.full((3, 3, 3), 255, np.uint8))
    assert np.array_equal(gif.median_cut(h), [[255, 255, 255]])
    with pytest.raises(ValueError):
        gif.median_cut(np.zeros((100, 4), np.uint32))
    with pytest.raises(ValueError):
        gif.median_cut(h, P=257)


def test_device_entries_refuse_bad_arguments_without_a_gpu():
    from kpx_amd._lib import lib
    a = 1 << 20                                                       # an aligned fake address
    hist = lambda rgb=a, g=1, n=16, h=a: lib.kpx_color_hist_add_u32(rgb, g, n, h, None)
    assert hist(rgb=None) == -1 and hist(h=None) == -1 and hist(h=a + 2) == -1
    assert hist(n=0) == -1 and hist(n=(1 << 24) + 1) == -1 and hist(g=0) == -1 and hist(g=65536) == -1

    def pmap(rgb=a, g=1, t=2, h=4, w=5, pal=a, sizes=a, pmax=256, dither=0, idx=a):
        return lib.kpx_palette_map_u8(rgb, g, t, h, w, pal, sizes, pmax, dither, idx, None)
    assert pmap(rgb=None) == -1 and pmap(pal=None) == -1 and pmap(sizes=None) == -1 and pmap(idx=None) == -1 and pmap(sizes=a + 1) == -1
    assert pmap(pmax=0) == -1 and pmap(pmax=257) == -1 and pmap(dither=-1) == -1 and pmap(dither=65) == -1
    assert pmap(g=0) == -1 and pmap(t=0) == -1 and pmap(h=0) == -1 and pmap(w=0) == -1 and pmap(t=1 << 16, h=1 << 16, w=2) == -1
    assert lib.kpx_gif_lzw_bound(0) >= 2 and lib.kpx_gif_lzw_bound(1000) >= 1503


def test_evaluate_refuses_gif_with_no_save_and_bad_ranges(tmp_path, capsys):
    import evaluate
    base = ['--config', str(tmp_path / 'none.yaml'), '--checkpoint_stage1', 'a', '--checkpoint_stage2', 'b']
    for extra, word in ((['--gif', '--no-save'], '--no-save'), (['--gif-fps', '5'], 'need it'), (['--gif', '--gif-fps', '0'], '1..50'),
                        (['--gif', '--gif-fps', '51'], '1..50'), (['--gif', '--gif-dither', '65'], '0..64'),
                        (['--gif', '--gif-dither', '-1'], '0..64')):
        with pytest.raises(SystemExit) as e:
            evaluate.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra


LZW_MAIN = r'''
#include "gif_lzw.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
static int run(const std::vector<uint8_t>& idx, int code, const char* what) {
    std::vector<uint8_t> out(kpx_lzw_bound(idx.size()));
    const long long n = kpx_lzw_encode(idx.data(), idx.size(), code, out.data(), out.size());
    if (n < 1 || (size_t)n > out.size()) { printf("FAIL %s: %lld\n", what, n); return 1; }
    std::vector<uint8_t> tight((size_t)n - 1);
    if (kpx_lzw_encode(idx.data(), idx.size(), code, tight.data(), tight.size()) != -1) { printf("FAIL %s: short buffer\n", what); return 1; }
    unsigned long long sum = 0;
    for (long long i = 0; i < n; ++i) sum = sum * 131 + out[(size_t)i];
    printf("%s %lld %llu\n", what, n, sum);
    return 0;
}
int main() {
    int bad = 0;
    bad += run(std::vector<uint8_t>(), 2, "empty");
    bad += run(std::vector<uint8_t>(1, 0), 2, "one");
    bad += run(std::vector<uint8_t>(70000, 3), 2, "run");
    std::vector<uint8_t> a(5000), b(20000);
    unsigned s = 12345;
    for (auto& v : a) { s = s * 1664525u + 1013904223u; v = (uint8_t)((s >> 16) & 1); }
    for (auto& v : b) { s = s * 1664525u + 1013904223u; v = (uint8_t)(s >> 24); }
    bad += run(a, 2, "random2");
    bad += run(b, 8, "random256");
    std::vector<uint8_t> c(3, 9);
    uint8_t o[64];
    if (kpx_lzw_encode(c.data(), 3, 3, o, 64) != -1) { printf("FAIL range\n"); ++bad; }
    return bad;
}
'''


def _lcg_bytes(n, state, shift, mask):
    out = np.empty(n, np.uint8)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xffffffff
        out[i] = (state >> shift) & mask
    return out, state


def test_lzw_header_stands_alone_under_the_sanitizers(tmp_path):
    """The LZW header alone (no HIP, nothing of the library) in a program of its own, built by the host compiler with the address and
    undefined-behaviour sanitizers and run as a child process; its streams are the restatement's."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    src, exe = tmp_path / 'lzw_main.cpp', tmp_path / 'lzw_main'
    src.write_text(LZW_MAIN)
    base = [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC, str(src), '-o', str(exe)]
    # the runtimes linked statically where the compiler can (gcc's default is shared): the program then needs nothing from its environment
    build = subprocess.run(base + ['-static-libasan', '-static-libubsan'], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(base, capture_output=True, text=True)
    if build.returncode != 0 and ('asan' in build.stderr or 'ubsan' in build.stderr or 'sanitizer' in build.stderr.lower()):
        pytest.skip('the host compiler cannot link the sanitizer runtimes')
    assert build.returncode == 0, build.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    a, s = _lcg_bytes(5000, 12345, 16, 1)
    b, _ = _lcg_bytes(20000, s, 24, 255)
    want = {'empty': ([], 2), 'one': ([0], 2), 'run': ([3] * 70000, 2), 'random2': (a, 2), 'random256': (b, 8)}
    lines = dict((ln.split()[0], ln.split()[1:]) for ln in res.stdout.strip().splitlines())
    assert set(lines) == set(want)
    for name, (idx, code) in want.items():
        stream = R.lzw(idx, code)
        total = 0
        for v in stream:
            total = (total * 131 + v) & 0xffffffffffffffff
        assert lines[name] == [str(len(stream)), str(total)], name


def test_restatement_maps_whole_rollouts_as_it_maps_frames():
    """gif_ref.palette_map takes an exact float32 matrix form above 65536 pixels: the same indices as the rule frame by frame, ties and
    dither included"""
    rs = np.random.RandomState(9)
    pal = rs.randint(0, 256, size=(256, 3)).astype(np.uint8)
    pal[100], pal[7] = pal[3], (0, 0, 0)
    pal[200] = (255, 255, 255)
    rgb = rs.randint(0, 256, size=(3, 150, 150, 3)).astype(np.uint8)
    rgb[0, :40] = pal[3]
    rgb[1, :40] = (rs.randint(0, 2, size=(40, 150, 1)) * 255).astype(np.uint8)
    for amp in (0, 64):
        whole = R.palette_map(rgb, pal, amp)
        frames = np.stack([R.palette_map(rgb[t:t + 1], pal, amp)[0] for t in range(3)])
        assert np.array_equal(whole, frames), amp
    assert (R.palette_map(rgb, pal)[0, :40] == 3).all()
