"""numpy restatement of the contact sheets (evaluate.py --actions): the two quantisers of evaluate._save_img and the
paste of frames into a sheet of cells.  numpy only: the CPU tests hold the quantisers to the bytes PIL writes, the GPU tests hold
kpx_sheet_paste_u8_f32 to ``paste`` bit for bit."""
import numpy as np

from metrics_ref import png8 as unit8      # _save_img(rescale=True): uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))), clamped, NaN -> 0


def raw8(x):
    """The bytes evaluate._save_img(rescale=False) writes for x in [0, 1]: uint8(trunc(fl(x * 255))), clamped to [0, 255], NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        v = x * np.float32(255)
    v = np.nan_to_num(np.clip(v, 0, 255), nan=0.0)
    return np.trunc(v).astype(np.uint8)


QUANTISERS = {'unit': unit8, 'raw': raw8}


def paste(canvas, src, frames, row, col, premap):
    """canvas uint8 [B, rows*H, cols*W, 3] (changed in place and returned), src float32 [B,F,H,W,C], C in (1, 3):
    canvas[b, row*H:(row+1)*H, (col+j)*W:(col+j+1)*W, :] = q(src[b, frames[j]]), one channel broadcast to the three."""
    b, f, h, w, c = src.shape
    assert canvas.dtype == np.uint8 and canvas.shape[0] == b and canvas.shape[3] == 3 and c in (1, 3)
    assert canvas.shape[1] % h == 0 and canvas.shape[2] % w == 0 and (col + len(frames)) * w <= canvas.shape[2] and (row + 1) * h <= canvas.shape[1]
    q = QUANTISERS[premap]
    for j, fr in enumerate(frames):
        assert 0 <= fr < f
        canvas[:, row * h:(row + 1) * h, (col + j) * w:(col + j + 1) * w, :] = q(src[:, fr])        # (C = 1 broadcasts)
    return canvas
