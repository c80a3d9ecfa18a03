"""float64 restatement of the frame metrics ([TF-sem metrics]): TF 1.12 tf.image.ssim (11-tap Gaussian window,
sigma 1.5, VALID, k1 = 0.01, k2 = 0.03, compensation 1) and tf.image.psnr, per frame of NHWC arrays, plus the 8-bit quantisation of
evaluate._save_img(rescale=True).  numpy only: the CPU tests check it against closed forms, the GPU tests hold the kernel to it."""
import numpy as np

SIZE, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def window_1d():
    """w[i] = exp(-(i-5)^2 / (2 sigma^2)) / sum_j exp(-(j-5)^2 / (2 sigma^2))"""
    i = np.arange(SIZE, dtype=np.float64)
    g = np.exp(-(i - (SIZE - 1) / 2.0) ** 2 / (2.0 * SIGMA ** 2))
    return g / g.sum()


def window_2d_tf():
    """TF 1.12 _fspecial_gauss: softmax over -(x^2 + y^2) / (2 sigma^2) of the centred coordinates."""
    coords = np.arange(SIZE, dtype=np.float64) - (SIZE - 1) / 2.0
    g = -0.5 * coords ** 2 / SIGMA ** 2
    g = (g[None, :] + g[:, None]).reshape(-1)
    e = np.exp(g - g.max())
    return (e / e.sum()).reshape(SIZE, SIZE)


def _filter(x, w):
    """Depthwise VALID filtering of [N,H,W,C] with w (x) w, separably: rows, then columns."""
    ho, wo = x.shape[1] - SIZE + 1, x.shape[2] - SIZE + 1
    h = sum(w[i] * x[:, :, i:i + wo, :] for i in range(SIZE))
    return sum(w[i] * h[:, i:i + ho, :, :] for i in range(SIZE))


def frame_metrics(a, b, max_val=1.0):
    """-> float64 [N,3] = (ssim, mse, psnr) of a[n] against b[n], both [N,H,W,C]."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    L = float(max_val)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    w = window_1d()
    mu_a, mu_b = _filter(a, w), _filter(b, w)
    num0 = mu_a * mu_b * 2.0
    den0 = mu_a ** 2 + mu_b ** 2
    lum = (num0 + c1) / (den0 + c1)
    cs = (_filter(a * b, w) * 2.0 - num0 + c2) / (_filter(a * a + b * b, w) - den0 + c2)
    ssim = (lum * cs).mean(axis=(1, 2)).mean(axis=-1)
    mse = ((a - b) ** 2).mean(axis=(1, 2, 3))
    with np.errstate(divide='ignore'):
        psnr = 20.0 * np.log10(L) - 10.0 * np.log10(mse)
    return np.stack([ssim, mse, psnr], axis=1)


def png8(x):
    """The bytes evaluate._save_img(rescale=True) writes: uint8(trunc(fl(fl(0.5 * fl(x + 1)) * 255))), clamped to [0, 255], NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    v = (np.float32(0.5) * (x + np.float32(1.0))) * np.float32(255)
    v = np.nan_to_num(np.clip(v, 0, 255), nan=0.0)
    return np.trunc(v).astype(np.uint8)


def frame_metrics_png8(a, b):
    """The metrics of the 8-bit frames of a and b, scored as q / 255 with L = 1."""
    return frame_metrics(png8(a) / 255.0, png8(b) / 255.0, 1.0)
