"""The yardstick of the brightness-corrected PSNR / SSIM (tests/test_correct_cpu.py, tests/test_gpu_correct.py), numpy only and written
without a look at fdn_hip/correct.py:

  the float64 truth       exact integer statistics of the whole image, the coefficient formulas of include/fdn_correct.h, the corrected
                          image z (double operations rounded once each, then one rounding to float32) and its PSNR;
  reference_mean_var_f32  the reference's scripts/metrics/calculate_psnr_ssim.py:31-54 under --correct_mean_var restated call by call in
                          float32, "corrected twice", so that the single affine map of the truth can be held to the procedure it stands for.

Images are uint8 [h][w][3] arrays."""
import math

import numpy as np

NAN, INF = float("nan"), float("inf")


def sums(img):
    """(S, Q): per channel the sum and the sum of squares of a uint8 [h][w][3] image, Python integers"""
    x = img.reshape(-1, 3).astype(np.int64)
    return [int(v) for v in x.sum(axis=0)], [int(v) for v in (x * x).sum(axis=0)]


def moments(gt, rs, crop=0):
    """the 13 integers per image of include/fdn_correct.h: S_g, Q_g, S_r, Q_r per channel, and the maximum of the cropped ground truth"""
    h, w, _ = gt.shape
    (sg, qg), (sr, qr) = sums(gt), sums(rs)
    return sg + qg + sr + qr + [int(gt[crop:h - crop, crop:w - crop].max())]


def coefficients(gt, rs, mode, bgr=True):
    """[3][5] Python floats: m_r, s, m_g, lo, hi per channel"""
    n = gt.shape[0] * gt.shape[1]
    (sg, qg), (sr, qr) = sums(gt), sums(rs)
    if mode == "mean_var":
        out = []
        for c in range(3):
            var_g, var_r = n * qg[c] - sg[c] ** 2, n * qr[c] - sr[c] ** 2              # times N^2, exact integers
            s = NAN if var_r == 0 else math.sqrt(float(var_g) / float(var_r))
            out.append([sr[c] / n, s, sg[c] / n, -INF, INF])
        return out
    assert mode == "gt_mean", mode
    r, b = (2, 0) if bgr else (0, 2)
    gray_g = 299 * sg[r] + 587 * sg[1] + 114 * sg[b]
    gray_r = 299 * sr[r] + 587 * sr[1] + 114 * sr[b]
    s = NAN if gray_r == 0 else float(gray_g) / float(gray_r)
    return [[0.0, s, 0.0, 0.0, 255.0]] * 3


def corrected(gt, rs, mode, bgr=True):
    """z: float32 [h][w][3], the corrected restored image in code units 0 .. 255; each numpy operation below is one correctly rounded
    double operation per element"""
    z = np.empty(rs.shape, np.float32)
    with np.errstate(invalid="ignore"):
        for c, (m_r, s, m_g, lo, hi) in enumerate(coefficients(gt, rs, mode, bgr)):
            t = rs[:, :, c].astype(np.float64) - np.float64(m_r)
            t = t * np.float64(s)
            t = t + np.float64(m_g)
            t = np.minimum(np.maximum(t, lo), hi)                                       # both propagate NaN
            z[:, :, c] = t.astype(np.float32)
    return z


def psnr(gt, z, crop=0):
    """calculate_psnr (basicsr/metrics/psnr_ssim.py:47-62) of img1 = gt (uint8), img2 = z (float32): float64 mean over the cropped region"""
    h, w, _ = gt.shape
    a, b = gt[crop:h - crop, crop:w - crop].astype(np.float64), z[crop:h - crop, crop:w - crop].astype(np.float64)
    mse = float(np.mean((a - b) ** 2))
    if mse == 0:
        return INF
    return 20.0 * math.log10((1.0 if a.max() <= 1 else 255.0) / math.sqrt(mse))


def reference_mean_var_f32(gt, rs):
    """-> img_restored * 255 (float32 [h][w][3]) as the reference hands it to calculate_psnr under --correct_mean_var: :31, :36, :38-54, :61"""
    img_gt = gt.astype(np.float32) / 255.
    img_restored = rs.astype(np.float32) / 255.
    mean_l = []
    std_l = []
    for j in range(3):
        mean_l.append(np.mean(img_gt[:, :, j]))
        std_l.append(np.std(img_gt[:, :, j]))
    for j in range(3):
        for _ in range(2):                                                              # "correct twice"
            mean = np.mean(img_restored[:, :, j])
            img_restored[:, :, j] = img_restored[:, :, j] - mean + mean_l[j]
            std = np.std(img_restored[:, :, j])
            img_restored[:, :, j] = img_restored[:, :, j] / std * std_l[j]
    return img_restored * 255


def textured(h, w, seed, gain=0.5, offset=20.0, noise=4.0, n=None, texture=12.0):
    """a textured ground truth (waves, blocks and noise at moderate brightness) and a restored image of about gain * gt + offset + noise,
    per channel slightly different: uint8 [h][w][3], or [n][h][w][3]"""
    g = np.random.default_rng(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    base = 110 + 45 * np.sin(xx / 5.3) * np.cos(yy / 7.1) + 25 * (((xx // 9) + (yy // 6)) % 2)
    gt = np.clip(base[..., None] * np.array([0.9, 1.0, 1.1]) + g.normal(0, texture, shape), 0, 255).round().astype(np.uint8)
    rs = np.clip(gt * (gain * np.array([1.0, 1.1, 0.9])) + offset + g.normal(0, noise, shape), 0, 255).round().astype(np.uint8)
    return gt, rs


def ssim_3d_f64(gt, z, crop=0):
    """the 3-D SSIM of calculate_ssim (basicsr/metrics/psnr_ssim.py:149-200) with every map in float64: what the reference's float32 maps
    approximate.  Where the two differ, the float32 reference is limited by its own rounding (E[x^2] - mu^2 on smooth bright images)."""
    h, w, _ = gt.shape
    a, b = gt[crop:h - crop, crop:w - crop].astype(np.float64), z[crop:h - crop, crop:w - crop].astype(np.float64)
    i = np.arange(11) - 5.0
    k = np.exp(-i * i / (2 * 1.5 * 1.5))
    k /= k.sum()

    def window(t):
        for ax in range(3):
            pad = [(0, 0)] * 3
            pad[ax] = (5, 5)
            t = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), ax, np.pad(t, pad, mode="edge"))
        return t
    L = 1 if a.max() <= 1 else 255
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mu1, mu2 = window(a), window(b)
    s1, s2, s12 = window(a * a) - mu1 * mu1, window(b * b) - mu2 * mu2, window(a * b) - mu1 * mu2
    return float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean())


# The inputs of tests/test_gpu_correct.py: (h, w, crop_border) -> (gain, offset) of the restored image.  Smaller than the window and a
# tile; one past the tile edges; a crop that moves the border; several tiles.  Strong texture (noise of 40 codes): on smoother images the
# reference's float32 SSIM map is itself rounding-limited beyond the bound it is compared at (tests/test_correct_cpu.py holds the
# inputs to that).
GPU_SHAPES = [(6, 7, 0), (33, 65, 0), (70, 90, 7), (96, 160, 0)]
GPU_GAINS = {(6, 7, 0): (0.6, 20.0), (33, 65, 0): (1.7, -45.0), (70, 90, 7): (0.7, 15.0), (96, 160, 0): (1.3, -20.0)}
GPU_BATCH = ((0.5, 30.0), (1.0, -10.0), (1.6, -40.0))         # three 33 x 65 pairs that differ in brightness per image (and per channel)


def gpu_case(shape):
    h, w, _ = shape
    gain, offset = GPU_GAINS[shape]
    return textured(h, w, seed=h * 1000 + w, gain=gain, offset=offset, texture=40.0)


def gpu_batch():
    pairs = [textured(33, 65, seed=40 + i, gain=g, offset=o, texture=40.0) for i, (g, o) in enumerate(GPU_BATCH)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
