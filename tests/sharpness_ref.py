"""The yardstick of the deblurring evaluation (tests/test_sharpness_cpu.py, tests/test_gpu_sharpness.py), numpy only and written from
the definitions in the head comment of include/fdn_sharpness.h without a look at csrc/sharpness.hip: integers where the definition has
integers, float64 elsewhere, and a `real` switch (np.longdouble) that shows how far float64 itself is from the formula.

Images are uint8 [h][w][3] arrays; a is the ground truth, b the restored image."""
import math

import numpy as np

K5 = np.array([1, 5, 8, 5, 1], dtype=np.int64)           # 20 times the reference's [.05 .25 .4 .25 .05]
EDGE_SCALE = 40800000                                     # 400 * 400 * 255: N / EDGE_SCALE is the reference's Laplacian difference
EDGE_EPS2 = 1e-6                                          # CharbonnierLoss: eps = 1e-3, squared
GMSD_T = 24480000000                                      # 170 * 144e6


def filter5(x):
    """sum over the 5 x 5 window of k_i k_j x(clamp(p + (i, j))) on the two leading axes of an int64 array: 400 G(x)"""
    h, w = x.shape[:2]
    p = np.pad(x, ((2, 2), (2, 2)) + ((0, 0),) * (x.ndim - 2), mode="edge")
    rows = sum(int(K5[i]) * p[i:i + h] for i in range(5))
    return sum(int(K5[j]) * rows[:, j:j + w] for j in range(5))


def edge_residual(a, b):
    """N of every element: int64 [h][w][3]"""
    d = a.astype(np.int64) - b.astype(np.int64)
    z = np.zeros_like(d)
    z[::2, ::2] = 4 * filter5(d)[::2, ::2]
    return 160000 * d - filter5(z)


def edge_terms(a, b, real=np.float64):
    """e of every element: [h][w][3] of `real`"""
    r = edge_residual(a, b).astype(real) / real(EDGE_SCALE)
    return np.sqrt(r * r + real(EDGE_EPS2))


def edge_sum(a, b, real=np.float64):
    """the sum of e over the image, as a Python float: exactly rounded (math.fsum) in float64"""
    e = edge_terms(a, b, real)
    return math.fsum(e.ravel().tolist()) if real is np.float64 else float(e.sum())


def edge_error(a, b, real=np.float64):
    return edge_sum(a, b, real) / a.size


def gray1000(img, bgr=True):
    """299 R + 587 G + 114 B: int64 [h][w]"""
    x = img.astype(np.int64)
    r, b = (2, 0) if bgr else (0, 2)
    return 299 * x[:, :, r] + 587 * x[:, :, 1] + 114 * x[:, :, b]


def gmsd_dims(h, w):
    return (h + 1) // 2, (w + 1) // 2


def block_sums(img, bgr=True):
    """s: int64 [hd][wd], the sum of the gray over the 2 x 2 block at (2i, 2j), samples outside the image counting 0"""
    y = gray1000(img, bgr)
    h, w = y.shape
    hd, wd = gmsd_dims(h, w)
    p = np.zeros((2 * hd, 2 * wd), np.int64)
    p[:h, :w] = y
    return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]


def grad2(img, bgr=True):
    """A = gx^2 + gy^2 of Prewitt on s with zero outside the grid: int64 [hd][wd]"""
    s = block_sums(img, bgr)
    hd, wd = s.shape
    p = np.pad(s, 1)
    gx = sum(p[1 + r:1 + r + hd, 2:2 + wd] - p[1 + r:1 + r + hd, 0:wd] for r in (-1, 0, 1))
    gy = sum(p[2:2 + hd, 1 + c:1 + c + wd] - p[0:hd, 1 + c:1 + c + wd] for c in (-1, 0, 1))
    return gx * gx + gy * gy


def gms_map(a, b, bgr=True, real=np.float64):
    """q of every grid point: [hd][wd] of `real`"""
    aa, ab = grad2(a, bgr), grad2(b, bgr)
    return (real(2) * np.sqrt(aa.astype(real) * ab.astype(real)) + real(GMSD_T)) / (aa + ab + GMSD_T).astype(real)


def std_from_sums(s1, s2, n):
    return math.sqrt(max(0.0, (s2 - s1 * s1 / n) / (n - 1)))


def gmsd_sums(a, b, bgr=True):
    """(sum of q, sum of q^2, n), the sums exactly rounded"""
    q = gms_map(a, b, bgr).ravel()
    return math.fsum(q.tolist()), math.fsum((q * q).tolist()), q.size


def gmsd(a, b, bgr=True):
    return std_from_sums(*gmsd_sums(a, b, bgr))


def gradient_terms(img, bgr=True, real=np.float64):
    """m of every grid point"""
    return np.sqrt(grad2(img, bgr).astype(real)) / real(12000)


def mean_gradient(img, bgr=True):
    m = gradient_terms(img, bgr).ravel()
    return math.fsum(m.tolist()) / m.size


def soft_pair(h, w, seed, n=None):
    """a textured image and a blurred, dimmed copy of it: uint8 [h][w][3] (or [n][h][w][3]) each"""
    g = np.random.default_rng(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    base = 120 + 50 * np.sin(xx / 2.3) * np.cos(yy / 3.1) + 40 * (((xx // 5) + (yy // 4)) % 2)
    src = np.clip(base[..., None] * np.array([0.9, 1.0, 1.1]) + g.normal(0, 25, shape), 0, 255)
    p = np.pad(src, [(0, 0)] * (src.ndim - 3) + [(1, 1), (1, 1), (0, 0)], mode="edge")
    blur = sum(p[..., i:i + h, j:j + w, :] for i in range(3) for j in range(3)) / 9.0
    return src.round().astype(np.uint8), np.clip(blur * 0.8 + 6, 0, 255).round().astype(np.uint8)


def random_pair(h, w, seed, n=None):
    """two unrelated images of full range"""
    g = np.random.default_rng(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    return g.integers(0, 256, shape, dtype=np.uint8), g.integers(0, 256, shape, dtype=np.uint8)
