"""The yardstick of the low-light evaluation (include/fdn_lowlight.h), restated in numpy: the lightness order error by brute force over
all pairs and from the joint histogram, its sample rule, and sRGB -> CIELAB -> CIEDE2000 (Sharma, Wu, Dalal 2005) with a dtype parameter,
so that the float64 formula can be judged against itself in np.longdouble.  Nothing here touches the GPU or the library."""
import numpy as np


def sample_dims(h, w, size):
    """(Md, Nd): every pixel for size == 0 or min(h, w) <= size, else h size / s and w size / s rounded half up, s = min(h, w)"""
    s = min(h, w)
    if size == 0 or s <= size:
        return h, w
    return (2 * h * size + s) // (2 * s), (2 * w * size + s) // (2 * s)


def sample_idx(n, nd):
    """source index of each of nd samples along an axis of n"""
    return ((2 * np.arange(nd, dtype=np.int64) + 1) * n) // (2 * nd)


def loe_sets(a, b, size):
    """a, b uint8 (h, w, 3) -> (La, Lb) int64 [Md][Nd] of the samples"""
    h, w = a.shape[:2]
    La, Lb = a.max(2).astype(np.int64), b.max(2).astype(np.int64)
    md, nd = sample_dims(h, w, size)
    if (md, nd) != (h, w):
        ii, jj = sample_idx(h, md), sample_idx(w, nd)
        La, Lb = La[np.ix_(ii, jj)], Lb[np.ix_(ii, jj)]
    return La, Lb


def loe_brute(a, b, size):
    """-> (numerator, m) by comparing every sample with every other"""
    x, y = (v.ravel() for v in loe_sets(a, b, size))
    f = (x[:, None] >= x[None, :]) != (y[:, None] >= y[None, :])
    return int(f.sum()), x.size


def loe_tables(x, y):
    """J, C, R, K of the lightness values x, y (any shape)"""
    J = np.zeros((256, 256), np.int64)
    np.add.at(J, (x.ravel(), y.ravel()), 1)
    C = J.cumsum(0).cumsum(1)
    return J, C, C[:, 255], C[255, :]


def loe_hist(a, b, size):
    """-> (numerator, m) from the joint histogram"""
    x, y = loe_sets(a, b, size)
    J, C, R, K = loe_tables(x, y)
    return int((J * (R[:, None] + K[None, :] - 2 * C)).sum()), x.size


def loe_map(a, b, size):
    """-> RD of every sample, int64 [Md][Nd]"""
    x, y = loe_sets(a, b, size)
    J, C, R, K = loe_tables(x, y)
    return R[x] + K[y] - 2 * C[x, y]


M = ((0.4124564, 0.3575761, 0.1804375), (0.2126729, 0.7151522, 0.0721750), (0.0193339, 0.1191920, 0.9503041))
WHITE = (0.95047, 1.0, 1.08883)


def lab(rgb, ft=np.float64):
    """uint8 [..., 3] R, G, B -> CIELAB [..., 3] in the float type ft; each row of the matrix is summed left to right"""
    c = rgb.astype(ft) / ft(255)
    lin = np.where(c <= ft(0.04045), c / ft(12.92), ((c + ft(0.055)) / ft(1.055)) ** ft(2.4))
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    d = ft(6) / ft(29)
    f = []
    for row, wp in zip(M, WHITE):
        t = (ft(row[0]) * r + ft(row[1]) * g + ft(row[2]) * b) / ft(wp)
        f.append(np.where(t > d * d * d, np.cbrt(t), t / (ft(3) * d * d) + ft(4) / ft(29)))
    return np.stack([ft(116) * f[1] - ft(16), ft(500) * (f[0] - f[1]), ft(200) * (f[1] - f[2])], -1)


def de00(l1, l2, ft=np.float64):
    """CIEDE2000 of CIELAB [..., 3] arrays, kL = kC = kH = 1"""
    L1, a1, b1 = [l1[..., i].astype(ft) for i in range(3)]
    L2, a2, b2 = [l2[..., i].astype(ft) for i in range(3)]
    p25 = ft(6103515625)                                   # 25^7
    C1, C2 = np.hypot(a1, b1), np.hypot(a2, b2)
    Cb = (C1 + C2) / ft(2)
    Cb7 = Cb ** ft(7)
    G = ft(0.5) * (ft(1) - np.sqrt(Cb7 / (Cb7 + p25)))
    a1p, a2p = (ft(1) + G) * a1, (ft(1) + G) * a2
    C1p, C2p = np.hypot(a1p, b1), np.hypot(a2p, b2)
    h1 = np.where((a1p == 0) & (b1 == 0), ft(0), np.degrees(np.arctan2(b1, a1p)) % ft(360))
    h2 = np.where((a2p == 0) & (b2 == 0), ft(0), np.degrees(np.arctan2(b2, a2p)) % ft(360))
    dL, dC = L2 - L1, C2p - C1p
    dh = h2 - h1
    z = (C1p * C2p) == 0
    dh = np.where(z, ft(0), np.where(dh > 180, dh - ft(360), np.where(dh < -180, dh + ft(360), dh)))
    dH = ft(2) * np.sqrt(C1p * C2p) * np.sin(np.radians(dh / ft(2)))
    Lb, Cbp = (L1 + L2) / ft(2), (C1p + C2p) / ft(2)
    hs, ad = h1 + h2, np.abs(h1 - h2)
    hb = np.where(z, hs, np.where(ad <= 180, hs / ft(2), np.where(hs < 360, (hs + ft(360)) / ft(2), (hs - ft(360)) / ft(2))))
    T = (ft(1) - ft(0.17) * np.cos(np.radians(hb - ft(30))) + ft(0.24) * np.cos(np.radians(ft(2) * hb))
         + ft(0.32) * np.cos(np.radians(ft(3) * hb + ft(6))) - ft(0.20) * np.cos(np.radians(ft(4) * hb - ft(63))))
    u = (hb - ft(275)) / ft(25)
    dth = ft(30) * np.exp(-(u * u))
    Cp7 = Cbp ** ft(7)
    Rc = ft(2) * np.sqrt(Cp7 / (Cp7 + p25))
    l2_ = (Lb - ft(50)) * (Lb - ft(50))
    Sl = ft(1) + ft(0.015) * l2_ / np.sqrt(ft(20) + l2_)
    Sc = ft(1) + ft(0.045) * Cbp
    Sh = ft(1) + ft(0.015) * Cbp * T
    Rt = -np.sin(np.radians(ft(2) * dth)) * Rc
    tl, tc, th = dL / Sl, dC / Sc, dH / Sh
    return np.sqrt(tl * tl + tc * tc + th * th + Rt * tc * th)


def deltae_u8(a, b, ft=np.float64):
    """a (ground truth), b (restored) uint8 [..., 3] R, G, B -> dE00 per pixel"""
    return de00(lab(a, ft), lab(b, ft), ft)


def dark_pair(h, w, seed):
    """a dark image and a brightened, noisy version of it, uint8 (h, w, 3): the inputs the identity was first checked with"""
    g = np.random.default_rng(seed)
    a = g.integers(0, 40, (h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) * 5 + g.integers(-20, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    return a, b
