"""numpy restatement of include/fdn_fusion.h, in two forms.
  * the weights from the header's formulas in float64, or in np.longdouble (dtype=): the second judges the first;
  * the pyramid in any dtype, every operation in the header's order: in float32 it reproduces the device bit for bit (numpy rounds every
    float32 operation once and fuses nothing), in float64 it is the definition the properties of tests/test_fusion_cpu.py are held on.
imgs are [K,3,h,w] arrays, already cropped; clamp=False leaves the samples as they are."""
import math

import numpy as np

MAX_K, MAX_LEVELS, TILE = 16, 16, 32
SIGMA2 = 0.08000000000000002                                    # 2 * 0.2 ** 2 in double


def reflect(i, n):
    """indices i (any integers) into an axis of length n, reflected without repeating the edge sample"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    r = np.mod(i, p)
    return np.where(r < n, r, p - r)


def clamp01(x):
    return np.where(x < 0, 0, np.where(x > 1, 1, x)).astype(x.dtype)


def levels(h, w):
    return min(int(math.floor(math.log2(min(h, w)))), MAX_LEVELS)


def sizes(h, w):
    out = [(h, w)]
    for _ in range(levels(h, w)):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def gray(img, dt):
    """[3,h,w] of dtype dt -> [h,w]"""
    return dt(0.2989) * img[0] + dt(0.587) * img[1] + dt(0.114) * img[2]


def raw_weights(imgs, exponents=(1, 1, 1), dtype=np.float64, clamp=True):
    """-> [K,h,w] of dtype: W_k = C^wc S^ws E^we + 1e-12 before the normalisation"""
    dt = dtype
    K, _, h, w = imgs.shape
    x = clamp01(np.asarray(imgs, dtype=np.float32)) if clamp else np.asarray(imgs)
    x = x.astype(dt)
    wc, ws, we = (float(e) for e in exponents)
    yu, yd, xl, xr = reflect(np.arange(h) - 1, h), reflect(np.arange(h) + 1, h), reflect(np.arange(w) - 1, w), reflect(np.arange(w) + 1, w)
    out = np.empty((K, h, w), dtype=dt)

    def factor(v, e):
        return v if e == 1.0 else np.power(v, dt(e))
    for k in range(K):
        R, G, B = x[k]
        g = gray(x[k], dt)
        v = np.ones((h, w), dtype=dt)
        if wc != 0.0:
            v = v * factor(np.abs(dt(4) * g - g[yu, :] - g[yd, :] - g[:, xl] - g[:, xr]), wc)
        if ws != 0.0:
            m = (R + G + B) / dt(3)
            dr, dg, db = R - m, G - m, B - m
            v = v * factor(np.sqrt((dr * dr + dg * dg + db * db) / dt(3)), ws)
        if we != 0.0:
            dr, dg, db = R - dt(0.5), G - dt(0.5), B - dt(0.5)
            v = v * factor(np.exp(-(dr * dr + dg * dg + db * db) / dt(SIGMA2)), we)
        out[k] = v + dt(1e-12)
    return out


def weights(imgs, exponents=(1, 1, 1), dtype=np.float64, clamp=True):
    """-> [K,h,w] of dtype: the normalised weights, summed from 0 in k order"""
    raw = raw_weights(imgs, exponents, dtype, clamp)
    total = np.zeros(raw.shape[1:], dtype=dtype)
    for k in range(raw.shape[0]):
        total = total + raw[k]
    return raw / total


def tap5(a0, a1, a2, a3, a4, dt):
    return (((a0 + a4) + dt(4) * (a1 + a3)) + dt(6) * a2) * dt(0.0625)


def down(x):
    """[..., hs, ws] -> [..., (hs + 1) // 2, (ws + 1) // 2], rows first"""
    dt = x.dtype.type
    hs, ws = x.shape[-2:]
    if ws > 1:
        j = 2 * np.arange((ws + 1) // 2)
        x = tap5(*(x[..., reflect(j + d, ws)] for d in range(-2, 3)), dt)
    if hs > 1:
        i = 2 * np.arange((hs + 1) // 2)
        x = tap5(*(x[..., reflect(i + d, hs), :] for d in range(-2, 3)), dt)
    return np.ascontiguousarray(x)


def _up_axis(take, nc, n, dt):
    """one axis of up: take(indices) -> the coarse samples at those places of the axis, n the fine length"""
    i = np.arange(n)
    j = i // 2
    if nc == 1:
        return take(np.zeros(n, dtype=np.int64)), None, None
    even = ((take(reflect(j - 1, nc)) + take(reflect(j + 1, nc))) + dt(6) * take(j)) * dt(0.125)
    odd = (take(j) + take(reflect(j + 1, nc))) * dt(0.5)
    return even, odd, (i % 2 == 1)


def up(c, h, w):
    """[..., (h + 1) // 2, (w + 1) // 2] -> [..., h, w], along x and then along y"""
    dt = c.dtype.type
    hc, wc = c.shape[-2:]
    assert (hc, wc) == ((h + 1) // 2, (w + 1) // 2)
    even, odd, is_odd = _up_axis(lambda idx: c[..., idx], wc, w, dt)
    u = even if odd is None else np.where(is_odd, odd, even)
    even, odd, is_odd = _up_axis(lambda idx: u[..., idx, :], hc, h, dt)
    return np.ascontiguousarray(even if odd is None else np.where(is_odd[:, None], odd, even))


def weight_pyramid(wts):
    """[K,h,w] -> the Gaussian pyramid of the weight planes, levels 0 .. L"""
    out = [wts]
    for _ in range(levels(*wts.shape[-2:])):
        out.append(down(out[-1]))
    return out


def fuse_pyramid(imgs, wts, dtype=np.float32, clamp=True):
    """imgs [K,3,h,w], wts [K,h,w] -> [3,h,w] of dtype: blend and collapse in the header's order"""
    x = np.asarray(imgs, dtype=np.float32)
    x = (clamp01(x) if clamp else np.asarray(imgs)).astype(dtype)
    K, _, h, w = x.shape
    gi, gw = [x], weight_pyramid(np.asarray(wts).astype(dtype))
    L = levels(h, w)
    for _ in range(L):
        gi.append(down(gi[-1]))
    out = None
    for l in range(L, -1, -1):
        hl, wl = gi[l].shape[-2:]
        acc = np.zeros((3, hl, wl), dtype=dtype)
        for k in range(K):
            d = gi[l][k] if l == L else gi[l][k] - up(gi[l + 1][k], hl, wl)
            acc = acc + gw[l][k][None] * d
        out = acc if l == L else acc + up(out, hl, wl)
    return out


def fuse(imgs, exponents=(1, 1, 1), dtype=np.float64, clamp=True):
    """weights in float64, then the pyramid in dtype on them as they are (dtype float32: on their float32 roundings)"""
    return fuse_pyramid(imgs, weights(imgs, exponents, np.float64, clamp).astype(dtype), dtype, clamp)


def scene(h, w, K, seed=0, outside=True):
    """K renderings [K,3,h,w] float32 of one random scene, from dark to bright, the last with samples outside [0, 1] (outside=True, K > 1)"""
    g = np.random.default_rng(seed)
    base = g.random((3, h, w))
    gains = np.linspace(0.15, 1.6, K) if K > 1 else np.array([0.8])
    imgs = np.stack([base * a + 0.02 * g.standard_normal((3, h, w)) for a in gains]).astype(np.float32)
    if outside and K > 1:
        imgs[-1] = (base * 2.5 - 0.6).astype(np.float32)
    return imgs
