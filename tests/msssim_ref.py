"""numpy restatement of include/fdn_msssim.h (multi-scale SSIM), in two forms that share the exact integer pyramid and nothing else:

  ordered   float64, every moment in the header's order (row pass, then column pass, r = r + g_t * x, no fused multiply-add: numpy rounds
            the product and the sum separately) - what the device is expected to reproduce bit for bit;
  truth     the direct 121-tap sum g_i g_j x in np.longdouble and the formulas in np.longdouble: another order and another precision,
            against which both the ordered form and the device are held to the a-priori bound of `bound`.

Also the independent input pairs of the tests and the host step."""
import math

import numpy as np

LEVELS, MIN_SIDE = 5, 161
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
U = 2.0 ** -53
K_BOUND = 128


def taps():
    """the 11 taps: exp(-(i - 5)^2 / (2 * 1.5^2)), normalised, float64 (fdn_hip.metrics.ssim3d_taps; the CPU test holds the two equal)"""
    i = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return k / k.sum()


def dims(h, w):
    """-> (five (h_s, w_s), five (h_s - 10, w_s - 10))"""
    lv = [(h, w)]
    for _ in range(LEVELS - 1):
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    return lv, [(a - 10, b - 10) for a, b in lv]


# ---- planes ---------------------------------------------------------------------------------------------------------------------------
def planes_u8(img, mode="rgb", bgr=True):
    """uint8 [h][w][3] -> (list of int64 planes, q0, L): R, G, B for rgb, the gray integer 299 R + 587 G + 114 B for gray"""
    x = img.astype(np.int64)
    r, g, b = (x[..., 2], x[..., 1], x[..., 0]) if bgr else (x[..., 0], x[..., 1], x[..., 2])
    if mode == "rgb":
        return [r, g, b], 1, 255
    return [299 * r + 587 * g + 114 * b], 1000, 255


def plane_luma(frame, h, w, bits):
    """one frame of samples, Y first -> (int64 plane, q0, L); a 10-bit code above 1023 counts as 1023"""
    y = np.asarray(frame).reshape(-1)[:h * w].astype(np.uint16 if bits == 10 else np.uint8).astype(np.int64).reshape(h, w)
    return (np.minimum(y, 1023) if bits == 10 else y), 1, (1 << bits) - 1


def downsample(x):
    """level s -> level s + 1: the sum over rows 2i, 2i + 1 and columns 2j, 2j + 1, an index equal to the size taken at size - 1"""
    h, w = x.shape
    i, j = np.arange((h + 1) // 2), np.arange((w + 1) // 2)
    r0, r1, c0, c1 = 2 * i, np.minimum(2 * i + 1, h - 1), 2 * j, np.minimum(2 * j + 1, w - 1)
    return x[r0][:, c0] + x[r0][:, c1] + x[r1][:, c0] + x[r1][:, c1]


def pyramid(plane):
    """-> the five levels, int64; level s is q0 * 4^s times the mean it stands for"""
    lv = [np.asarray(plane, dtype=np.int64)]
    for _ in range(LEVELS - 1):
        lv.append(downsample(lv[-1]))
    assert lv[-1].max() < 2 ** 31
    return lv


# ---- per level ------------------------------------------------------------------------------------------------------------------------
def constants(q0, L, s, dtype=np.float64):
    """C1', C2' of level s, multiplied left to right as the header writes them"""
    q = dtype(q0)
    for _ in range(s):
        q = q * dtype(4.0)
    k1, k2 = dtype(0.01) * dtype(L), dtype(0.03) * dtype(L)
    return k1 * k1 * q * q, k2 * k2 * q * q


def _moment_ordered(x, g):
    h, w = x.shape
    r = np.zeros((h, w - 10))
    for t in range(11):
        r = r + g[t] * x[:, t:t + w - 10]
    m = np.zeros((h - 10, w - 10))
    for t in range(11):
        m = m + g[t] * r[t:t + h - 10, :]
    return m


def level_ordered(a, b, q0, L, s, g=None):
    """int64 level-s planes a, b -> (cs, ss) float64 maps in the header's order"""
    g = taps() if g is None else g
    A, B = a.astype(np.float64), b.astype(np.float64)
    ma, mb, maa, mbb, mab = (_moment_ordered(x, g) for x in (A, B, A * A, B * B, A * B))
    c1, c2 = constants(q0, L, s)
    va, vb, vab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
    cs = (2.0 * vab + c2) / (va + vb + c2)
    l = (2.0 * (ma * mb) + c1) / (ma * ma + mb * mb + c1)
    return cs, l * cs


def _moment_truth(x, g2):
    h, w = x.shape
    m = np.zeros((h - 10, w - 10), dtype=np.longdouble)
    for i in range(11):
        for j in range(11):
            m += g2[i, j] * x[i:i + h - 10, j:j + w - 10]
    return m


def level_truth(a, b, q0, L, s, g=None):
    """-> (cs, ss, ratio) in np.longdouble from the direct 121-tap sums; ratio = (m_aa + m_bb + m_a^2 + m_b^2 + C2') / (va + vb + C2'),
    the conditioning the bound is stated in"""
    g = (taps() if g is None else g).astype(np.longdouble)
    g2 = np.outer(g, g)
    A, B = a.astype(np.longdouble), b.astype(np.longdouble)
    ma, mb, maa, mbb, mab = (_moment_truth(x, g2) for x in (A, B, A * A, B * B, A * B))
    # 0.01 and 0.03 are the doubles the device multiplies by: the constants are the header's values, formed without further rounding
    c1, c2 = (np.longdouble(c) for c in constants(q0, L, s))
    va, vb, vab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
    cs = (2 * vab + c2) / (va + vb + c2)
    l = (2 * (ma * mb) + c1) / (ma * ma + mb * mb + c1)
    ratio = (maa + mbb + ma * ma + mb * mb + c2) / (va + vb + c2)
    return cs, l * cs, ratio


def bound(ratio):
    """-> (bound on |d cs|, bound on |d ss|), float64 maps, from the truth's ratio: K U ratio and K U (ratio + 1), K = 128"""
    r = ratio.astype(np.float64)
    return K_BOUND * U * r, K_BOUND * U * (r + 1.0)


# ---- the host step --------------------------------------------------------------------------------------------------------------------
def from_means(means):
    """five unclamped means (cs of levels 0 .. 3, ss of level 4) -> MS-SSIM, math.pow in level order"""
    score = math.pow(max(means[0], 0.0), WEIGHTS[0])
    for s in range(1, LEVELS):
        score = score * math.pow(max(means[s], 0.0), WEIGHTS[s])
    return score


def plane_result(a, b, q0, L):
    """two int64 planes -> dict: pyr_a, pyr_b (five levels each), cs, ss (five ordered maps each), means, ms_ssim"""
    pa, pb = pyramid(a), pyramid(b)
    maps = [level_ordered(pa[s], pb[s], q0, L, s) for s in range(LEVELS)]
    cs, ss = [m[0] for m in maps], [m[1] for m in maps]
    means = [math.fsum(cs[s].ravel().tolist()) / cs[s].size for s in range(LEVELS - 1)] + [math.fsum(ss[-1].ravel().tolist()) / ss[-1].size]
    return {"pyr_a": pa, "pyr_b": pb, "cs": cs, "ss": ss, "means": means, "ms_ssim": from_means(means)}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
INPUTS = ("noise", "smooth", "inverse", "const", "same", "dark")


def smooth_field(h, w, seed=0):
    """uint8 [h][w][3]: waves a few pixels long in both axes, steep enough that every 11 x 11 window of every level sees a slope"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = 0.7 * seed
    ch = [127.5 + 120.0 * np.sin((x + 0.6 * y) / (2.2 + 0.3 * c) + ph + c) * np.cos((y - 0.4 * x) / (2.6 + 0.2 * c) + 0.5 * c) for c in range(3)]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


def pair(kind, h, w, seed=0):
    """-> (a, b) uint8 [h][w][3], one of INPUTS"""
    g = np.random.default_rng(1000 * h + w + 7919 * seed + INPUTS.index(kind))
    if kind == "noise":
        return g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "const":
        return np.full((h, w, 3), 255, np.uint8), np.full((h, w, 3), 254, np.uint8)
    if kind == "same":
        a = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        return a, a.copy()
    a = smooth_field(h, w, seed)
    if kind == "smooth":
        return a, np.clip(a.astype(np.int64) + g.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    if kind == "inverse":
        return a, (255 - a).astype(np.uint8)
    if kind == "dark":
        d = (a // 16).astype(np.uint8)
        return d, (d + g.integers(0, 3, a.shape)).astype(np.uint8)
    raise ValueError(kind)
