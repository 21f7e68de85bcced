"""NIQE restated in numpy, written here from the description of basicsr/metrics/niqe.py (not a copy): the model of what
csrc/niqe.hip computes, for checks on sizes the golden fixture does not hold.  The plane and the MSCN planes follow the reference's
float32 / float64 steps; the per-block sums are float64 (the reference takes float32 means), the table search is a nearest-entry search
on the increasing r_gam.  No scipy: the 7x7 window runs as 49 shifted float64 multiply-adds in the order scipy.ndimage.convolve uses."""
import math

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))


def tables():
    gam = np.arange(0.2, 10.001, 0.001)
    rec = 1.0 / gam
    g = np.vectorize(math.gamma)
    r_gam = g(rec * 2) ** 2 / (g(rec) * g(rec * 3))
    return gam, r_gam, np.sqrt(g(1 / gam) / g(3 / gam)), g(2 / gam) / g(1 / gam)


def plane(img, crop_border=0, input_order="CHW", convert_to="y"):
    """uint8 / float (C,H,W) B, G, R or (H,W) -> the float32 plane niqe() sees, cut to whole blocks"""
    x = np.asarray(img).astype(np.float32)
    if input_order != "HW":
        if x.shape[0] == 3 and convert_to == "y":
            f = (x / np.float32(255)).astype(np.float64)
            y = f[0] * 24.966 + f[1] * 128.553 + f[2] * 65.481 + 16.0
            x = (y / 255.0).astype(np.float32) * np.float32(255)
        elif x.shape[0] == 3 and convert_to == "gray":
            f = x / np.float32(255)
            x = ((f[0] * np.float32(0.114) + f[1] * np.float32(0.587)) + f[2] * np.float32(0.299)) * np.float32(255)
        elif x.shape[0] == 1 and convert_to == "y":
            x = (x[0] / np.float32(255)) * np.float32(255)
        else:
            raise ValueError((x.shape, convert_to))
    if crop_border:
        x = x[crop_border:-crop_border, crop_border:-crop_border]
    h, w = x.shape
    return np.ascontiguousarray(x[: h // BLOCK * BLOCK, : w // BLOCK * BLOCK])


def mscn(x, window):
    x = x.astype(np.float32)
    h, w = x.shape
    p = np.pad(x, 3, mode="edge").astype(np.float64)
    q = np.pad(np.square(x), 3, mode="edge").astype(np.float64)
    m = np.zeros((h, w))
    s = np.zeros((h, w))
    for a in range(7):
        for c in range(7):
            wt = window[6 - a, 6 - c]
            m = m + p[a:a + h, c:c + w] * wt
            s = s + q[a:a + h, c:c + w] * wt
    mu, ex2 = m.astype(np.float32), s.astype(np.float32)
    sigma = np.sqrt(np.abs(ex2 - np.square(mu)))
    return (x - mu) / (sigma + np.float32(1))


def half(x):
    """cv2.resize(x / 255., (w // 2, h // 2), INTER_LINEAR) * 255. at exactly half size: the 2x2 mean, float32"""
    f = x / np.float32(255)
    return ((((f[0::2, 0::2] + f[0::2, 1::2]) + f[1::2, 0::2]) + f[1::2, 1::2]) * np.float32(0.25)) * np.float32(255)


def aggd(v, tab):
    """v [nblocks][n] float32 -> alpha, beta_l, beta_r, table index per block (float64 sums)"""
    gam, r_gam, beta, _ = tab
    d = v.astype(np.float64)
    neg, pos = d < 0, d > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        left = np.sqrt((d * d * neg).sum(1) / neg.sum(1))
        right = np.sqrt((d * d * pos).sum(1) / pos.sum(1))
        gh = left / right
        n = d.shape[1]
        rhat = (np.abs(d).sum(1) / n) ** 2 / ((d * d).sum(1) / n)
        rn = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
    idx = np.clip(np.searchsorted(r_gam, rn, side="left"), 1, len(r_gam) - 1)
    lo = np.where((r_gam[idx] - rn) ** 2 < (r_gam[idx - 1] - rn) ** 2, idx, idx - 1)
    lo = np.where(np.isfinite(rn), lo, 0)
    return gam[lo], left * beta[lo], right * beta[lo], lo


def features(m, bs, tab):
    """MSCN plane -> [nblocks][18], blocks idx_w outer, idx_h inner; also the table indices [nblocks][5]"""
    h, w = m.shape
    nbh, nbw = h // bs, w // bs
    blocks = m.reshape(nbh, bs, nbw, bs).transpose(2, 0, 1, 3).reshape(nbh * nbw, bs, bs)
    out, idxs = [], []
    a, bl, br, i = aggd(blocks.reshape(len(blocks), -1), tab)
    out += [a, (bl + br) / 2]
    idxs.append(i)
    for s in SHIFTS:
        prod = blocks * np.roll(blocks, s, axis=(1, 2))
        a, bl, br, i = aggd(prod.reshape(len(blocks), -1), tab)
        out += [a, (br - bl) * tab[3][i], bl, br]
        idxs.append(i)
    return np.stack(out, axis=1), np.stack(idxs, axis=1)


def score(dist, mu_pris, cov_pris):
    ok = dist[~np.isnan(dist).any(axis=1)]
    mu = np.nanmean(dist, axis=0)
    cov = np.cov(ok, rowvar=False)
    inv = np.linalg.pinv((cov_pris + cov) / 2)
    d = mu_pris - mu
    return float(np.sqrt(d @ inv @ d.T).item())


def niqe(img, params, crop_border=0, input_order="CHW", convert_to="y", tab=None):
    """-> (score, {"plane", "mscn1", "mscn2", "feat1", "feat2", "idx1", "idx2"})"""
    tab = tables() if tab is None else tab
    p = plane(img, crop_border, input_order, convert_to)
    m1 = mscn(p, params["gaussian_window"])
    m2 = mscn(half(p), params["gaussian_window"])
    f1, i1 = features(m1, BLOCK, tab)
    f2, i2 = features(m2, BLOCK // 2, tab)
    q = score(np.concatenate([f1, f2], axis=1), params["mu_pris_param"], params["cov_pris_param"])
    return q, {"plane": p, "mscn1": m1, "mscn2": m2, "feat1": f1, "feat2": f2, "idx1": i1, "idx2": i2}


def _hash(idx, seed):
    """splitmix64 of (index, seed) in wrapping uint64 arithmetic: the same bits on every platform and numpy version"""
    with np.errstate(over="ignore"):
        z = idx.astype(np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _value_noise(seed, h, w, cell, amp):
    """integer value noise: random values on a grid of `cell` pixels, bilinear with integer weights, in [-amp, amp]"""
    gh, gw = h // cell + 2, w // cell + 2
    g = (_hash(np.arange(gh * gw), seed) % np.uint64(2 * amp + 1)).astype(np.int64).reshape(gh, gw) - amp
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    iy, fy, ix, fx = y // cell, y % cell, x // cell, x % cell
    v = (g[iy, ix] * (cell - fy) * (cell - fx) + g[iy, ix + 1] * (cell - fy) * fx + g[iy + 1, ix] * fy * (cell - fx)
         + g[iy + 1, ix + 1] * fy * fx)
    return v // (cell * cell)


def synth_u8(seed, h, w, dark=False):
    """a uint8 B, G, R frame (3, h, w) from integer arithmetic only, so the golden fixture can name it instead of storing it: shading
    at two scales, a checker of edges, fine texture and per-channel noise; dark = under-exposed with a flat black region"""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    tri = np.abs((x + 2 * y) % 74 - 37) - 18                                        # a slanted triangle wave, [-18, 19]
    v = (110 + _value_noise(seed, h, w, 48, 60) + _value_noise(seed + 1, h, w, 6, 14) + 25 * ((x // 40 + y // 56) % 2) + tri
         + _value_noise(seed + 2, h, w, 2, 6))
    n = (_hash(np.arange(3 * h * w), seed + 3) % np.uint64(3)).astype(np.int64).reshape(3, h, w) - 1
    img = np.stack([v * 4 // 5 + 10, v, v * 9 // 10 - 5]) + n
    if dark:
        img = img // 4 - 8
        img[:, : h // 2, : w // 3] = 0
    return np.clip(img, 0, 255).astype(np.uint8)


def load_fixture(here):
    """tests/golden/niqe.npz (make_golden_niqe.py) -> (arrays, cases, params, image(name) -> the uint8 input of a case).  The inputs are
    not stored: a case names a window of a synth_u8 frame (meta "src": [seed, h, w, dark, channel or None, y0, x0, h, w]), and the
    fixture keeps a CRC-32 of each frame to show that this generator still makes the frames the reference scored."""
    import json
    import os
    import zlib
    z = np.load(os.path.join(here, "golden", "niqe.npz"))
    cases = json.loads(z["cases_json"].tobytes())
    params = dict(np.load(os.path.join(here, "golden", "niqe_pris_params.npz")))

    def image(name):
        seed, fh, fw, dark, c, y0, x0, h, w = cases[name]["src"]
        a = synth_u8(seed, fh, fw, dark)
        assert zlib.crc32(a.tobytes()) == cases[name]["crc32"], name
        return a[:, y0:y0 + h, x0:x0 + w] if c is None else a[c, y0:y0 + h, x0:x0 + w]
    return z, cases, params, image


def alpha_index(alpha):
    """the table index of an alpha of the grid (gam[i] is within 1e-12 of 0.2 + i * 0.001)"""
    return np.rint((np.asarray(alpha) - 0.2) / 0.001).astype(np.int64)


ALPHA_COLS = (0, 2, 6, 10, 14)           # the alpha of each of the five fits in a row of 18 features
MEAN_COLS = (3, 7, 11, 15)               # the AGGD mean (beta_r - beta_l) * G(2/a) / G(1/a) of the four product fits
BETA_COLS = ((4, 5), (8, 9), (12, 13), (16, 17))


def compare_feats(got, want, tab):
    """got, want [nblocks][18] -> (alpha index identical [nblocks][5], largest |index difference|, worst relative error of the other
    features where the index agrees).  The AGGD mean is a difference of two betas that nearly cancel in some blocks, so its error is
    taken relative to max(|beta_l|, |beta_r|) * G(2/a) / G(1/a), the size of its terms; every other feature relative to itself."""
    ig, iw = alpha_index(got[:, ALPHA_COLS]), alpha_index(want[:, ALPHA_COLS])
    same = ig == iw
    mask = np.repeat(same, [2, 4, 4, 4, 4], axis=1) & np.isfinite(want)
    scale = np.abs(want).copy()
    for k, (m, (bl, br)) in enumerate(zip(MEAN_COLS, BETA_COLS)):
        scale[:, m] = np.maximum(np.abs(want[:, bl]), np.abs(want[:, br])) * tab[3][np.clip(iw[:, k + 1], 0, len(tab[3]) - 1)]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(got - want) / scale
    worst = float(rel[mask].max()) if mask.any() else 0.0
    return same, int(np.abs(ig - iw).max()), worst
