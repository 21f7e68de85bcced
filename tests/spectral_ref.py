"""A float64 numpy restatement of the Fourier evaluation (include/fdn_spectral.h, fdn_hip.spectral), written from the formulas and not from
the kernel: numpy.fft.rfft2, the band of a bin from its coordinates, the five sums per band, the derived figures.  Test tooling; the GPU
tests and tests/test_spectral_cpu.py judge the library against it, and the CPU test judges it on its own (Parseval, amp + pha = total).

With Xa, Xb the spectra of the restored image and of the ground truth, h the Hermitian weight of a half-spectrum bin (1 for kx = 0 and
kx = W/2, else 2) and the band of a bin as below, per band
    0  sum h |Xa - Xb|^2        1  sum h (|Xa| - |Xb|)^2        2  sum h max(0, 2 (|Xa| |Xb| - Re(Xa conj(Xb))))        3  sum h |Xb|^2
    4  sum |dRe| + |dIm|, unweighted."""
import math
from fractions import Fraction

import numpy as np

TERMS = 5


def band_of(ky, kx, H, W, nb):
    """the band of bin (ky, kx), in exact rational arithmetic: 0 for the zero-frequency bin, else 1 + min(floor(2 nb rho), nb - 1) with
    rho^2 = (ky' / H)^2 + (kx / W)^2, ky' = min(ky, H - ky)"""
    if ky == 0 and kx == 0:
        return 0
    kyp = min(ky, H - ky)
    rho2 = Fraction(kyp * kyp, H * H) + Fraction(kx * kx, W * W)
    t = 4 * nb * nb * rho2                                   # (2 nb rho)^2
    r0 = math.isqrt(t.numerator // t.denominator)            # floor(sqrt(t)) = isqrt(floor(t)) for t >= 0
    return 1 + min(r0, nb - 1)


def band_map(H, W, nb):
    """int array [H][W/2 + 1] of bands, by the integer rule on arrays (numpy int64): the largest r0 with r0^2 D <= q, q = 4 nb^2
    (ky'^2 W^2 + kx^2 H^2), D = H^2 W^2.  The squares are tested directly, with no square root at all: q is looked up among the
    thresholds r^2 D, r = 0 .. nb - 1 (r0 above nb - 1 changes nothing)."""
    ky = np.arange(H, dtype=np.int64)
    kyp = np.minimum(ky, H - ky)[:, None]
    kx = np.arange(W // 2 + 1, dtype=np.int64)[None, :]
    q = 4 * nb * nb * (kyp * kyp * (W * W) + kx * kx * (H * H))
    D = np.int64(H) * H * W * W
    thresholds = np.array([r * r for r in range(nb)], dtype=np.int64) * D
    band = np.searchsorted(thresholds, q.ravel(), side="right").reshape(q.shape)      # = 1 + the number of r >= 1 with r^2 D <= q
    band[0, 0] = 0
    return band


def weights(W):
    """Hermitian weights [W/2 + 1]"""
    h = np.full(W // 2 + 1, 2.0)
    h[0] = h[W // 2] = 1.0
    return h


def band_counts(H, W, nb):
    band = band_map(H, W, nb)
    h = np.broadcast_to(weights(W), band.shape)
    return [int(c) for c in np.bincount(band.ravel(), weights=h.ravel(), minlength=nb + 1)]      # sums of 1s and 2s below 2^53: exact


def band_counts_slow(H, W, nb):
    """the same from band_of, bin by bin (small shapes)"""
    out = [0] * (nb + 1)
    for ky in range(H):
        for kx in range(W // 2 + 1):
            out[band_of(ky, kx, H, W, nb)] += 1 if kx in (0, W // 2) else 2
    return out


def spectrum_sums(Xa, Xb, H, W, nb):
    """complex spectra [..., H, W/2 + 1] (any complex or float dtype: taken to float64 first) -> float64 [..., nb + 1, 5]"""
    Xa, Xb = np.asarray(Xa), np.asarray(Xb)
    ar, ai = Xa.real.astype(np.float64), Xa.imag.astype(np.float64)
    br, bi = Xb.real.astype(np.float64), Xb.imag.astype(np.float64)
    dr, di = ar - br, ai - bi
    ma, mb = np.sqrt(ar * ar + ai * ai), np.sqrt(br * br + bi * bi)
    h = weights(W)
    terms = [h * (dr * dr + di * di), h * (ma - mb) ** 2, h * np.maximum(0.0, 2.0 * (ma * mb - (ar * br + ai * bi))), h * (br * br + bi * bi),
             np.abs(dr) + np.abs(di)]
    band = band_map(H, W, nb)
    out = np.zeros(Xa.shape[:-2] + (nb + 1, TERMS))
    for b in range(nb + 1):
        m = band == b
        for t in range(TERMS):
            out[..., b, t] = terms[t][..., m].sum(axis=-1)
    return out


def pair_bands(a, b, nb):
    """images [..., H, W] (restored, ground truth) -> float64 [..., nb + 1, 5] through numpy.fft.rfft2 in float64"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    H, W = a.shape[-2:]
    return spectrum_sums(np.fft.rfft2(a), np.fft.rfft2(b), H, W, nb)


def _psnr(peak, mse):
    return float("inf") if mse == 0 else 10.0 * math.log10(peak * peak / mse)


def _ratio(x, y):
    return x / y if y != 0 else float("nan")


def metrics(sums, H, W, peak=1.0):
    """the derived figures of one image from its sums [C][nb + 1][5], the channels summed"""
    s = np.asarray(sums, dtype=np.float64).sum(axis=0)
    tot, amp, pha = s[:, 0].sum(), s[:, 1].sum(), s[:, 2].sum()
    C = len(sums)
    n = C * (float(H) * W) ** 2
    return {"mse": tot / n, "psnr": _psnr(peak, tot / n), "amp_share": _ratio(amp, amp + pha), "pha_share": _ratio(pha, amp + pha),
            "dc_share": _ratio(s[0, 0], tot), "psnr_amp": _psnr(peak, amp / n), "psnr_pha": _psnr(peak, pha / n),
            "fft_l1": s[:, 4].sum() / (C * H * (W // 2 + 1) * 2.0),
            "bands": [{"share": _ratio(p[0], tot), "amp_share": _ratio(p[1], amp + pha), "pha_share": _ratio(p[2], amp + pha),
                       "rel_err": _ratio(p[0], p[3])} for p in s]}


def fft_l1(a, b):
    """FFTLoss(reduction='mean') of an image pair [C][H][W] by the float64 formula: mean |d| over the real and imaginary parts of rfft2"""
    d = np.fft.rfft2(np.asarray(a, dtype=np.float64)) - np.fft.rfft2(np.asarray(b, dtype=np.float64))
    return float((np.abs(d.real) + np.abs(d.imag)).sum() / (2 * d.size))


def textured(h, w, seed, n=None):
    """textured uint8 images [h][w][3] (or [n][h][w][3]): waves of a few frequencies plus noise at moderate brightness"""
    g = np.random.default_rng(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    y, x = np.mgrid[0:h, 0:w]
    base = 110 + 50 * np.sin(0.37 * x + 0.11 * y) + 30 * np.cos(0.9 * y - 0.23 * x)
    img = base[..., None] + g.normal(0.0, 25.0, shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
