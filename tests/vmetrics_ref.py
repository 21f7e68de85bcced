"""numpy restatement of the video evaluation (include/fdn_vmetrics.h, fdn_hip/video_metrics.py): squared errors and luma sums as plain
integers, the luma SSIM as the reference's _ssim_cly (basicsr/metrics/psnr_ssim.py:202-240) written separably in float64 with
np.pad(mode="edge"), scene cuts and the flicker figures on integers and Fractions.  The yardstick of tests/test_gpu_vmetrics.py;
tests/test_vmetrics_cpu.py judges it on its own (against oracle.fdn_oracle._ssim_planes and by hand)."""
import math
from fractions import Fraction

import numpy as np

from yuv_ref import PIX_FMTS, pack, random_frames, sample_dtype, unpack  # noqa: F401  (the frame helpers, shared)

# shapes of the GPU tests (h, w, B): see the table in tests/test_gpu_vmetrics.py
SHAPES = [(2, 2, 1), (2, 4, 1), (12, 14, 1), (34, 38, 2), (70, 514, 2)]


def top_code(pix_fmt):
    return 2 ** PIX_FMTS[pix_fmt][1] - 1


def planes(frames, h, w, pix_fmt):
    """frames [B, h*w*3/2] -> int64 planes y, u, v with a 10-bit word above 1023 counted as 1023"""
    return unpack(np.minimum(frames.astype(np.int64), top_code(pix_fmt)), h, w, pix_fmt)


def pair_stats(a, b, h, w, pix_fmt):
    """-> list of B tuples of Python ints (SSE_Y, SSE_Cb, SSE_Cr, sum of a's luma, sum of b's luma); b None: (0, 0, 0, sum, 0)"""
    ya, ua, va = planes(a, h, w, pix_fmt)
    if b is None:
        return [(0, 0, 0, int(ya[i].sum()), 0) for i in range(a.shape[0])]
    yb, ub, vb = planes(b, h, w, pix_fmt)
    return [(int(((ya[i] - yb[i]) ** 2).sum()), int(((ua[i] - ub[i]) ** 2).sum()), int(((va[i] - vb[i]) ** 2).sum()), int(ya[i].sum()),
             int(yb[i].sum())) for i in range(a.shape[0])]


def taps():
    """cv2.getGaussianKernel(11, 1.5) in float64"""
    i = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return k / k.sum()


def _filter(p, k):
    """the 11 x 11 window outer(k, k) over a float64 plane, border replicated: along W, then along H"""
    h, w = p.shape
    q = np.pad(p, 5, mode="edge")
    rows = sum(k[t] * q[:, t:t + w] for t in range(11))
    return sum(k[t] * rows[t:t + h] for t in range(11))


def ssim_plane(a, b, bits):
    """mean of the SSIM map of two integer planes, C1 / C2 for L = 2^bits - 1, whole map (no crop)"""
    L = 2 ** bits - 1
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    a, b, k = a.astype(np.float64), b.astype(np.float64), taps()
    mu1, mu2 = _filter(a, k), _filter(b, k)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = _filter(a * a, k) - mu1_sq, _filter(b * b, k) - mu2_sq, _filter(a * b, k) - mu12
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return float(m.mean())


def ssim_y(a, b, h, w, pix_fmt):
    """-> list of B floats"""
    ya, yb = planes(a, h, w, pix_fmt)[0], planes(b, h, w, pix_fmt)[0]
    return [ssim_plane(ya[i], yb[i], PIX_FMTS[pix_fmt][1]) for i in range(a.shape[0])]


def luma_hist(frames, h, w, pix_fmt):
    """-> int64 [B, 256]: bin = code >> (bits - 8) after the clamp"""
    y = planes(frames, h, w, pix_fmt)[0] >> (PIX_FMTS[pix_fmt][1] - 8)
    return np.stack([np.bincount(y[i].reshape(-1), minlength=256) for i in range(frames.shape[0])]).astype(np.int64)


def psnr(sse, n, bits):
    if sse == 0:
        return float("inf")
    L = 2 ** bits - 1
    return 10.0 * math.log10(L * L * n / sse)


def cut_above(cut, h, w):
    return math.floor(Fraction(cut) * (2 * h * w))


def records(dist, ref, h, w, pix_fmt, cut=0.3):
    """the per-frame records of VideoScore for a whole stream -> list of dicts.  A frame is a cut when it is the first or when the L1
    distance of its luma histogram (of ref when there is one, else of dist) from the previous frame's exceeds floor(cut 2 h w); PSNR per
    plane and pooled over h w 3 / 2 samples, on the codes; mean_y = S / (h w 2^(bits-8)); dmean the difference of two such sums, formed
    exactly, None at a cut."""
    bits = PIX_FMTS[pix_fmt][1]
    stats = pair_stats(dist, ref, h, w, pix_fmt)
    hist = luma_hist(dist if ref is None else ref, h, w, pix_fmt)
    ssim = ssim_y(dist, ref, h, w, pix_fmt) if ref is not None else None
    above, unit = cut_above(cut, h, w), h * w * 2 ** (bits - 8)
    out = []
    for t, st in enumerate(stats):
        is_cut = t == 0 or int(np.abs(hist[t] - hist[t - 1]).sum()) > above
        r = {"psnr_y": None, "psnr_u": None, "psnr_v": None, "psnr_avg": None, "ssim_y": None, "mean_y": float(Fraction(st[3], unit)),
             "mean_y_ref": None, "cut": is_cut, "dmean": None, "dmean_ref": None}
        if ref is not None:
            r.update(psnr_y=psnr(st[0], h * w, bits), psnr_u=psnr(st[1], h * w // 4, bits), psnr_v=psnr(st[2], h * w // 4, bits),
                     psnr_avg=psnr(st[0] + st[1] + st[2], h * w * 3 // 2, bits), ssim_y=ssim[t], mean_y_ref=float(Fraction(st[4], unit)))
        if not is_cut:
            r["dmean"] = float(Fraction(st[3] - stats[t - 1][3], unit))
            if ref is not None:
                r["dmean_ref"] = float(Fraction(st[4] - stats[t - 1][4], unit))
        out.append(r)
    return out


def flicker(recs):
    """-> (flicker, flicker_ref, flicker_err): means of |dmean|, |dmean_ref|, |dmean - dmean_ref| over the frames that are no cut"""
    def mean(v):
        return math.fsum(v) / len(v) if v else float("nan")
    d = [r for r in recs if not r["cut"]]
    both = [r for r in d if r["dmean_ref"] is not None]
    return (mean([abs(r["dmean"]) for r in d]), mean([abs(r["dmean_ref"]) for r in both]),
            mean([abs(r["dmean"] - r["dmean_ref"]) for r in both]))


def scene_stream(pix_fmt, seed=3, h=34, w=38, n=7, change_at=4):
    """(ref, dist) streams of n frames: dim noisy luma up to frame change_at - 1, bright from there on (every luma sample changes its bin, so
    more than 30 % do); within a scene the frames differ by noise and a small brightness drift.  dist = ref with a per-frame luma offset (the
    flicker) and noise on every plane."""
    bits = PIX_FMTS[pix_fmt][1]
    s, top = 2 ** (bits - 8), 2 ** bits - 1
    rng = np.random.default_rng(seed)
    base = [rng.integers(20 * s, 36 * s, size=(h, w)), rng.integers(150 * s, 166 * s, size=(h, w))]
    c = rng.integers(100 * s, 140 * s, size=(2, h // 2, w // 2))
    ref_y = np.stack([base[t >= change_at] + rng.integers(0, 2 * s, size=(h, w)) + (t % 3) * s for t in range(n)])
    ref_u, ref_v = np.stack([c[0]] * n), np.stack([c[1]] * n)
    offs = np.array([0, 1, -1, 2, 1, -1, 1][:n]) * s
    d_y = np.clip(ref_y + offs[:, None, None] + rng.integers(-2 * s, 2 * s + 1, size=ref_y.shape), 0, top)
    d_u = np.clip(ref_u + rng.integers(-3, 4, size=ref_u.shape), 0, top)
    d_v = np.clip(ref_v + rng.integers(-1, 2, size=ref_v.shape), 0, top)
    return pack(ref_y, ref_u, ref_v, pix_fmt), pack(d_y, d_u, d_v, pix_fmt)
