"""Brightness-corrected PSNR / SSIM of 8-bit image pairs (include/fdn_correct.h, libfdn_correct.so): the restored image is mapped, channel
by channel, by one affine function towards its ground truth and then scored as fdn_hip.metrics.calculate_psnr_ssim_u8 scores it.  FDN's
output brightness hangs on one predicted scalar, the ratio; a score that removes global brightness tells a wrong ratio from a wrong picture.

`mode="mean_var"` is the reference's scripts/metrics/calculate_psnr_ssim.py --correct_mean_var (:38-54): every channel of the restored
image is shifted and scaled to the ground truth's mean and standard deviation.  The reference does it in float32 and "twice"; in exact
arithmetic the second pass only undoes the mean shift the first pass's scaling introduced, so the whole is the single map
    z = (x - m_r) * s + m_g,     m = S / N,     s = sqrt((N Q_g - S_g^2) / (N Q_r - S_r^2))
with S = sum x, Q = sum x^2 over the N pixels of the channel (g: ground truth, r: restored).

`mode="gt_mean"` is NOT in the reference checkout; it is defined here by this formula, the convention under which KinD, LLFlow and
Retinexformer (--GT_mean) report LOL-v1 numbers: the restored image times
    s = (299 R_g + 587 G_g + 114 B_g) / (299 R_r + 587 G_r + 114 B_r)
(R, G, B the channel sums: the ratio of the mean grays), clipped to [0, 255].

All statistics are of the WHOLE image (the reference corrects before it crops) and are exact: int64 sums from the device, Python
integers here, then one division (and one math.sqrt) in double.  The corrected sample is formed in double, one rounding per operation,
and rounded once to float32; it exists only inside the scoring launch (no float copy of the images in memory) unless `corrected_u8` is
asked for it.  A flat restored channel (mean_var) or a black restored image (gt_mean) has no correction: its coefficients, PSNR and SSIM
are NaN, which is what numpy's 0 / 0 gives the reference; the other images of the batch are not affected.  No CPU fallback."""
import ctypes
import math
import os

import numpy as np
import torch

from . import FdnHipError, _declare, check, ptr, stream
from ._abi_correct import PROTOTYPES, VERSION      # generated from include/fdn_correct.h by tools/gen_abi_table.py

MODES = ("gt_mean", "mean_var")
PAIR_MOMENTS = 13                                         # FDN_PAIR_MOMENTS of include/fdn_correct.h: S_g[3], Q_g[3], S_r[3], Q_r[3], max of cropped gt
ABI_VERSION = VERSION[1]

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_correct.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_correct.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has correct ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def check_mode(mode):
    if mode not in MODES:
        raise FdnHipError(f"correction mode must be one of {', '.join(MODES)}, got {mode!r}")
    return mode


def correction_coefficients(moments, mode, bgr=True, *, n):
    """moments: per image the 13 integers of fdn_pair_moments_fold, n: pixels per image -> per image [3][5] doubles m_r, s, m_g, lo, hi
    (the coef of include/fdn_correct.h).  Host only: Python integers, one division (and one square root) in double.  A zero denominator
    gives NaN for s: the channel (mean_var) or the image (gt_mean) has no correction."""
    check_mode(mode)
    n = int(n)
    if n < 1:
        raise FdnHipError(f"n, the number of pixels per image, must be >= 1, got {n}")
    nan, inf = float("nan"), float("inf")
    out = []
    for m in moments:
        m = [int(v) for v in m]
        if len(m) != PAIR_MOMENTS:
            raise FdnHipError(f"an image has {PAIR_MOMENTS} moments, got {len(m)}")
        sg, qg, sr, qr = m[0:3], m[3:6], m[6:9], m[9:12]
        if mode == "mean_var":
            rows = []
            for c in range(3):
                num, den = n * qg[c] - sg[c] * sg[c], n * qr[c] - sr[c] * sr[c]              # N^2 times the variances, exact
                s = math.sqrt(float(num) / float(den)) if den else nan
                rows.append([sr[c] / n, s, sg[c] / n, -inf, inf])
        else:
            wts = (114, 587, 299) if bgr else (299, 587, 114)                                # gray = 0.299 R + 0.587 G + 0.114 B
            num, den = sum(k * v for k, v in zip(wts, sg)), sum(k * v for k, v in zip(wts, sr))
            s = float(num) / float(den) if den else nan
            rows = [[0.0, s, 0.0, 0.0, 255.0] for _ in range(3)]
        out.append(rows)
    return out


def _pair(gt, restored, crop_border, what):
    from .metrics import _u8_pair
    a, b, single = _u8_pair(gt, restored, crop_border, what)
    if a.shape[1] * a.shape[2] > 2 ** 31 - 1:
        raise FdnHipError(f"{what}: {a.shape[1]}x{a.shape[2]} has more than 2^31 - 1 pixels")
    return a, b, single


def _moments(a, b, cb):
    """enqueue fdn_pair_moments_u8 and its fold on contiguous device tensors -> int64 [B][13] on the device"""
    from .metrics import PAIR_PARTS
    B, h, w, _ = a.shape
    l = lib()
    parts = torch.empty((B, PAIR_PARTS, PAIR_MOMENTS), dtype=torch.int64, device=a.device)
    folded = torch.empty((B, PAIR_MOMENTS), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        s = stream()
        check(l.fdn_pair_moments_u8(ptr(a), ptr(b), B, h, w, cb, ptr(parts), s), "fdn_pair_moments_u8")
        check(l.fdn_pair_moments_fold(ptr(parts), B, ptr(folded), s), "fdn_pair_moments_fold")
    return folded


def _coefficients(a, b, cb, mode, bgr):
    """-> (coef float64 [B][3][5] and is255 int32 [B] on the device, the host's coefficient rows and maxima of the cropped ground truth)"""
    host = _moments(a, b, cb).cpu().tolist()                                                 # the one copy of the moments
    rows = correction_coefficients(host, mode, bgr, n=a.shape[1] * a.shape[2])
    mx = [m[12] for m in host]
    coef = torch.tensor(rows, dtype=torch.float64).to(a.device)
    is255 = torch.tensor([int(v > 1) for v in mx], dtype=torch.int32).to(a.device)           # img1.max() <= 1 -> peak 1 (psnr_ssim.py:60, :311)
    return coef, is255, rows, mx


def _apply(b, coef):
    B, h, w, _ = b.shape
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device=b.device)
    with torch.cuda.device(b.device):
        check(lib().fdn_pair_apply_u8(ptr(b), ptr(coef), B, h, w, ptr(out), stream()), "fdn_pair_apply_u8")
    return out


def _corrected_launch(a, b, cb, coef, is255, out):
    """enqueue fdn_pair_corrected_u8; out: float64 [B][2] on the device"""
    from .metrics import ssim3d_channel_matrix, ssim3d_taps
    B, h, w, _ = a.shape
    l = lib()
    nws = int(l.fdn_pair_corrected_ws(B, h, w, cb))
    if nws <= 0:
        raise FdnHipError(f"fdn_pair_corrected_ws refuses {B} images of {h}x{w} with crop_border={cb}")
    ws = torch.empty(nws, dtype=torch.float64, device=a.device)
    taps, mix = ssim3d_taps(), np.ascontiguousarray(ssim3d_channel_matrix())
    with torch.cuda.device(a.device):
        check(l.fdn_pair_corrected_u8(ptr(a), ptr(b), B, h, w, cb, ptr(coef), ptr(is255), taps.ctypes.data_as(ctypes.c_void_p),
                                      mix.ctypes.data_as(ctypes.c_void_p), ptr(ws), ptr(out), stream()), "fdn_pair_corrected_u8")


def calculate_psnr_ssim_corrected_u8(gt, restored, mode, crop_border=0, test_y_channel=False, ssim3d=True, bgr=True):
    """calculate_psnr and calculate_ssim (basicsr/metrics/psnr_ssim.py) of img1 = gt (the bytes) and img2 = the corrected restored image
    (float32, code units 0 .. 255): (h,w,3) or (B,h,w,3) uint8 numpy arrays or tensors -> (psnr, ssim), two floats for one pair, two lists
    of B floats for a batch, as calculate_psnr_ssim_u8 returns them.  mode: "mean_var" or "gt_mean" (the module's docstring).  The
    ground truth decides the peak value (its maximum over the cropped region <= 1 -> 1, else 255).  The default branch (RGB PSNR with the
    squared error summed in float64, 3-D SSIM) is one pass for the moments and one tiled launch over the whole batch, with one small
    device-to-host copy of the folded moments and one of the scores; the scores have the same bits on every call and do not depend on
    the rest of the batch.  test_y_channel=True and ssim3d=False go image by image through the float32 entry points
    (metrics.calculate_psnr / calculate_ssim) on the corrected planes.  bgr: the channels are B, G, R, else R, G, B (gt_mean's gray and
    the Y channel depend on it)."""
    check_mode(mode)                                                                         # before the device is touched
    from .metrics import _psnr_from_sse, calculate_psnr, calculate_ssim
    a, b, single = _pair(gt, restored, crop_border, "calculate_psnr_ssim_corrected_u8")
    cb = int(crop_border)
    B, h, w, _ = a.shape
    coef, is255, rows, mx = _coefficients(a, b, cb, mode, bgr)
    if test_y_channel or not ssim3d:
        z = _apply(b, coef)
        psnr, ssim = [], []
        for i in range(B):
            if any(math.isnan(v) for row in rows[i] for v in row):
                psnr.append(float("nan"))
                ssim.append(float("nan"))
                continue
            x, y = a[i].permute(2, 0, 1).to(torch.float32), z[i]                             # (3,h,w) planes, values 0..255
            if test_y_channel and not bgr:
                x, y = x.flip(0), y.flip(0)
            psnr.append(calculate_psnr(x, y, cb, test_y_channel))
            ssim.append(calculate_ssim(x, y, cb, test_y_channel, ssim3d))
    else:
        out = torch.empty((B, 2), dtype=torch.float64, device=a.device)
        _corrected_launch(a, b, cb, coef, is255, out)
        res = out.cpu().tolist()                                                             # the one copy of the scores: [B][sse, ssim]
        n = 3 * (h - 2 * cb) * (w - 2 * cb)
        psnr = [_psnr_from_sse(r[0], m, n) for r, m in zip(res, mx)]
        ssim = [r[1] for r in res]
    return (psnr[0], ssim[0]) if single else (psnr, ssim)


def corrected_u8(gt, restored, mode, bgr=True):
    """-> the corrected restored image, float32 [B][3][h][w] on the device (B = 1 for one (h,w,3) pair), planes in the channel order of
    the bytes, code units 0 .. 255 (mean_var is not clipped; gt_mean is, to [0, 255])"""
    check_mode(mode)
    a, b, _ = _pair(gt, restored, 0, "corrected_u8")
    return _apply(b, _coefficients(a, b, 0, mode, bgr)[0])
