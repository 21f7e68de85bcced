"""Fourier evaluation (include/fdn_spectral.h): how much of the error of a restored image is a brightness error and how much a structure
or blur error, and at which frequencies.  FDN rests on the claim that low light shows in the amplitude of an image's spectrum and blur in
its phase; with Xa, Xb the spectra of the restored image and of the ground truth the squared error of every bin splits exactly,

    |Xa - Xb|^2  =  (|Xa| - |Xb|)^2  +  2 (|Xa| |Xb| - Re(Xa conj(Xb)))
       total         amplitude part            phase part  (= 2 |Xa| |Xb| (1 - cos dphi) >= 0)

and by Parseval the left side, summed over the full spectrum and divided by (H W)^2, is the squared error of the image pair: the MSE
behind PSNR falls apart into an amplitude share and a phase share per radial frequency band.  Band 0 is the zero-frequency bin alone
(the global brightness offset); bands 1 .. n cut the radial frequency rho (cycles per pixel) at multiples of 0.5 / n, and the corners of
the spectrum beyond rho = 0.5 fall into band n.  `fft_l1` is the FFT term of the loss the reference trains with (FFTLoss,
basicsr/models/losses/losses.py:109-115, options/train/FDN.yml): the mean of |dRe| and |dIm| over the half spectrum of rfft2.

The spectrum is fdn_rfft_rows followed by fdn_fft_cols_c2c (float32, unscaled), the sums per band are float64 and run in a fixed order:
a pair scores the same bits on every call and wherever it sits in a batch.  Everything is enqueued on the current stream; only
fourier_metrics and calculate_fourier copy the few words per image back (which synchronises).  No CPU fallback."""
import ctypes
import math

import numpy as np
import torch

from . import FdnHipError, check, lib, ptr, stream
from . import ops

TERMS = 5                       # per band: total, amplitude part, phase part, the ground truth's energy, sum |dRe| + |dIm|
MAX_H, MAX_W, MAX_BANDS = 4096, 10240, 32


def _bands(bands):
    if isinstance(bands, bool) or not isinstance(bands, int) or not 1 <= bands <= MAX_BANDS:
        raise FdnHipError(f"bands must be an integer in 1 .. {MAX_BANDS}, got {bands!r}")
    return bands


def _size(H, W):
    if not 1 <= H <= MAX_H:
        raise FdnHipError(f"height {H}: the band sums take 1 .. {MAX_H} rows")
    if W % 2:
        raise FdnHipError(f"odd width {W}: the real FFT here takes even widths only, and nothing is cropped silently")
    if not 2 <= W <= MAX_W:
        raise FdnHipError(f"width {W}: the band sums take 2 .. {MAX_W} columns")


def _real(x, what, dims=None):
    if not isinstance(x, torch.Tensor):
        raise FdnHipError(f"{what} must be a torch tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise FdnHipError(f"{what} must live on a ROCm device (got {x.device}); Fourier evaluation has no CPU fallback")
    if x.dtype != torch.float32:
        raise FdnHipError(f"{what} must be float32 (got {x.dtype})")
    if (dims is not None and x.dim() != dims) or x.dim() < 2 or x.numel() == 0:
        raise FdnHipError(f"{what} must be a non-empty [{'B, C, H, W' if dims == 4 else '..., H, W'}] tensor, got {tuple(x.shape)}")
    if x.shape[-1] % 2:
        raise FdnHipError(f"{what} has the odd width {x.shape[-1]}: the real FFT here takes even widths only, and nothing is cropped silently")
    return x.contiguous()


def _rfft2(x):
    """contiguous fp32 [..., H, W] -> interleaved complex fp32 [..., H, W/2 + 1, 2]"""
    H, W = x.shape[-2:]
    with torch.cuda.device(x.device):
        z = ops.rfft_rows(x)
        check(lib().fdn_fft_cols_c2c(ptr(z), ctypes.c_long(x.numel() // (H * W)), H, W // 2 + 1, stream()), "fdn_fft_cols_c2c")
    return z


def rfft2(x):
    """fp32 [..., H, W] on a ROCm device, W even -> complex64 [..., H, W/2 + 1]: torch.fft.rfft2(x) (norm='backward') through
    fdn_rfft_rows and fdn_fft_cols_c2c."""
    return torch.view_as_complex(_rfft2(_real(x, "x")))


def band_counts(H, W, bands=8):
    """-> list of bands + 1 ints: the Hermitian-weighted number of bins per band of an H x W image (they sum to H * W).  Host
    arithmetic, no GPU needed."""
    H, W = int(H), int(W)
    _size(H, W)
    out = (ctypes.c_long * (_bands(bands) + 1))()
    check(lib().fdn_spectrum_band_counts(H, W, bands, out), "fdn_spectrum_band_counts")
    return list(out)


def spectrum_pair_bands(za, zb, H, W, bands=8):
    """two spectra as _rfft2 / rfft2 give them (complex64 [..., H, Wf >= W/2 + 1], or float32 with a last axis of 2; Wf is the row pitch) ->
    float64 [planes, bands + 1, 5] (fdn_spectrum_pair_bands); za is the restored image's, zb the ground truth's."""
    _size(int(H), int(W))
    bands = _bands(bands)
    planes = []
    for z, what in ((za, "za"), (zb, "zb")):
        if isinstance(z, torch.Tensor) and z.dtype == torch.complex64:
            z = torch.view_as_real(z)
        if not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != torch.float32 or not z.is_contiguous():
            raise FdnHipError(f"{what} must be a contiguous complex64 (or float32 [..., 2]) ROCm tensor; Fourier evaluation has no CPU fallback")
        if z.dim() < 3 or z.shape[-1] != 2 or z.shape[-3] != H or z.shape[-2] < W // 2 + 1:
            raise FdnHipError(f"{what}: expected a spectrum [..., {H}, >= {W // 2 + 1}] of a {H}x{W} image, got {tuple(z.shape[:-1])}")
        planes.append(z)
    za, zb = planes
    if za.shape != zb.shape or za.device != zb.device:
        raise FdnHipError(f"the two spectra differ: {tuple(za.shape)} on {za.device}, {tuple(zb.shape)} on {zb.device}")
    n = za.numel() // (2 * H * za.shape[-2])
    nws = int(lib().fdn_spectrum_pair_bands_ws(ctypes.c_long(n), H, W, bands))
    if nws <= 0:
        raise FdnHipError(f"fdn_spectrum_pair_bands_ws refuses {n} planes of {H}x{W} with {bands} bands")
    ws = torch.empty(nws, dtype=torch.float64, device=za.device)
    out = torch.empty((n, bands + 1, TERMS), dtype=torch.float64, device=za.device)
    with torch.cuda.device(za.device):
        check(lib().fdn_spectrum_pair_bands(ptr(za), ptr(zb), ptr(out), ptr(ws), ctypes.c_long(n), H, W, ctypes.c_long(za.shape[-2]),
                                            bands, stream()), "fdn_spectrum_pair_bands")
    return out


def pair_bands(a, b, bands=8):
    """a (restored), b (ground truth): fp32 [B, C, H, W] on one ROCm device, W even -> float64 [B, C, bands + 1, 5]: per channel and
    band the sums over the band's bins, h the Hermitian weight (1 for kx = 0 and kx = W/2, else 2),
        0  sum h |Xa - Xb|^2    1  sum h (|Xa| - |Xb|)^2    2  sum h max(0, 2 (|Xa| |Xb| - Re(Xa conj(Xb))))    3  sum h |Xb|^2
        4  sum |dRe| + |dIm| over the half spectrum, unweighted (the numerator of FFTLoss)
    of the unscaled spectra; words 0 .. 3 divided by (H W)^2 are sums over the pixels.  Band 0 is the zero-frequency bin alone."""
    bands = _bands(bands)
    a, b = _real(a, "a", 4), _real(b, "b", 4)
    if a.shape != b.shape:
        raise FdnHipError(f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}.")
    if a.device != b.device:
        raise FdnHipError(f"the two images are on different devices ({a.device}, {b.device})")
    B, C, H, W = a.shape
    _size(H, W)
    return spectrum_pair_bands(_rfft2(a), _rfft2(b), H, W, bands).view(B, C, bands + 1, TERMS)


def _psnr(peak, mse):
    return float("inf") if mse == 0 else 10.0 * math.log10(peak * peak / mse)


def _ratio(x, y):
    return x / y if y != 0 else float("nan")


def metrics_from_sums(sums, H, W, peak=1.0):
    """The derived figures of ONE image from its band sums [C][bands + 1][5] (nested lists or an array; host arithmetic, float64):
      mse                            sum of word 0 over channels and bands / (C (H W)^2): the MSE of the image pair (Parseval)
      psnr                           10 log10(peak^2 / mse), inf for mse == 0
      amp_share, pha_share           A / (A + P), P / (A + P) with A, P the sums of words 1 and 2: the amplitude and the phase share of
                                     the MSE (A + P equals word 0's sum to rounding; the two shares add up to 1); nan for two equal images
      dc_share                       band 0's word 0 over the sum of word 0
      psnr_amp, psnr_pha             the PSNR if only that part of the error were there: from A / (C (H W)^2) and P / (C (H W)^2); inf when the part is 0
      fft_l1                         sum of word 4 / (C H (W/2 + 1) 2): the reference's FFTLoss(reduction='mean') of the pair
      bands                          per band a dict: share (the band's word 0 over the sum of word 0), amp_share and pha_share (the
                                     band's words 1 and 2 over A + P: they add up to the figures above) and rel_err (word 0 over word 3:
                                     the error relative to the ground truth's energy in the band; nan for a band without energy)"""
    s = np.asarray(sums, dtype=np.float64)
    C, nb1, _ = s.shape
    per = [[math.fsum(s[:, k, t].tolist()) for t in range(TERMS)] for k in range(nb1)]            # channels summed, per band
    tot, amp, pha = (math.fsum(p[t] for p in per) for t in range(3))
    n = float(C) * (float(H) * float(W)) ** 2
    out = {"mse": tot / n, "psnr": _psnr(peak, tot / n),
           "amp_share": _ratio(amp, amp + pha), "pha_share": _ratio(pha, amp + pha), "dc_share": _ratio(per[0][0], tot),
           "psnr_amp": _psnr(peak, amp / n), "psnr_pha": _psnr(peak, pha / n),
           "fft_l1": math.fsum(p[4] for p in per) / (C * H * (W // 2 + 1) * 2.0)}
    out["bands"] = [{"share": _ratio(p[0], tot), "amp_share": _ratio(p[1], amp + pha), "pha_share": _ratio(p[2], amp + pha),
                     "rel_err": _ratio(p[0], p[3])} for p in per]
    return out


def fourier_metrics(a, b, bands=8, peak=1.0):
    """a (restored), b (ground truth) as pair_bands takes them, values on a scale with the peak `peak` -> a list of B dicts, one per
    image with its channels summed (metrics_from_sums names the keys).  One device-to-host copy of B * C * (bands + 1) * 5 doubles."""
    H, W = a.shape[-2:] if isinstance(a, torch.Tensor) and a.dim() >= 2 else (0, 0)
    sums = pair_bands(a, b, bands).cpu().numpy()
    return [metrics_from_sums(s, H, W, peak) for s in sums]


def _u8_planes(img1, img2, bgr):
    """two uint8 image batches -> (planes of img1, planes of img2, single): fp32 [B, 3, h, w] RGB in [0, 1] through fdn_pre_u8, unpadded"""
    from .metrics import _u8_pair
    try:
        a, b, single = _u8_pair(img1, img2, 0)
    except FdnHipError as e:
        raise FdnHipError(str(e).replace("calculate_psnr_ssim_u8", "calculate_fourier")) from None
    B, h, w, _ = a.shape
    _size(h, w)
    out = []
    with torch.cuda.device(a.device):
        for t in (a, b):
            p = torch.empty((B, 3, h, w), device=t.device, dtype=torch.float32)
            check(lib().fdn_pre_u8(ptr(t), ptr(p), B, h, w, h, w, int(bool(bgr)), stream()), "fdn_pre_u8")
            out.append(p)
    return out[0], out[1], single


def calculate_fourier(img1, img2, bands=8, bgr=True):
    """The Fourier figures of 8-bit image pairs, taken as calculate_psnr_ssim_u8 takes them: (h,w,3) or (B,h,w,3) uint8 numpy arrays or
    tensors (host data is moved to the current ROCm device), img1 the restored image and img2 the ground truth, scaled to [0, 1] by
    fdn_pre_u8 without padding (so psnr is the PSNR of the 8-bit images).  bgr says whether the channels are B, G, R or R, G, B; the planes
    are R, G, B either way and the figures sum the channels, so it only decides which plane is which.  -> the dict of metrics_from_sums
    for one pair, a list of B dicts for a batch.  The width must be even."""
    bands = _bands(bands)
    a, b, single = _u8_planes(img1, img2, bgr)
    res = fourier_metrics(a, b, bands)
    return res[0] if single else res


def csv_header(bands):
    """the columns fourier_row fills, in order: the figures of the image, then per band share / amp / pha / rel_err"""
    cols = ["mse", "psnr", "amp_share", "pha_share", "dc_share", "psnr_amp", "psnr_pha", "fft_l1"]
    for k in range(bands + 1):
        cols += [f"band{k}_share", f"band{k}_amp", f"band{k}_pha", f"band{k}_rel_err"]
    return cols


def csv_row(m):
    """one dict of metrics_from_sums -> the values under csv_header, as repr strings"""
    vals = [m[k] for k in ("mse", "psnr", "amp_share", "pha_share", "dc_share", "psnr_amp", "psnr_pha", "fft_l1")]
    for bd in m["bands"]:
        vals += [bd["share"], bd["amp_share"], bd["pha_share"], bd["rel_err"]]
    return [repr(float(v)) for v in vals]
