"""Video evaluation straight from codec samples (include/fdn_vmetrics.h): an enhanced stream of Y'CbCr 4:2:0 frames scored against a
ground-truth stream on the GPU, never through 8-bit RGB, so what the video route rounded once is judged as it was written and 10 bit
stays 10 bit.  Per frame: PSNR of Y, Cb and Cr, SSIM on luma (the reference's _ssim_cly, basicsr/metrics/psnr_ssim.py:202-240, on the
luma codes), mean luma, scene cuts (fdn_hip.temporal.RatioFilter's rule) and the change of mean luma between neighbouring frames of a
scene, whose mean magnitude is the brightness-flicker figure the ratio filter exists to bring down.

PSNR is taken on the codes with the peak 2^bits - 1, whatever the range flag of the stream says (a limited-range stream never reaches
its peak): the convention of every video tool, ffmpeg's psnr filter among them.  mean_y and dmean are in 8-bit code units for every bit
depth (10-bit codes / 4), so figures of an 8-bit and a 10-bit version of one stream compare.

pair_stats and ssim_y enqueue on the current stream and synchronise nothing.  No CPU fallback; the functions that take Python ints
(psnr_from_sse, psnr_avg, cut_above, hist_distance, dmean, mean_abs) and VideoScore.add_host are plain host arithmetic."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import torch

from . import FdnHipError, check, lib, stream
from .harness import _yuv_frames, _yuv_ptr
from .metrics import ssim3d_taps

RECORD_KEYS = ("psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y", "mean_y_ref", "cut", "dmean", "dmean_ref")
_NAN = float("nan")
_TAPS = np.ascontiguousarray(ssim3d_taps(), dtype=np.float64)        # the host array fdn_yuv420_ssim_y reads its window from


def _pair(a, b, h, w, fmt):
    a = _yuv_frames(a, h, w, fmt)
    if b is not None:
        b = _yuv_frames(b, h, w, fmt)
        if b.shape != a.shape or b.device != a.device:
            raise FdnHipError(f"the two streams differ: {tuple(a.shape)} on {a.device}, {tuple(b.shape)} on {b.device}")
    return a, b


def pair_stats(a, b, h, w, fmt):
    """frames a, b [B, h*w*3/2] as preprocess_yuv420 takes them (uint8, or int16 / uint16 for 10 bit), fmt their VideoFormat -> int64
    [B,5] = SSE_Y, SSE_Cb, SSE_Cr, the sum of a's luma codes, the sum of b's; exact integers.  b=None: only word 3, the others are 0."""
    a, b = _pair(a, b, h, w, fmt)
    B = a.shape[0]
    pa, pb = _yuv_ptr(a, "frames"), (None if b is None else _yuv_ptr(b, "frames"))
    out = torch.empty((B, 5), dtype=torch.int64, device=a.device)
    check(lib().fdn_yuv420_pair_stats(pa, pb, ctypes.c_void_p(out.data_ptr()), B, h, w, fmt.layout, fmt.bits, stream()), "fdn_yuv420_pair_stats")
    return out


def ssim_y(a, b, h, w, fmt):
    """frames a, b as pair_stats takes them -> float64 [B]: the mean of the SSIM map of the two luma planes (11 x 11 Gaussian, replicate
    border, no crop, C1 / C2 for L = 2^bits - 1), float64 throughout; the same bits for a frame wherever it sits in a batch."""
    a, b = _pair(a, b, h, w, fmt)
    if b is None:
        raise FdnHipError("ssim_y needs two streams")
    B = a.shape[0]
    pa, pb = _yuv_ptr(a, "frames"), _yuv_ptr(b, "frames")
    n = int(lib().fdn_yuv420_ssim_y_ws(B, h, w))
    if n <= 0:
        raise FdnHipError(f"fdn_yuv420_ssim_y_ws refuses B = {B}, {h}x{w}")
    ws = torch.empty(n, dtype=torch.float64, device=a.device)
    out = torch.empty(B, dtype=torch.float64, device=a.device)
    check(lib().fdn_yuv420_ssim_y(pa, pb, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(_TAPS.ctypes.data),
                                  B, h, w, fmt.bits, stream()), "fdn_yuv420_ssim_y")
    return out


# ---- host arithmetic on Python ints ---------------------------------------------------------------------------------------------------
def psnr_from_sse(sse, n, bits):
    """10 log10(L^2 n / sse) for a sum of squared code differences over n samples, L = 2^bits - 1; inf for sse == 0"""
    sse, n = int(sse), int(n)
    if sse == 0:
        return float("inf")
    peak = (1 << bits) - 1
    return 10.0 * math.log10(peak * peak * n / sse)


def psnr_avg(sse_y, sse_u, sse_v, h, w, bits):
    """the three planes pooled over the h*w*3/2 samples of a 4:2:0 frame: the `average` of ffmpeg's psnr filter"""
    return psnr_from_sse(int(sse_y) + int(sse_u) + int(sse_v), h * w * 3 // 2, bits)


def cut_above(cut, h, w):
    """floor(cut * 2 h w), exactly (Fraction(cut) is the double's value): RatioFilter's threshold on the histograms' L1 distance"""
    return math.floor(Fraction(float(cut)) * (2 * h * w))


def hist_distance(hist, prev):
    """sum |hist - prev| of two 256-bin histograms, in integers"""
    return int(sum(abs(int(x) - int(y)) for x, y in zip(hist, prev)))


def dmean(s, s_prev, h, w, bits):
    """(S(t) - S(t-1)) / (h w 2^(bits-8)): the change of mean luma in 8-bit code units, formed exactly and rounded to float64 once"""
    return float(Fraction(int(s) - int(s_prev), h * w * (1 << (bits - 8))))


def mean_luma(s, h, w, bits):
    """S / (h w 2^(bits-8)): mean luma in 8-bit code units, rounded to float64 once"""
    return float(Fraction(int(s), h * w * (1 << (bits - 8))))


def mean_abs(values):
    """mean |v| of the values that are not None; nan when there is none"""
    v = [abs(x) for x in values if x is not None]
    return math.fsum(v) / len(v) if v else _NAN


def _mean(values):
    v = [x for x in values if x is not None]
    return math.fsum(v) / len(v) if v else _NAN


class VideoScore:
    """The score of ONE stream of h x w frames of VideoFormat fmt, taken in order, with or without a ground-truth stream.
    update(dist, ref=None) takes a batch of frames (the same ref= choice on every call) and appends one record per frame to .frames:
      psnr_y / psnr_u / psnr_v / psnr_avg, ssim_y   against ref (None without one); PSNR on the codes, peak 2^bits - 1;
      mean_y, mean_y_ref                            mean luma of dist and of ref, in 8-bit code units;
      cut                                           True for the first frame and where sum |H_t - H_(t-1)| > cut_above(cut, h, w), H the
                                                    256-bin luma histogram of ref when there is one (a flickering output must not define
                                                    the scenes), else of dist: RatioFilter's rule on the integer histograms;
      dmean, dmean_ref                              the change of mean luma against the frame before, None at a cut.
    .stats holds the five integers of pair_stats per frame.  The frame before - luma sums and histogram - is carried across batches, so
    N frames in batches of 1, 3 or N give equal records.  summary() pools the stream.  device: where the frames of this stream live;
    update() refuses frames from elsewhere ("cuda" takes any ROCm device), the launches run where the frames are."""

    def __init__(self, h, w, fmt, cut=0.3, device="cuda"):
        h, w = int(h), int(w)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"a 4:2:0 frame needs even, positive sides, got {h}x{w}")
        if h * w >= 1 << 30:
            raise ValueError(f"{h}x{w}: a frame of 2^30 pixels or more is not supported")
        cut = float(cut)
        if not 0.0 <= cut <= 1.0:
            raise ValueError(f"cut {cut!r}: a fraction in [0, 1]")
        self.h, self.w, self.fmt, self.bits, self.cut = h, w, fmt, fmt.bits, cut
        self.cut_above = cut_above(cut, h, w)
        self.device = torch.device(device)
        self.frames, self.stats = [], []
        self.has_ref = None
        self._prev = None                                      # (sum of dist's luma, sum of ref's luma or None, histogram) of the last frame

    def update(self, dist, ref=None):
        """one batch, on the current stream; the few words per frame come back in one copy (which synchronises)"""
        dist, ref = _pair(dist, ref, self.h, self.w, self.fmt)
        if self.has_ref is not None and self.has_ref != (ref is not None):
            raise ValueError("a stream is scored with a reference on every call or on none")
        if not dist.is_cuda:
            raise FdnHipError("frames must be a contiguous ROCm tensor; video evaluation has no CPU fallback")
        if dist.device.type != self.device.type or (self.device.index is not None and dist.device.index != self.device.index):
            raise FdnHipError(f"this score was made for frames on {self.device}, these are on {dist.device}")
        B = dist.shape[0]
        stats = pair_stats(dist, ref, self.h, self.w, self.fmt)
        hist = torch.empty((B, 256), dtype=torch.int32, device=dist.device)
        check(lib().fdn_luma_hist(_yuv_ptr(dist if ref is None else ref, "frames"), ctypes.c_void_p(hist.data_ptr()), B, self.h, self.w,
                                  self.bits, stream()), "fdn_luma_hist")
        cols = [stats, hist.to(torch.int64)]                   # a bin holds at most h w < 2^30: no sign to mind
        if ref is not None:
            cols.append(ssim_y(dist, ref, self.h, self.w, self.fmt).view(torch.int64).unsqueeze(1))
        words = torch.cat(cols, dim=1).cpu().numpy()
        ssim = words[:, 261].copy().view(np.float64).tolist() if ref is not None else None
        self.add_host(words[:, :5].tolist(), words[:, 5:261].tolist(), ssim)
        return self.frames[-B:]

    def add_host(self, stats, hists, ssim=None):
        """the host half of update(): per frame the five integers of pair_stats, the 256 bins of the luma histogram that defines the
        scenes, and the SSIM (None: no reference, words 0 .. 2 and 4 of stats are ignored)"""
        has_ref = ssim is not None
        if self.has_ref is not None and self.has_ref != has_ref:
            raise ValueError("a stream is scored with a reference on every call or on none")
        self.has_ref = has_ref
        h, w, bits = self.h, self.w, self.bits
        for t, (st, hist) in enumerate(zip(stats, hists)):
            st = tuple(int(v) for v in st)
            hist = [int(v) for v in hist]
            s_dist, s_ref = st[3], (st[4] if has_ref else None)
            is_cut = self._prev is None or hist_distance(hist, self._prev[2]) > self.cut_above
            rec = dict.fromkeys(RECORD_KEYS)
            if has_ref:
                rec["psnr_y"] = psnr_from_sse(st[0], h * w, bits)
                rec["psnr_u"] = psnr_from_sse(st[1], h * w // 4, bits)
                rec["psnr_v"] = psnr_from_sse(st[2], h * w // 4, bits)
                rec["psnr_avg"] = psnr_avg(st[0], st[1], st[2], h, w, bits)
                rec["ssim_y"] = float(ssim[t])
                rec["mean_y_ref"] = mean_luma(s_ref, h, w, bits)
            rec["mean_y"] = mean_luma(s_dist, h, w, bits)
            rec["cut"] = bool(is_cut)
            if not is_cut:
                rec["dmean"] = dmean(s_dist, self._prev[0], h, w, bits)
                if has_ref:
                    rec["dmean_ref"] = dmean(s_ref, self._prev[1], h, w, bits)
            self._prev = (s_dist, s_ref, hist)
            self.frames.append(rec)
            self.stats.append(st)

    def summary(self):
        """-> dict: `frames`, `cuts`, the mean of every per-frame column, psnr_{y,u,v,avg}_global from the squared errors totalled over
        the stream, flicker = mean |dmean| over the frames that are no cut and, with a reference, flicker_ref and flicker_err = mean
        |dmean - dmean_ref|.  A figure with nothing to average is nan."""
        f, n = self.frames, len(self.frames)
        h, w, bits = self.h, self.w, self.bits
        out = {"frames": n, "cuts": sum(1 for r in f if r["cut"])}
        for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y", "mean_y_ref"):
            out[k] = _mean([r[k] for r in f])
        if self.has_ref and n:
            sy, su, sv = (sum(st[i] for st in self.stats) for i in range(3))
            out["psnr_y_global"] = psnr_from_sse(sy, n * h * w, bits)
            out["psnr_u_global"] = psnr_from_sse(su, n * (h * w // 4), bits)
            out["psnr_v_global"] = psnr_from_sse(sv, n * (h * w // 4), bits)
            out["psnr_avg_global"] = psnr_from_sse(sy + su + sv, n * (h * w * 3 // 2), bits)
        else:
            out.update(dict.fromkeys(("psnr_y_global", "psnr_u_global", "psnr_v_global", "psnr_avg_global"), _NAN))
        out["flicker"] = mean_abs([r["dmean"] for r in f])
        out["flicker_ref"] = mean_abs([r["dmean_ref"] for r in f])
        out["flicker_err"] = mean_abs([r["dmean"] - r["dmean_ref"] for r in f if r["dmean"] is not None and r["dmean_ref"] is not None])
        return out
