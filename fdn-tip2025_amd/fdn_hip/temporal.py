"""The ratio across the frames of a video (include/fdn_temporal.h; no reference counterpart).

FDN's output brightness hangs on one scalar per frame, ratio_i: MAR multiplies its features by it and the result is the exponent of
1 - pow(1 - x, 40 i).  LPNet predicts it from one frame alone, so on noisy low-light footage it moves with the noise and the output
flickers.  RatioFilter keeps it steady: a causal exponential moving average per stream of frames, started afresh at a scene cut, which
is found by the distance between the luma histograms of neighbouring frames.  Histogram, cut decision and filter run on the GPU
(fdn_luma_hist, fdn_ratio_smooth), where the codec samples and LPNet's ratio already are: no host round trip between LPNet and FDN.
"""
import math
from fractions import Fraction

import torch

from . import lib, check, ptr, stream, FdnHipError

STATE_WORDS = 258        # FDN_TEMPORAL_STATE_WORDS: histogram of the last frame, bits of the last filtered ratio, flags


class RatioFilter:
    """The filter of ONE stream of h x w frames, taken in order.
    bits: 8 (uint8 samples) or 10 (int16 / uint16); alpha in (0, 1]: the weight of the new frame's ratio, ratio_hat = prev + alpha *
    (ratio - prev) - 1 filters nothing but still finds cuts; cut in [0, 1]: the fraction of pixels that have to change their luma bin
    between two frames for a scene cut (the histograms' L1 distance is at most 2 h w: cut_above = floor(cut * 2 h w)), 1 = never,
    apart from the first frame of the stream.  The state words and the scratch tensors live on `device`."""

    def __init__(self, h, w, bits, alpha, cut=0.3, device="cuda"):
        h, w, bits = int(h), int(w), int(bits)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"a 4:2:0 frame needs even, positive sides, got {h}x{w}")
        if h * w >= 1 << 30:
            raise ValueError(f"{h}x{w}: a frame of 2^30 pixels or more is not supported")
        if bits not in (8, 10):
            raise ValueError(f"bits {bits!r}: 8 or 10")
        alpha, cut = float(alpha), float(cut)
        if not 0.0 < alpha <= 1.0:
            raise ValueError(f"alpha {alpha!r}: a value in (0, 1]")
        if not 0.0 <= cut <= 1.0:
            raise ValueError(f"cut {cut!r}: a fraction in [0, 1]")
        self.h, self.w, self.bits, self.alpha, self.cut = h, w, bits, alpha, cut
        self.cut_above = math.floor(Fraction(cut) * (2 * h * w))      # exact: Fraction(cut) is the double's value
        self.device = torch.device(device)
        self.state = torch.zeros(STATE_WORDS, dtype=torch.int32, device=self.device)
        self._cuts = torch.zeros((), dtype=torch.int64, device=self.device)
        self._hist = self._dist = self._cut = None
        self.last_cut = self.last_dist = None

    def matches(self, h, w, bits):
        return (self.h, self.w, self.bits) == (int(h), int(w), int(bits))

    def reset(self):
        """forget the stream: the next frame is a first frame"""
        self.state.zero_()
        self._cuts.zero_()
        self.last_cut = self.last_dist = None

    def cuts_seen(self):
        """scene cuts since the last reset, the first frame included (synchronises)"""
        return int(self._cuts.item())

    def _frames(self, frames):
        ok = (torch.uint8,) if self.bits == 8 else (torch.int16, torch.uint16)
        if not isinstance(frames, torch.Tensor) or frames.dtype not in ok:
            raise FdnHipError(f"{self.bits}-bit frames must be {' or '.join(str(d) for d in ok)} tensors, got {getattr(frames, 'dtype', type(frames))}")
        if frames.dim() == 1:
            frames = frames.unsqueeze(0)
        n = self.h * self.w * 3 // 2
        if frames.dim() != 2 or frames.shape[1] != n or frames.shape[0] < 1:
            raise FdnHipError(f"expected frames [B, {n}] for {self.h}x{self.w}, got {tuple(frames.shape)}")
        if not frames.is_cuda or not frames.is_contiguous():
            raise FdnHipError("frames must be a contiguous ROCm tensor; the filter has no CPU fallback")
        return frames

    def step(self, frames, ratio):
        """frames [B, h*w*3/2] as preprocess_yuv420 takes them, ratio [B,1] fp32 of those frames -> the filtered ratio [B,1].  Two launches
        on the current stream, nothing synchronised; last_cut (int32) and last_dist (uint32 bits in an int32 tensor) are the device
        tensors [B] of this step."""
        frames = self._frames(frames)
        B = frames.shape[0]
        if not isinstance(ratio, torch.Tensor) or tuple(ratio.shape) != (B, 1) or ratio.dtype != torch.float32:
            raise FdnHipError(f"ratio must be a float32 tensor [B,1] for B = {B}, got {getattr(ratio, 'dtype', None)} {tuple(getattr(ratio, 'shape', ()))}")
        if not ratio.is_cuda or frames.device != self.state.device or ratio.device != self.state.device:
            raise FdnHipError(f"frames, ratio and the filter must live on one ROCm device ({frames.device}, {ratio.device}, {self.state.device})")
        ratio = ratio.contiguous()
        if self._hist is None or self._hist.shape[0] < B:
            self._hist = torch.empty((B, 256), dtype=torch.int32, device=self.device)
            self._dist = torch.empty(B, dtype=torch.int32, device=self.device)
            self._cut = torch.empty(B, dtype=torch.int32, device=self.device)
        out = torch.empty_like(ratio)
        check(lib().fdn_luma_hist(ptr(frames), ptr(self._hist), B, self.h, self.w, self.bits, stream()), "fdn_luma_hist")
        check(lib().fdn_ratio_smooth(ptr(self._hist), ptr(ratio), ptr(self.state), self.alpha, self.cut_above, B, ptr(out),
                                     ptr(self._dist), ptr(self._cut), stream()), "fdn_ratio_smooth")
        self.last_cut, self.last_dist = self._cut[:B], self._dist[:B]
        self._cuts += self.last_cut.sum()
        return out
