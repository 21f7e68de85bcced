"""Motion-compensated temporal denoising of an enhanced video stream (include/fdn_mctf.h, libfdn_mctf.so).

Low-light enhancement multiplies sensor noise by the ratio, and a network run frame by frame lands a little differently on every frame:
the output boils.  temporal.RatioFilter steadies the one global ratio and motion.MotionScore measures what remains; this filters it.  A
recursive temporal filter on the enhanced fp32 R'G'B' frames, before the one rounding to codec samples: the previous FILTERED frame is
moved along the block vectors motion.search finds between the unfiltered frames (as codec samples), overlapped between the four nearest
blocks so that the 16 x 16 grid does not show, and blended in with a weight k per pixel that falls to 0 where the prediction does not fit
(k = strength * max(1 - (D / threshold)^2, 0), D the 3 x 3 mean of the largest channel difference) and is 0 everywhere at a scene cut.

    blend(cur, prev, mv, stats, h, w, strength, threshold, cut_limit, kmap=False) -> out [B,3,h,w]  (, kmap [B,h,w])
    TemporalDenoiser(h, w, fmt, strength=0.6, threshold=0.12, radius=8, cut=0.10)   the filter of one stream, fed batch by batch

blend enqueues B launches on the current stream and synchronises nothing.  Every operation is ordered and rounded once in fp32, so a
float32 numpy restatement equals the device bit for bit.  No CPU fallback."""
import ctypes
import math
import os
import struct
from fractions import Fraction

import torch

from . import FdnHipError, _declare, check, ptr, stream
from . import motion
from ._abi_mctf import PROTOTYPES, VERSION    # generated from include/fdn_mctf.h by tools/gen_abi_table.py
from .harness import postprocess_yuv420

ABI_VERSION = VERSION[1]

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_mctf.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_mctf.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has mctf ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def check_strength(strength):
    """-> float in [0, 1]; anything else raises ValueError"""
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= strength <= 1.0:
        raise ValueError(f"denoise strength {strength!r}: a number in [0, 1]")
    return float(strength)


def inv_threshold(threshold):
    """the float32 the kernel multiplies D by: 1 / threshold formed in double and rounded to float32 once; ValueError unless threshold is a
    positive finite number whose reciprocal is a finite, positive float32"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 < threshold < math.inf:
        raise ValueError(f"denoise threshold {threshold!r}: a positive, finite number")
    try:
        inv = struct.unpack("f", struct.pack("f", 1.0 / float(threshold)))[0]
    except OverflowError:
        inv = math.inf
    if not 0.0 < inv < math.inf:
        raise ValueError(f"denoise threshold {threshold!r}: its reciprocal is no positive, finite float32")
    return inv


def cut_limit(cut, h, w, bits):
    """floor(cut * (2^bits - 1) * h * w): the sum of the chosen SADs (in codes) above which a frame counts as a scene cut; exact, Fraction(cut)
    being the double's value"""
    cut = float(cut)
    if not 0.0 <= cut <= 1.0:
        raise ValueError(f"denoise cut {cut!r}: a fraction in [0, 1]")
    return math.floor(Fraction(cut) * ((2 ** int(bits) - 1) * int(h) * int(w)))


def _f32(t, shape, what, like=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise FdnHipError(f"{what} must be a float32 tensor {list(shape)}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if not t.is_cuda or not t.is_contiguous() or (like is not None and t.device != like.device):
        raise FdnHipError(f"{what} must be a contiguous ROCm tensor" + ("" if like is None else f" on {like.device}") +
                          "; the temporal denoiser has no CPU fallback")
    return t


def blend(cur, prev, mv, stats, h, w, strength, threshold, cut_limit, kmap=False):
    """cur: fp32 [B,3,H,W], the forward's result, of which the top-left h x w is read; prev: fp32 [3,h,w], the FILTERED frame before frame 0,
    or None; mv int16 [B,nby,nbx,2] and stats int64 [B,4] as motion.search returns them (of stats only word 0 is read) -> out fp32
    [B,3,h,w], frame i filtered against out[i-1] and frame 0 against prev; with kmap=True (out, k fp32 [B,h,w]).  A frame without a
    predecessor, or with stats[i,0] > cut_limit, is clamp01(cur) with k = 0.  threshold reaches the kernel as inv_threshold(threshold)."""
    strength, inv, cut_limit = check_strength(strength), inv_threshold(threshold), int(cut_limit)
    if cut_limit < 0:
        raise ValueError(f"cut_limit {cut_limit}: not negative")
    h, w = int(h), int(w)
    if not isinstance(cur, torch.Tensor) or cur.dim() != 4 or cur.shape[1] != 3 or h < 1 or w < 1 or h > cur.shape[2] or w > cur.shape[3]:
        raise FdnHipError(f"cannot filter {h}x{w} out of {tuple(getattr(cur, 'shape', ()))}: cur is [B,3,H,W] with H >= h, W >= w")
    if h * w >= 1 << 30:
        raise FdnHipError(f"{h}x{w}: a frame of 2^30 pixels or more is not supported")
    B, _, H, W = cur.shape
    cur = _f32(cur, cur.shape, "cur")
    if prev is not None:
        prev = _f32(prev, (3, h, w), "prev", like=cur)
    nby, nbx = motion.block_grid(h, w)
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or tuple(mv.shape) != (B, nby, nbx, 2) or mv.device != cur.device \
            or not mv.is_contiguous():
        raise FdnHipError(f"mv must be a contiguous int16 [{B},{nby},{nbx},2] beside cur, got {getattr(mv, 'dtype', type(mv))} "
                          f"{tuple(getattr(mv, 'shape', ()))}")
    if not isinstance(stats, torch.Tensor) or stats.dtype != torch.int64 or tuple(stats.shape) != (B, 4) or stats.device != cur.device \
            or not stats.is_contiguous():
        raise FdnHipError(f"stats must be a contiguous int64 [{B},4] beside cur, got {getattr(stats, 'dtype', type(stats))} "
                          f"{tuple(getattr(stats, 'shape', ()))}")
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device=cur.device)
    k = torch.empty((B, h, w), dtype=torch.float32, device=cur.device) if kmap else None
    with torch.cuda.device(cur.device):
        check(lib().fdn_mctf_blend(ptr(cur), ptr(prev), ptr(mv), ptr(stats), ptr(out), ptr(k), B, h, w, H, W, strength, inv, cut_limit, stream()),
              "fdn_mctf_blend")
    return (out, k) if kmap else out


class TemporalDenoiser:
    """The temporal filter of ONE stream of h x w frames of VideoFormat fmt, taken in order.
    step(res) takes the forward's fp32 result [B,3,H,W] (H >= h, W >= w) and returns the filtered frames fp32 [B,3,h,w], which then go to
    postprocess_yuv420 in place of res.  Across calls it keeps, on the device, the last UNFILTERED frame as 4:2:0 samples - the guide of the
    block search: vectors are found between the frames as they came out of the network, so the filter's own smoothing never feeds the
    search - and the last FILTERED fp32 frame, the predecessor of the recursion.  N frames in batches of 1, 3 or N give equal bits.
      strength   in [0, 1]: the weight of the motion-compensated predecessor where it fits perfectly (0 only clamps);
      threshold  > 0, in units of the [0, 1] signal: the 3 x 3 mean of the largest channel difference at which the weight reaches 0;
      radius     0 .. 16: the search radius of motion.search;
      cut        in [0, 1]: a frame whose chosen block SADs sum to more than cut * (2^bits - 1) * h * w codes - a mean absolute luma error
                 of the best match above `cut` of the range - starts afresh, unfiltered: a scene cut.  1 = never.
    The defaults come from a numpy prototype of the definition on synthetic noise (a smooth random texture, still or moving, iid Gaussian
    noise of sigma 0.02 and 0.05; DESIGN.md has the figures); they are NOT tuned on footage.  The first frame of a stream, and the first
    after reset(), is returned clamped and unfiltered."""

    def __init__(self, h, w, fmt, strength=0.6, threshold=0.12, radius=8, cut=0.10, device="cuda"):
        h, w = int(h), int(w)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"a 4:2:0 frame needs even, positive sides, got {h}x{w}")
        if h * w >= 1 << 30:
            raise ValueError(f"{h}x{w}: a frame of 2^30 pixels or more is not supported")
        self.h, self.w, self.fmt, self.bits = h, w, fmt, fmt.bits
        self.strength, self.threshold, self.radius, self.cut = check_strength(strength), threshold, motion.check_radius(radius), float(cut)
        inv_threshold(threshold)
        self.cut_limit = cut_limit(cut, h, w, fmt.bits)
        self.device = torch.device(device)
        self._guide = self._prev = None                        # [1, n] samples of the last unfiltered frame; fp32 [3,h,w] of the last filtered one

    def matches(self, h, w, bits):
        return (self.h, self.w, self.bits) == (int(h), int(w), int(bits))

    def reset(self):
        """forget the stream: the next frame is a first frame"""
        self._guide = self._prev = None

    def step(self, res):
        """res fp32 [B,3,H,W] on the filter's device -> fp32 [B,3,h,w].  One postprocess_yuv420, one batched motion.search and B blend launches
        on the current stream, nothing synchronised."""
        if not isinstance(res, torch.Tensor) or not res.is_cuda:
            raise FdnHipError("res must be a contiguous float32 ROCm tensor [B,3,H,W]; the temporal denoiser has no CPU fallback")
        if res.device.type != self.device.type or (self.device.index is not None and res.device.index != self.device.index):
            raise FdnHipError(f"this denoiser was made for frames on {self.device}, these are on {res.device}")
        guide = postprocess_yuv420(res, self.h, self.w, self.fmt)
        mv, _, stats = motion.search(guide, self._guide, self.h, self.w, self.fmt, self.radius)
        out = blend(res, self._prev, mv, stats, self.h, self.w, self.strength, self.threshold, self.cut_limit)
        self._guide, self._prev = guide[-1:].clone(), out[-1].clone()
        return out
