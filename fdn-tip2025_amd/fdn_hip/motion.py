"""Motion-compensated temporal consistency of a video stream (include/fdn_motion.h, libfdn_motion.so).

video_metrics' one temporal figure, flicker, is the change of a frame's mean luma: it sees a global brightness pump and nothing local.
Enhanced low-light video fails locally - boiling amplified noise, tone shifts that come and go, deblurring that lands differently from
frame to frame - and a plain frame difference charges camera and object motion to the method.  Here the motion is taken from a guide
stream by full-search block matching on luma (16 x 16 blocks, +-radius, exact integers), and the change of the scored stream from frame
to frame is measured along those vectors.

    block_grid(h, w)                                               -> (nby, nbx)
    search(guide, prev, h, w, fmt, radius=8)                       -> (mv int16 [B,nby,nbx,2], sad int32 [B,nby,nbx,2], stats int64 [B,4])
    residual(frames, frames_prev, guide, guide_prev, mv, h, w, fmt) -> int64 [B,5]
    MotionScore(h, w, fmt, radius=8)                               the score of one stream, fed batch by batch

search and residual enqueue on the current stream and synchronise nothing.  Every figure is an exact integer, so a numpy restatement
equals the device.  No CPU fallback; MotionScore.add_host and summary are plain host arithmetic on Python ints."""
import ctypes
import math
import os
from fractions import Fraction

import torch

from . import FdnHipError, _declare, check, stream
from ._abi_motion import PROTOTYPES, VERSION    # generated from include/fdn_motion.h by tools/gen_abi_table.py
from .harness import _yuv_frames, _yuv_ptr
from .video_metrics import psnr_from_sse

ABI_VERSION = VERSION[1]
BLOCK, MAX_RADIUS = 16, 16                                # FDN_MOTION_BLOCK, FDN_MOTION_MAX_RADIUS of include/fdn_motion.h
RECORD_KEYS = ("mc_psnr", "mc_psnr_ref", "tc_rmse", "moving", "mean_mv")
_NAN = float("nan")

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_motion.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_motion.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has motion ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def check_radius(radius):
    """-> int in 0 .. 16; anything else raises ValueError"""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"motion radius {radius!r}: an integer in 0 .. {MAX_RADIUS}")
    return radius


def block_grid(h, w):
    """-> (nby, nbx): the 16 x 16 blocks of an h x w luma plane, cut from the top-left corner; the last of a row or column may be partial"""
    return -(-int(h) // BLOCK), -(-int(w) // BLOCK)


def _frames(x, h, w, fmt, what, like=None, one=False):
    """a batch of frames (or, one=True, the one frame before a batch) -> tensor [B, n]; dtype and shape are judged before where it lives"""
    x = _yuv_frames(x, h, w, fmt)
    if one and x.shape[0] != 1:
        raise FdnHipError(f"{what} is the ONE frame before the batch, got {x.shape[0]}")
    if like is not None and (x.device != like.device or (not one and x.shape != like.shape)):
        raise FdnHipError(f"{what} differs from the batch: {tuple(x.shape)} on {x.device}, {tuple(like.shape)} on {like.device}")
    return x


def search(guide, prev, h, w, fmt, radius=8):
    """guide: frames [B, h*w*3/2] as preprocess_yuv420 takes them; prev: the one frame before them, or None -> (mv int16 [B,nby,nbx,2] =
    (dy, dx) of every block against the frame before, sad int32 [B,nby,nbx,2] = (SAD of that vector, SAD of the zero vector), stats int64
    [B,4] = the sum of each, the sum of |dy| + |dx| and the count of blocks with a non-zero vector).  A block at p matches p + (dy, dx) in
    the frame before: content that moved by +s gives -s.  prev=None: frame 0's rows are 0."""
    radius = check_radius(radius)
    guide = _frames(guide, h, w, fmt, "guide")
    prev = None if prev is None else _frames(prev, h, w, fmt, "prev", like=guide, one=True)
    pg, pp = _yuv_ptr(guide, "guide"), (None if prev is None else _yuv_ptr(prev, "prev"))
    B = guide.shape[0]
    nby, nbx = block_grid(h, w)
    mv = torch.empty((B, nby, nbx, 2), dtype=torch.int16, device=guide.device)
    sad = torch.empty((B, nby, nbx, 2), dtype=torch.int32, device=guide.device)
    stats = torch.empty((B, 4), dtype=torch.int64, device=guide.device)
    with torch.cuda.device(guide.device):
        check(lib().fdn_motion_search(pg, pp, ctypes.c_void_p(mv.data_ptr()), ctypes.c_void_p(sad.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                                      B, h, w, fmt.bits, radius, stream()), "fdn_motion_search")
    return mv, sad, stats


def residual(frames, frames_prev, guide, guide_prev, mv, h, w, fmt):
    """frames and guide [B, h*w*3/2], the one frame before each (both or neither None), mv int16 [B,nby,nbx,2] from search -> int64 [B,5] =
    sum |rD|, sum rD^2, sum |rG|, sum rG^2, sum (rD - rG)^2 over the luma plane, rD(p) = frames_t(p) - frames_(t-1)(clamp(p + mv(p))) and rG
    the same on the guide.  guide may be frames itself.  Both prevs None: frame 0's row is 0."""
    frames = _frames(frames, h, w, fmt, "frames")
    guide = _frames(guide, h, w, fmt, "guide", like=frames)
    if (frames_prev is None) != (guide_prev is None):
        raise FdnHipError("residual needs the frame before both streams or before neither")
    if frames_prev is not None:
        frames_prev = _frames(frames_prev, h, w, fmt, "frames_prev", like=frames, one=True)
        guide_prev = _frames(guide_prev, h, w, fmt, "guide_prev", like=frames, one=True)
    B = frames.shape[0]
    if not isinstance(mv, torch.Tensor) or mv.dtype != torch.int16 or tuple(mv.shape) != (B, *block_grid(h, w), 2) or mv.device != frames.device \
            or not mv.is_contiguous():
        raise FdnHipError(f"mv must be a contiguous int16 [{B},{block_grid(h, w)[0]},{block_grid(h, w)[1]},2] beside the frames, got "
                          f"{getattr(mv, 'dtype', type(mv))} {tuple(getattr(mv, 'shape', ()))}")
    pf, pg = _yuv_ptr(frames, "frames"), _yuv_ptr(guide, "guide")
    pfp, pgp = (None, None) if frames_prev is None else (_yuv_ptr(frames_prev, "frames_prev"), _yuv_ptr(guide_prev, "guide_prev"))
    stats = torch.empty((B, 5), dtype=torch.int64, device=frames.device)
    with torch.cuda.device(frames.device):
        check(lib().fdn_motion_residual(pf, pfp, pg, pgp, ctypes.c_void_p(mv.data_ptr()), ctypes.c_void_p(stats.data_ptr()), B, h, w, fmt.bits,
                                        stream()), "fdn_motion_residual")
    return stats


# ---- host arithmetic on Python ints ---------------------------------------------------------------------------------------------------
def tc_rmse(sq, n, bits):
    """sqrt(sq / n) / 2^(bits-8): the quotient sq / (n 4^(bits-8)) formed exactly and rounded to float64 once, then the root"""
    return math.sqrt(float(Fraction(int(sq), int(n) * 4 ** (bits - 8))))


def _mean(values):
    v = [x for x in values if x is not None]
    return math.fsum(v) / len(v) if v else _NAN


class MotionScore:
    """The temporal consistency of ONE stream of h x w frames of VideoFormat fmt, taken in order, beside video_metrics.VideoScore.
    update(dist, ref=None, cuts=None) takes a batch (the same ref= choice on every call) and appends one record per frame to .frames:
      mc_psnr       10 log10(L^2 h w / sum rD^2), L = 2^bits - 1, inf at 0: how well the previous OUTPUT frame, moved by the motion,
                    predicts this one;
      mc_psnr_ref   the same from sum rG^2, on the guide itself: the ceiling that occlusion and real change leave;
      tc_rmse       sqrt(sum (rD - rG)^2 / (h w)) / 2^(bits-8): the RMS difference of the compensated temporal change against the truth's,
                    in 8-bit code units - the local counterpart of video_metrics' flicker_err;
      moving        the share of blocks with a non-zero vector;      mean_mv   the mean |dy| + |dx| per block.
    The motion comes from the guide: ref when given.  Without ref the stream compensates itself: the search then tracks the stream's own
    noise and artefacts as if they were motion, so mc_psnr is flattered, a fault that moves with the content is invisible, and there is no
    truth to hold the change against - mc_psnr_ref and tc_rmse are None.
    cuts[i] is True where frame i of the batch starts a scene (VideoScore's `cut` flags); cuts=None: only the stream's first frame is one.
    At a cut - and at the stream's first frame whatever cuts says - every figure is None.  .stats holds the nine integers per frame (four
    of the search, five of the residual).  The last frame of dist and of the guide stays on the device across calls, so N frames in batches
    of 1, 3 or N give equal records.  summary() pools the stream."""

    def __init__(self, h, w, fmt, radius=8, device="cuda"):
        h, w = int(h), int(w)
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"a 4:2:0 frame needs even, positive sides, got {h}x{w}")
        if h * w >= 1 << 30:
            raise ValueError(f"{h}x{w}: a frame of 2^30 pixels or more is not supported")
        self.h, self.w, self.fmt, self.bits, self.radius = h, w, fmt, fmt.bits, check_radius(radius)
        self.blocks = block_grid(h, w)[0] * block_grid(h, w)[1]
        self.device = torch.device(device)
        self.frames, self.stats = [], []
        self.has_ref = None
        self._prev = None                                      # (last frame of dist, last frame of the guide), each [1, n] on the device

    def update(self, dist, ref=None, cuts=None):
        """one batch, on the current stream; the nine words per frame come back in one copy (which synchronises)"""
        dist = _yuv_frames(dist, self.h, self.w, self.fmt)
        if self.has_ref is not None and self.has_ref != (ref is not None):
            raise ValueError("a stream is scored with a reference on every call or on none")
        if not dist.is_cuda:
            raise FdnHipError("frames must be a contiguous ROCm tensor; motion compensation has no CPU fallback")
        if dist.device.type != self.device.type or (self.device.index is not None and dist.device.index != self.device.index):
            raise FdnHipError(f"this score was made for frames on {self.device}, these are on {dist.device}")
        guide = dist if ref is None else _frames(ref, self.h, self.w, self.fmt, "ref", like=dist)
        B = dist.shape[0]
        if cuts is not None and len(cuts) != B:
            raise ValueError(f"{len(cuts)} cut flags for {B} frames")
        prev_d, prev_g = self._prev if self._prev is not None else (None, None)
        mv, _, s_stats = search(guide, prev_g, self.h, self.w, self.fmt, self.radius)
        r_stats = residual(dist, prev_d, guide, prev_g, mv, self.h, self.w, self.fmt)
        words = torch.cat([s_stats, r_stats], dim=1).cpu().tolist()
        last = dist[-1:].clone()
        self._prev = (last, last if ref is None else guide[-1:].clone())
        self.add_host([x[:4] for x in words], [x[4:] for x in words], cuts, has_ref=ref is not None)
        return self.frames[-B:]

    def add_host(self, search_stats, residual_stats, cuts=None, has_ref=True):
        """the host half of update(): per frame the four integers of search and the five of residual, and the cut flags"""
        if self.has_ref is not None and self.has_ref != has_ref:
            raise ValueError("a stream is scored with a reference on every call or on none")
        self.has_ref = has_ref
        n, bits = self.h * self.w, self.bits
        for t, (s, r) in enumerate(zip(search_stats, residual_stats)):
            s, r = tuple(int(v) for v in s), tuple(int(v) for v in r)
            is_cut = not self.frames or (cuts is not None and bool(cuts[t]))
            rec = dict.fromkeys(RECORD_KEYS)
            if not is_cut:
                rec["mc_psnr"] = psnr_from_sse(r[1], n, bits)
                rec["moving"] = float(Fraction(s[3], self.blocks))
                rec["mean_mv"] = float(Fraction(s[2], self.blocks))
                if has_ref:
                    rec["mc_psnr_ref"] = psnr_from_sse(r[3], n, bits)
                    rec["tc_rmse"] = tc_rmse(r[4], n, bits)
            self.frames.append(rec)
            self.stats.append(s + r)

    def summary(self):
        """-> dict: `frames`, `cuts` (frames without figures), the mean of every per-frame column over the others, and mc_psnr_global,
        mc_psnr_ref_global, tc_rmse_global from the integers totalled over those frames.  A figure with nothing to average is nan."""
        f, n, bits = self.frames, self.h * self.w, self.bits
        live = [t for t, r in enumerate(f) if r["mc_psnr"] is not None]
        out = {"frames": len(f), "cuts": len(f) - len(live)}
        for k in RECORD_KEYS:
            out[k] = _mean([f[t][k] for t in live])
        out.update(dict.fromkeys(("mc_psnr_global", "mc_psnr_ref_global", "tc_rmse_global"), _NAN))
        if live:
            out["mc_psnr_global"] = psnr_from_sse(sum(self.stats[t][5] for t in live), len(live) * n, bits)
            if self.has_ref:
                out["mc_psnr_ref_global"] = psnr_from_sse(sum(self.stats[t][7] for t in live), len(live) * n, bits)
                out["tc_rmse_global"] = tc_rmse(sum(self.stats[t][8] for t in live), len(live) * n, bits)
        return out
