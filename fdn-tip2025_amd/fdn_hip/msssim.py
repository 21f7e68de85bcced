"""Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) of 8-bit image pairs and of video luma planes (include/fdn_msssim.h,
libfdn_msssim.so): contrast and structure over five octaves, luminance only at the coarsest.  Residual blur over a few pixels costs the
fine levels, a tone shift across a region the coarse ones, which single-scale SSIM at full resolution does not tell apart.

mode "rgb"   three planes per image; the image's score is the mean of the three channels' MS-SSIM values, added in the order R, G, B.
mode "gray"  one plane y = 299 R + 587 G + 114 B (the integer of fdn_hip.sharpness's GMSD; NOT the Y of bgr2ycbcr).
luma         the Y plane of 4:2:0 video frames, 8 bit or 10 bit scored as 10 bit (peak 1023), never through 8-bit RGB.

The pyramid is Wang's: 2 x 2 block sums kept as exact integers down to the window, the last row / column counted twice at odd sizes;
the 11 x 11 Gaussian window (sigma 1.5) runs over 'valid' positions only, in float64 in a fixed order.  The coarsest of the five maps needs
11 x 11 samples, so both sides must be at least MIN_SIDE = 161: anything smaller is refused, no scale is dropped silently.  Two equal
planes score exactly 1.0; a negative mean contrast at any level clamps the score to 0.0, and the unclamped per-level means are returned
beside the score, so nothing is hidden.

Images are uint8 [B][h][w][3] (or one [h][w][3]), numpy arrays or tensors; frames as fdn_hip.video_metrics takes them.  Everything is
enqueued on the current stream; sums run in a fixed order and no floating-point atomic is used: a plane scores the same bits on every
call and wherever it sits in a batch.  The functions that return Python numbers copy the few words per plane back once per batch (which
synchronises).  No CPU fallback; msssim_dims and ms_ssim_from_sums are plain host arithmetic."""
import ctypes
import math
import os

import numpy as np
import torch

from . import FdnHipError, _declare, check, ptr, stream
from ._abi_msssim import PROTOTYPES, VERSION    # generated from include/fdn_msssim.h by tools/gen_abi_table.py
from .metrics import ssim3d_taps

ABI_VERSION = VERSION[1]
LEVELS, MIN_SIDE, TILE_H, TILE_W = 5, 161, 16, 32         # FDN_MSSSIM_LEVELS, _MIN_SIDE, _TILE_H, _TILE_W of include/fdn_msssim.h
MODES = {"rgb": 0, "gray": 1}                             # FDN_MSSSIM_RGB, FDN_MSSSIM_GRAY
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_TAPS = np.ascontiguousarray(ssim3d_taps(), dtype=np.float64)        # the host array the entry points read their window from

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_msssim.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_msssim.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has msssim ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def msssim_dims(h, w):
    """-> (levels, maps): five (h_s, w_s) and five (h_s - 10, w_s - 10) of an h x w plane (fdn_msssim_dims).  Host arithmetic, no GPU
    needed; FdnHipError below 161 in either side."""
    arr = [(ctypes.c_int * LEVELS)() for _ in range(4)]
    code = lib().fdn_msssim_dims(int(h), int(w), *arr)
    if code:
        raise FdnHipError(f"fdn_msssim_dims refuses {h}x{w}: MS-SSIM over five scales needs at least {MIN_SIDE}x{MIN_SIDE} (code {code})")
    lh, lw, mh, mw = (list(a) for a in arr)
    return list(zip(lh, lw)), list(zip(mh, mw))


def ms_ssim_from_sums(sums, sizes):
    """the host step.  sums: per level (the sum of cs, the sum of ss) over the level's map, five pairs; sizes: the five maps' numbers of
    positions -> {"ms_ssim", "levels"}: levels = the unclamped means of cs at levels 0 .. 3 and of ss at level 4, ms_ssim the product of
    max(mean, 0)^w in level order."""
    if len(sums) != LEVELS or len(sizes) != LEVELS:
        raise ValueError(f"{LEVELS} levels, got {len(sums)} sums and {len(sizes)} sizes")
    means = [float(sums[s][1 if s == LEVELS - 1 else 0]) / int(sizes[s]) for s in range(LEVELS)]
    score = math.pow(max(means[0], 0.0), WEIGHTS[0])
    for s in range(1, LEVELS):
        score = score * math.pow(max(means[s], 0.0), WEIGHTS[s])
    return {"ms_ssim": score, "levels": means}


def _sizes(h, w):
    return [a * b for a, b in msssim_dims(h, w)[1]]


def _split(buf, P, shapes):
    """a level-after-level buffer -> one [P][rows][cols] view per level"""
    out, at = [], 0
    for r, c in shapes:
        out.append(buf[at:at + P * r * c].view(P, r, c))
        at += P * r * c
    return out


def _launch(call, what, B, planes, h, w, dev, want_pyr=False, want_maps=False):
    """enqueue one scoring entry: call(taps, pyr_a, pyr_b, cs_map, ss_map, ws, out) -> the status.  -> (out float64 [P][5][2] on the
    device, (levels 1 .. 4 of a, of b) or None, (cs maps, ss maps of levels 0 .. 4) or None)"""
    nws = int(lib().fdn_msssim_ws(B, planes, h, w))
    if nws <= 0:
        raise FdnHipError(f"{what}: fdn_msssim_ws refuses {B} images of {h}x{w}: MS-SSIM over five scales needs at least {MIN_SIDE}x{MIN_SIDE}")
    levels, maps = msssim_dims(h, w)
    P = B * planes
    ws = torch.empty(nws, dtype=torch.float64, device=dev)
    out = torch.empty((P, LEVELS, 2), dtype=torch.float64, device=dev)
    pa = pb = cs = ss = None
    if want_pyr:
        n = P * sum(a * b for a, b in levels[1:])
        pa, pb = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    if want_maps:
        n = P * sum(a * b for a, b in maps)
        cs, ss = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(call(ctypes.c_void_p(_TAPS.ctypes.data), ptr(pa), ptr(pb), ptr(cs), ptr(ss), ptr(ws), ptr(out)), what)
    pyr = (_split(pa, P, levels[1:]), _split(pb, P, levels[1:])) if want_pyr else None
    mp = (_split(cs, P, maps), _split(ss, P, maps)) if want_maps else None
    return out, pyr, mp


def _mode(mode):
    if mode not in MODES:
        raise FdnHipError(f"mode {mode!r}: rgb or gray")
    return MODES[mode], (3 if mode == "rgb" else 1)


def _u8(gt, restored, mode, bgr, what, **want):
    from .metrics import _u8_pair
    code, planes = _mode(mode)
    a, b, single = _u8_pair(gt, restored, 0, what)
    B, h, w, _ = a.shape
    if h < MIN_SIDE or w < MIN_SIDE:
        raise FdnHipError(f"{what}: {h}x{w} is too small: MS-SSIM over five scales needs at least {MIN_SIDE}x{MIN_SIDE}")
    if h * w > 2 ** 31 - 1:
        raise FdnHipError(f"{what}: {h}x{w} has more than 2^31 - 1 pixels")
    l = lib()
    call = lambda taps, pa, pb, cs, ss, ws, out: l.fdn_msssim_u8(ptr(a), ptr(b), B, h, w, code, int(bool(bgr)), taps, pa, pb, cs, ss, ws, out,  # noqa: E731
                                                                 stream())
    return _launch(call, "fdn_msssim_u8", B, planes, h, w, a.device, **want) + (B, planes, h, w, single)


def _luma(a, b, h, w, fmt, what, **want):
    from .harness import _yuv_frames, _yuv_ptr
    a, b = _yuv_frames(a, h, w, fmt), _yuv_frames(b, h, w, fmt)
    if b.shape != a.shape or b.device != a.device:
        raise FdnHipError(f"the two streams differ: {tuple(a.shape)} on {a.device}, {tuple(b.shape)} on {b.device}")
    if h < MIN_SIDE or w < MIN_SIDE:
        raise FdnHipError(f"{what}: {h}x{w} is too small: MS-SSIM over five scales needs at least {MIN_SIDE}x{MIN_SIDE}")
    pa, pb = _yuv_ptr(a, "frames"), _yuv_ptr(b, "frames")
    B, stride = a.shape[0], a.shape[1]
    l = lib()
    call = lambda taps, qa, qb, cs, ss, ws, out: l.fdn_msssim_luma(pa, pb, B, h, w, fmt.bits, stride, taps, qa, qb, cs, ss, ws, out, stream())  # noqa: E731
    return _launch(call, "fdn_msssim_luma", B, 1, h, w, a.device, **want) + (B,)


def _records(rows, B, planes, sizes):
    """the host step on the [P][5][2] sums of a batch -> one dict per image"""
    res = []
    for i in range(B):
        per = [ms_ssim_from_sums(rows[i * planes + k], sizes) for k in range(planes)]
        if planes == 1:
            res.append(per[0])
        else:
            score = (per[0]["ms_ssim"] + per[1]["ms_ssim"] + per[2]["ms_ssim"]) / 3
            levels = [(per[0]["levels"][s] + per[1]["levels"][s] + per[2]["levels"][s]) / 3 for s in range(LEVELS)]
            res.append({"ms_ssim": score, "levels": levels, "channels": [p["ms_ssim"] for p in per], "channel_levels": [p["levels"] for p in per]})
    return res


def ms_ssim_sums_u8(gt, restored, mode="rgb", bgr=True):
    """-> (rows, sizes): per plane (three per image in the order R, G, B for rgb, else one) the five (sum of cs, sum of ss) pairs of
    fdn_msssim_u8 as floats, and the five maps' numbers of positions"""
    out, _, _, B, planes, h, w, _ = _u8(gt, restored, mode, bgr, "ms_ssim_u8")
    return out.cpu().tolist(), _sizes(h, w)


def ms_ssim_u8(gt, restored, mode="rgb", bgr=True):
    """gt, restored: B, G, R bytes with bgr (as cv2 reads them) else R, G, B -> a list of B dicts (also for one (h,w,3) pair): ms_ssim,
    levels (the five unclamped per-level means; for rgb the mean over the channels) and for rgb channels (the scores of R, G, B) and
    channel_levels.  Two equal images give exactly 1.0.  An image below 161 in either side raises FdnHipError."""
    out, _, _, B, planes, h, w, _ = _u8(gt, restored, mode, bgr, "ms_ssim_u8")
    return _records(out.cpu().tolist(), B, planes, _sizes(h, w))


def ms_ssim_pyramids_u8(gt, restored, mode="rgb", bgr=True):
    """-> (levels of gt, levels of restored): each a list of four int32 tensors [P][h_s][w_s] on the device, levels 1 .. 4, exact"""
    return _u8(gt, restored, mode, bgr, "ms_ssim_pyramids_u8", want_pyr=True)[1]


def ms_ssim_maps_u8(gt, restored, mode="rgb", bgr=True, with_scores=False):
    """-> (cs maps, ss maps): each a list of five float64 tensors [P][h_s - 10][w_s - 10] on the device, levels 0 .. 4.
    with_scores: -> (the list of ms_ssim_u8, those maps), from the same launches."""
    out, _, maps, B, planes, h, w, _ = _u8(gt, restored, mode, bgr, "ms_ssim_maps_u8", want_maps=True)
    return (_records(out.cpu().tolist(), B, planes, _sizes(h, w)), maps) if with_scores else maps


def ms_ssim_sums_luma(a, b, h, w, fmt):
    """frames a, b [B, h*w*3/2] as fdn_hip.video_metrics takes them -> (rows, sizes) as ms_ssim_sums_u8, one row per frame"""
    out = _luma(a, b, h, w, fmt, "ms_ssim_luma")[0]
    return out.cpu().tolist(), _sizes(h, w)


def ms_ssim_luma(a, b, h, w, fmt):
    """-> a list of B dicts {ms_ssim, levels} for the luma planes of the frames; 10 bit is scored against the peak 1023"""
    out, _, _, B = _luma(a, b, h, w, fmt, "ms_ssim_luma")
    return _records(out.cpu().tolist(), B, 1, _sizes(h, w))


def ms_ssim_pyramids_luma(a, b, h, w, fmt):
    """-> (levels of a, levels of b) as ms_ssim_pyramids_u8, P = B"""
    return _luma(a, b, h, w, fmt, "ms_ssim_pyramids_luma", want_pyr=True)[1]


def ms_ssim_maps_luma(a, b, h, w, fmt):
    """-> (cs maps, ss maps) as ms_ssim_maps_u8, P = B"""
    return _luma(a, b, h, w, fmt, "ms_ssim_maps_luma", want_maps=True)[2]


class MsSsimScore:
    """MS-SSIM on luma of ONE stream of h x w frames of VideoFormat fmt against its ground-truth stream, taken in order: update(dist,
    ref) takes a batch and appends one record {ms_ssim_y, levels} per frame to .frames; summary() gives the mean over the frames (nan
    without one).  An object of its own beside fdn_hip.video_metrics.VideoScore, whose records stay what they were.  ValueError for a
    frame below 161 in either side, before anything touches the GPU."""

    def __init__(self, h, w, fmt, device="cuda"):
        h, w = int(h), int(w)
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"MS-SSIM over five scales needs frames of at least {MIN_SIDE}x{MIN_SIDE}, got {w}x{h}")
        self.h, self.w, self.fmt = h, w, fmt
        self.device = torch.device(device)
        self.frames = []

    def update(self, dist, ref):
        if ref is None:
            raise FdnHipError("MS-SSIM needs a ground-truth stream")
        recs = [{"ms_ssim_y": r["ms_ssim"], "levels": r["levels"]} for r in ms_ssim_luma(ref, dist, self.h, self.w, self.fmt)]
        self.frames += recs
        return recs

    def summary(self):
        n = len(self.frames)
        return {"frames": n, "ms_ssim_y": math.fsum(r["ms_ssim_y"] for r in self.frames) / n if n else float("nan")}
