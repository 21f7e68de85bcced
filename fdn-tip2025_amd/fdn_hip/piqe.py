"""PIQE, the perception-based no-reference image quality evaluator (Venkatanath et al., NCC 2015; MATLAB's `piqe`), of 8-bit images and
of video luma planes (include/fdn_piqe.h, libfdn_piqe.so).  It needs no ground truth, no trained model and no data file: the plane is
normalised by a 7 x 7 Gaussian (MSCN), cut into 16 x 16 blocks, and every block whose variance exceeds 0.1 is priced for two failure
modes: a flat six-sample segment on one of its edges (blocking, WNDC) and a centre that is noisier than its surround (noise, WNC).
0 is best, 100 is worst.

The header is the definition: it was written out from the paper and MATLAB's documented constants, and where MATLAB's piqe differs in a
detail (the exact rgb2gray coefficients, for one) the header wins.  No comparison against MATLAB or pyiqa has been made.

images       uint8 [B][h][w][3] (or one [h][w][3]), numpy arrays or tensors; scored on the gray code (299 R + 587 G + 114 B + 500) / 1000.
luma         the Y plane of 4:2:0 video frames, as fdn_hip.video_metrics takes them; 10 bit keeps its two extra bits as quarters of a
             code, so a 10-bit plane of codes 4 c scores the bits of the 8-bit plane of codes c.

A flat image has no active block and scores exactly 100.0: that is the published behaviour, the score of an image PIQE has nothing to
say about is its worst.  Any size from 1 x 1 is taken; the plane is padded to whole blocks by replication.

Everything is enqueued on the current stream; sums run in a fixed order and no floating-point atomic is used: a plane scores the same
bits on every call and wherever it sits in a batch.  The functions that return Python numbers copy two words per plane back once per
batch (which synchronises).  No CPU fallback; piqe_dims and piqe_from_sums are plain host arithmetic."""
import ctypes
import math
import os

import numpy as np
import torch

from . import FdnHipError, _declare, check, ptr, stream
from ._abi_piqe import PROTOTYPES, VERSION    # generated from include/fdn_piqe.h by tools/gen_abi_table.py

ABI_VERSION = VERSION[1]
BLOCK, TILE_H, TILE_W = 16, 32, 64                        # FDN_PIQE_BLOCK, _TILE_H, _TILE_W of include/fdn_piqe.h
ACTIVE, WNDC, WNC = 1, 2, 4                               # FDN_PIQE_ACTIVE, _WNDC, _WNC: the bits of a block's class byte


def piqe_taps():
    """the 7 taps exp(-t^2 / (2 (7/6)^2)), t = -3 .. 3, normalised, float64"""
    t = np.arange(7, dtype=np.float64) - 3.0
    k = np.exp(-(t * t) / (2.0 * (7.0 / 6.0) * (7.0 / 6.0)))
    return k / k.sum()


_TAPS = np.ascontiguousarray(piqe_taps(), dtype=np.float64)          # the host array the entry points read their window from

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_piqe.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_piqe.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has piqe ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def piqe_dims(h, w):
    """-> {"H", "W", "blocks": (rows, cols), "tiles": (rows, cols)} of an h x w plane (fdn_piqe_dims).  Host arithmetic, no GPU needed."""
    d = (ctypes.c_int * 6)()
    code = lib().fdn_piqe_dims(int(h), int(w), d)
    if code:
        raise FdnHipError(f"fdn_piqe_dims refuses {h}x{w} (code {code})")
    return {"H": d[0], "W": d[1], "blocks": (d[2], d[3]), "tiles": (d[4], d[5])}


def piqe_from_sums(D, nhsa):
    """the host step: D the sum of the active blocks' distortions, nhsa their number -> (D + 1) / (1 + nhsa) * 100"""
    return (float(D) + 1.0) / (1.0 + float(nhsa)) * 100.0


def _launch(call, what, B, h, w, dev, maps=False, ws=None):
    """enqueue one scoring entry: call(taps, mscn, var, cls, ws, out) -> the status.  -> (out float64 [B][2] on the device, None or
    {"mscn": float64 [B][H][W], "var": float64 [B][H/16][W/16], "cls": uint8 [B][H/16][W/16]})"""
    nws = int(lib().fdn_piqe_ws(B, h, w))
    if nws <= 0:
        raise FdnHipError(f"{what}: fdn_piqe_ws refuses {B} planes of {h}x{w}")
    d = piqe_dims(h, w)
    if ws is None:
        ws = torch.empty(nws, dtype=torch.float64, device=dev)
    elif ws.dtype != torch.float64 or ws.numel() < nws or ws.device != dev or not ws.is_contiguous():
        raise FdnHipError(f"{what}: the workspace must be {nws} contiguous float64 words on {dev}")
    out = torch.empty((B, 2), dtype=torch.float64, device=dev)
    m = None
    if maps:
        nb = d["blocks"]
        m = {"mscn": torch.empty((B, d["H"], d["W"]), dtype=torch.float64, device=dev),
             "var": torch.empty((B,) + nb, dtype=torch.float64, device=dev), "cls": torch.empty((B,) + nb, dtype=torch.uint8, device=dev)}
    with torch.cuda.device(dev):
        check(call(ctypes.c_void_p(_TAPS.ctypes.data), ptr(m["mscn"]) if m else None, ptr(m["var"]) if m else None,
                   ptr(m["cls"]) if m else None, ptr(ws), ptr(out)), what)
    return out, m


def _images(img, what):
    """-> contiguous uint8 [B][h][w][3] on a ROCm device"""
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise FdnHipError(f"{what} takes uint8 images (h,w,3) or (B,h,w,3), numpy arrays or tensors, got "
                          f"{getattr(img, 'dtype', type(img).__name__)} {tuple(getattr(img, 'shape', ()))}")
    img = img if img.dim() == 4 else img.unsqueeze(0)
    B, h, w, _ = img.shape
    if B < 1 or h < 1 or w < 1:
        raise FdnHipError(f"{what}: nothing to score in {tuple(img.shape)}")
    if not img.is_cuda:
        if not torch.cuda.is_available():
            raise FdnHipError(f"{what} needs a ROCm device; there is no CPU fallback")
        img = img.to(torch.device("cuda", torch.cuda.current_device()))
    return img.contiguous()


def piqe_sums_u8(images, bgr=False, maps=False, ws=None):
    """-> (out, maps): out float64 [B][2] = {D, NHSA} per image on the device (fdn_piqe_u8), maps None or the dict of _launch.  ws: a
    float64 device tensor to use as the workspace instead of a fresh one (its contents do not matter)."""
    a = _images(images, "piqe_u8")
    B, h, w, _ = a.shape
    l = lib()
    call = lambda taps, mscn, var, cls, wsp, out: l.fdn_piqe_u8(ptr(a), B, h, w, int(bool(bgr)), taps, mscn, var, cls, wsp, out, stream())  # noqa: E731
    return _launch(call, "fdn_piqe_u8", B, h, w, a.device, maps, ws)


def piqe_sums_luma(frames, h, w, fmt, maps=False, ws=None):
    """frames [B, h*w*3/2] as fdn_hip.video_metrics takes them -> (out, maps) as piqe_sums_u8, one row per frame"""
    from .harness import _yuv_frames, _yuv_ptr
    a = _yuv_frames(frames, h, w, fmt)
    p = _yuv_ptr(a, "frames")
    B, stride = a.shape[0], a.shape[1]
    l = lib()
    call = lambda taps, mscn, var, cls, wsp, out: l.fdn_piqe_luma(p, B, h, w, fmt.bits, stride, taps, mscn, var, cls, wsp, out, stream())  # noqa: E731
    return _launch(call, "fdn_piqe_luma", B, h, w, a.device, maps, ws)


def _records(out):
    return [{"piqe": piqe_from_sums(D, n), "d": D, "nhsa": int(n)} for D, n in out.cpu().tolist()]


def piqe_u8(images, bgr=False, maps=False):
    """images: R, G, B bytes (bgr: B, G, R, as cv2 reads them) -> a list of B dicts (also for one (h,w,3) image): piqe (0 best, 100
    worst; exactly 100.0 for an image without an active block), d (the sum of the active blocks' distortions) and nhsa (their number).
    maps: -> (that list, {"mscn", "var", "cls"}): the MSCN plane [B][H][W], the block variances and the block classes (bit 0 active,
    bit 1 WNDC, bit 2 WNC) [B][H/16][W/16], on the device, from the same launch."""
    out, m = piqe_sums_u8(images, bgr, maps)
    return (_records(out), m) if maps else _records(out)


def piqe_luma(frames, h, w, fmt, maps=False):
    """-> a list of B dicts {piqe, d, nhsa} for the luma planes of the frames (maps as piqe_u8); 10-bit codes count as quarters"""
    out, m = piqe_sums_luma(frames, h, w, fmt, maps)
    return (_records(out), m) if maps else _records(out)


def piqe_line(rec, name="PIQE"):
    """one record -> the text the command lines print for it"""
    return f"{name}: {rec['piqe']:.6f} ({rec['nhsa']} active blocks)"


class PiqeScore:
    """PIQE on luma of ONE stream of h x w frames of VideoFormat fmt, taken in order: update(frames) takes a batch and appends one
    record {piqe_y, nhsa} per frame to .frames; summary() gives the mean over the frames (nan without one).  An object of its own
    beside fdn_hip.video_metrics.VideoScore, whose records stay what they were; it needs no reference stream.  Frames are moved to `device`."""

    def __init__(self, h, w, fmt, device="cuda"):
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"PIQE needs frames of at least 1x1, got {w}x{h}")
        self.h, self.w, self.fmt = h, w, fmt
        self.device = torch.device(device)
        self.frames = []

    def update(self, frames):
        if isinstance(frames, torch.Tensor):
            frames = frames.to(self.device)                                           # scored on the device the object was made for
        recs = [{"piqe_y": r["piqe"], "nhsa": r["nhsa"]} for r in piqe_luma(frames, self.h, self.w, self.fmt)]
        self.frames += recs
        return recs

    def summary(self):
        n = len(self.frames)
        return {"frames": n, "piqe_y": math.fsum(r["piqe_y"] for r in self.frames) / n if n else float("nan")}
