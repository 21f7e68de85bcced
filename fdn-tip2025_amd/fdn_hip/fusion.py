"""Exposure fusion of K renderings of one frame (include/fdn_fusion.h, libfdn_fusion.so; Mertens, Kautz, Van Reeth 2007).

FDN's brightness is one scalar per frame, ratio_i.  A night scene with lamps has no right value: what opens the shadows burns the lamps.
Here a frame is rendered at a bracket of ratios around the one it would be fed, every pixel of every rendering is weighed by contrast,
saturation and well-exposedness, and the renderings are blended level by level through Laplacian pyramids into one locally exposed frame.

    weights(imgs, h, w, exponents)        fp32 [K,3,H,W] -> the normalised weights fp32 [K,h,w] (evaluated in double, rounded once)
    pyr_down(x, h, w), pyr_up(c, h, w)    the two resampling steps of the pyramids, on C planes
    fuse_pyramid(imgs, weights, h, w)     -> fp32 [3,h,w], not clamped: harness.postprocess finishes it
    fuse(imgs, h, w, exponents)           weights then fuse_pyramid
    check_bracket(evs), bracket_ratios(ratio, evs)     the stops of a bracket and the ratios they make of a frame's ratio

imgs are the results of K forwards on one padded frame; only [:h, :w] is read, and every sample is clamped to [0, 1] as it is read.
Everything is enqueued on the current stream; every sum runs in a fixed order and no floating-point atomic is used: a frame fuses to the
same bits on every call.  The header writes out the order of the pyramid's fp32 operations, and a float32 numpy restatement reproduces
them bit for bit.  No CPU fallback."""
import ctypes
import math
import os

import torch

from . import FdnHipError, _declare, check, dev, ptr, stream
from ._abi_fusion import PROTOTYPES, VERSION    # generated from include/fdn_fusion.h by tools/gen_abi_table.py

ABI_VERSION = VERSION[1]
MAX_K, MAX_LEVELS, TILE = 16, 16, 32                      # FDN_FUSION_MAX_K, FDN_FUSION_MAX_LEVELS, FDN_FUSION_TILE of include/fdn_fusion.h

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_fusion.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_fusion.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has fusion ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def check_bracket(evs):
    """The stops of a bracket -> a tuple of 1 to 16 distinct finite floats, in the caller's order; anything else raises ValueError."""
    try:
        evs = tuple(float(v) for v in evs)
    except (TypeError, ValueError):
        raise ValueError(f"bracket {evs!r}: a sequence of exposure stops, for example (-1, 0, 1)")
    if not 1 <= len(evs) <= MAX_K:
        raise ValueError(f"bracket of {len(evs)} stops: 1 to {MAX_K}")
    if not all(math.isfinite(v) for v in evs):
        raise ValueError(f"bracket {evs}: every stop must be finite")
    if len(set(evs)) != len(evs):
        raise ValueError(f"bracket {evs}: a stop is given twice")
    return evs


def check_exponents(exponents):
    """(wc, ws, we), the exponents of contrast, saturation and well-exposedness -> three finite floats >= 0; else ValueError"""
    try:
        e = tuple(float(v) for v in exponents)
    except (TypeError, ValueError):
        raise ValueError(f"fusion weights {exponents!r}: three numbers, the exponents of contrast, saturation and well-exposedness")
    if len(e) != 3 or not all(math.isfinite(v) and v >= 0 for v in e):
        raise ValueError(f"fusion weights {exponents!r}: three finite numbers >= 0")
    return e


def bracket_ratios(ratio, evs):
    """ratio [B,1] (what FDN would be fed for each frame) -> [B,K,1], ratio * 2^-ev for every stop of the bracket: ratio_i is the input's
    mean gray over the target's, so a positive stop, a smaller ratio, makes the frame brighter.  Nothing is clamped: a ratio outside
    what a checkpoint was trained on is the caller's business."""
    evs = check_bracket(evs)
    if not isinstance(ratio, torch.Tensor) or ratio.dim() != 2 or ratio.shape[1] != 1:
        raise FdnHipError(f"bracket_ratios needs ratio [B,1], got {tuple(getattr(ratio, 'shape', ()))}")
    scale = torch.tensor([2.0 ** -ev for ev in evs], dtype=torch.float32, device=ratio.device)
    return ratio.to(torch.float32).reshape(-1, 1, 1) * scale.reshape(1, -1, 1)


def dims(h, w):
    """-> (L, [(h_0, w_0), ..., (h_L, w_L)]): the levels of the pyramid of an h x w frame and their sizes (fdn_fusion_dims; n_{l+1} =
    (n_l + 1) // 2).  Host arithmetic, no GPU needed."""
    L = ctypes.c_int(0)
    check(lib().fdn_fusion_dims(int(h), int(w), ctypes.byref(L)), "fdn_fusion_dims")
    sizes = [(int(h), int(w))]
    for _ in range(L.value):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return L.value, sizes


def _imgs(imgs, h, w, what):
    if not isinstance(imgs, torch.Tensor) or imgs.dim() != 4 or imgs.shape[1] != 3:
        raise FdnHipError(f"{what}: imgs must be fp32 [K,3,H,W], got {tuple(getattr(imgs, 'shape', ()))}")
    K, _, H, W = imgs.shape
    if not 1 <= K <= MAX_K:
        raise FdnHipError(f"{what}: {K} renderings, 1 to {MAX_K} can be fused")
    if not (1 <= h <= H and 1 <= w <= W):
        raise FdnHipError(f"{what}: cannot read {h}x{w} out of {tuple(imgs.shape)}")
    if h * w > 2 ** 31 - 1:
        raise FdnHipError(f"{what}: {h}x{w} has more than 2^31 - 1 pixels")
    return dev(imgs, "imgs"), K, H, W


def weights(imgs, h, w, exponents=(1, 1, 1)):
    """imgs fp32 [K,3,H,W] -> fp32 [K,h,w]: contrast^wc * saturation^ws * well-exposedness^we + 1e-12 of every pixel of [:h, :w],
    normalised over k (fdn_fuse_weights).  An exponent 0 leaves its factor out."""
    wc, ws, we = check_exponents(exponents)
    p, K, H, W = _imgs(imgs, h, w, "weights")
    out = torch.empty((K, h, w), dtype=torch.float32, device=imgs.device)
    with torch.cuda.device(imgs.device):
        check(lib().fdn_fuse_weights(p, ptr(out), K, h, w, H, W, wc, ws, we, stream()), "fdn_fuse_weights")
    return out


def _planes(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise FdnHipError(f"{what} must be fp32 planes [C,H,W], got {tuple(getattr(x, 'shape', ()))}")
    return dev(x, what)


def pyr_down(x, h=None, w=None, clamp=False):
    """x fp32 [C,H,W], of which [:h, :w] is the level (default: all of it) -> [C,(h+1)//2,(w+1)//2]: the taps (1, 4, 6, 4, 1) / 16 per axis
    at every second sample, reflected at the edge (fdn_pyr_down).  clamp: samples clamped to [0, 1] as they are read."""
    p = _planes(x, "x")
    C, H, W = x.shape
    h, w = H if h is None else int(h), W if w is None else int(w)
    if not (1 <= h <= H and 1 <= w <= W):
        raise FdnHipError(f"pyr_down: cannot read {h}x{w} out of {tuple(x.shape)}")
    out = torch.empty((C, (h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().fdn_pyr_down(p, ptr(out), C, h, w, H, W, int(bool(clamp)), stream()), "fdn_pyr_down")
    return out


def pyr_up(c, h, w):
    """c fp32 [C,(h+1)//2,(w+1)//2] -> [C,h,w]: even samples (c[j-1] + 6 c[j] + c[j+1]) / 8, odd ones (c[j] + c[j+1]) / 2, per axis
    (fdn_pyr_up)."""
    h, w = int(h), int(w)
    if h < 1 or w < 1 or not isinstance(c, torch.Tensor) or c.dim() != 3 or tuple(c.shape[1:]) != ((h + 1) // 2, (w + 1) // 2):
        raise FdnHipError(f"pyr_up to {h}x{w} needs planes of {(h + 1) // 2}x{(w + 1) // 2}, got {tuple(getattr(c, 'shape', ()))}")
    p = _planes(c, "c")
    out = torch.empty((c.shape[0], h, w), dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        check(lib().fdn_pyr_up(p, ptr(out), c.shape[0], h, w, stream()), "fdn_pyr_up")
    return out


def fuse_pyramid(imgs, weights, h, w):
    """imgs fp32 [K,3,H,W], weights fp32 [K,h,w] -> fp32 [3,h,w]: the renderings blended level by level with the Gaussian pyramids of the
    weight planes, and collapsed (fdn_fuse_pyramid).  Not clamped."""
    p, K, H, W = _imgs(imgs, h, w, "fuse_pyramid")
    if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (K, h, w) or weights.device != imgs.device:
        raise FdnHipError(f"fuse_pyramid: weights must be fp32 [{K},{h},{w}] beside imgs, got {tuple(getattr(weights, 'shape', ()))}")
    pw = dev(weights, "weights")
    nws = int(lib().fdn_fusion_ws(K, h, w))
    if nws < 0:
        raise FdnHipError(f"fdn_fusion_ws refuses {K} renderings of {h}x{w}")
    work = torch.empty(nws // 4, dtype=torch.float32, device=imgs.device) if nws else None
    out = torch.empty((3, h, w), dtype=torch.float32, device=imgs.device)
    with torch.cuda.device(imgs.device):
        check(lib().fdn_fuse_pyramid(p, pw, ptr(out), ptr(work), K, h, w, H, W, stream()), "fdn_fuse_pyramid")
    return out


def fuse(imgs, h, w, exponents=(1, 1, 1)):
    """imgs fp32 [K,3,H,W] -> fp32 [3,h,w]: weights(imgs, h, w, exponents), then fuse_pyramid with them."""
    return fuse_pyramid(imgs, weights(imgs, h, w, exponents), h, w)
