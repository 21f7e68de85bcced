"""Geometric self-ensemble on the GPU (include/fdn_ensemble.h; the reference has no such option): the network runs on the flipped and
transposed copies of a frame, each result is mapped back, and the results are averaged - the "+" variant of restoration papers.

Codes k = 0 .. 7: bit 1 mirrors the columns, bit 2 mirrors the rows, bit 4 transposes, mirrors first; a set of codes is an 8-bit mask.
`ensemble` = 1, 2, 4 or 8 copies stands for MASKS[ensemble]: the identity, plus the column mirror, plus all mirrors, plus all of D4.

The copies are made by fdn_d4_pre_u8 (from uint8 frames) or fdn_d4_apply (from fp32 tiles) and folded back by fdn_d4_post_u8 /
fdn_d4_mean: the sum over ascending k of the inverse-transformed results in fp32, divided once by the number of copies.  The four
codes that transpose have another shape (w x h), so a set is handled as two halves, `a` (mask & 0x0F) and `b` (mask & 0xF0).  No CPU
fallback: the tensors must live on the ROCm device.

What the tests pin is that the result equals the composition of single passes, bit for bit.  No accuracy gain has been measured: only
tamed test weights exist here, no trained checkpoint.
"""
import ctypes

import torch

from . import FdnHipError, check, dev_as, lib, stream

MASKS = {1: 0x01, 2: 0x03, 4: 0x0F, 8: 0xFF}


def check_ensemble(ensemble):
    """the `ensemble` keyword -> its mask; anything but 1, 2, 4, 8 raises ValueError"""
    if isinstance(ensemble, bool) or ensemble not in MASKS:
        raise ValueError(f"ensemble {ensemble!r}: 1, 2, 4 or 8 copies")
    return MASKS[ensemble]


def codes(mask):
    """the codes of a mask in ascending order"""
    if isinstance(mask, bool) or not isinstance(mask, int) or not 1 <= mask <= 255:
        raise ValueError(f"mask {mask!r}: a set of the codes 0 .. 7, 1 .. 255")
    return [k for k in range(8) if mask >> k & 1]


def d4_shape(k, h, w):
    """the size of T_k of an h x w image"""
    if not 0 <= k <= 7:
        raise ValueError(f"code {k!r}: 0 .. 7")
    return (w, h) if k & 4 else (h, w)


def _half(mask):
    """a mask whose codes all make one shape -> True when that shape is the transposed one"""
    if mask & 0x0F and mask & 0xF0:
        raise ValueError(f"mask {mask:#04x} has codes on both sides of bit 4: one call makes one output shape")
    return bool(mask & 0xF0)


def _copies(src, dtype, what, mask, pad, call):
    """the body of pre_u8 / apply: src [B,h,w,3] uint8 or [N,3,h,w] float32 -> (out [K,B,3,H,W], h', w')"""
    from .harness import padded_size
    ks = codes(mask)
    tr = _half(mask)
    B = src.shape[0]
    h, w = (src.shape[1], src.shape[2]) if dtype == torch.uint8 else (src.shape[2], src.shape[3])
    hp, wp = (w, h) if tr else (h, w)
    H, W = padded_size(hp, wp) if pad else (hp, wp)
    if H - hp >= hp or W - wp >= wp:
        raise FdnHipError(f"reflect padding {hp}x{wp} -> {H}x{W} needs pad < size (F.pad raises the same way)")
    p = dev_as(src, dtype, what)
    out = torch.empty((len(ks), B, 3, H, W), device=src.device, dtype=torch.float32)
    call(p, ctypes.c_void_p(out.data_ptr()), B, h, w, H, W)
    return out, hp, wp


def pre_u8(img_u8, mask, bgr=True, pad=True):
    """uint8 [B,h,w,3] on the GPU -> (fp32 [K,B,3,H,W], h', w'): harness.preprocess of T_k(img) for every code k of mask, ascending;
    (H, W) = padded_size(h', w'), or (h', w') with pad=False.  The codes of one call all transpose or all do not."""
    if not isinstance(img_u8, torch.Tensor) or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise FdnHipError(f"expected uint8 images [B,h,w,3], got {tuple(getattr(img_u8, 'shape', ()))}")
    return _copies(img_u8, torch.uint8, "img", mask, pad, lambda p, o, B, h, w, H, W: check(
        lib().fdn_d4_pre_u8(p, o, B, h, w, H, W, mask, int(bool(bgr)), stream()), "fdn_d4_pre_u8"))


def apply(x, mask, pad=True):
    """fp32 [N,3,h,w] on the GPU -> (fp32 [K,N,3,H,W], h', w'): T_k(x) for every code k of mask, ascending, reflect-padded bottom /
    right as pre_u8 pads (nothing for the tiles of the tiled route, whose sides are multiples of 32)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
        raise FdnHipError(f"expected float32 images [N,3,h,w], got {tuple(getattr(x, 'shape', ()))}")
    return _copies(x, torch.float32, "x", mask, pad, lambda p, o, N, h, w, H, W: check(
        lib().fdn_d4_apply(p, o, N, h, w, H, W, mask, stream()), "fdn_d4_apply"))


def _results(res_a, res_b, mask, h, w):
    """the checks of mean / post_u8 -> (pointer a, pointer b, B, Ha, Wa, Hb, Wb, device)"""
    ks = codes(mask)
    ka, kb = sum(1 for k in ks if not k & 4), sum(1 for k in ks if k & 4)
    dims, ptrs, B, device = [], [], None, None
    sides = ((res_a, ka, (h, w), "res_a"), (res_b, kb, (w, h), "res_b"))
    for res, K, _, name in sides:
        if (res is None) != (K == 0):
            raise FdnHipError(f"{name} must be given exactly when mask {mask:#04x} has codes on its side of bit 4")
    for res, K, (hp, wp), name in sides:
        if res is None:
            dims += [0, 0]
            ptrs.append(None)
            continue
        ptrs.append(dev_as(res, torch.float32, name))
        if res.dim() != 5 or res.shape[0] != K or res.shape[2] != 3 or res.shape[3] < hp or res.shape[4] < wp or \
                (B is not None and res.shape[1] != B):
            raise FdnHipError(f"{name} must be [{K},B,3,>={hp},>={wp}], got {tuple(res.shape)}")
        B, device = res.shape[1], res.device
        dims += [res.shape[3], res.shape[4]]
    return ptrs[0], ptrs[1], B, dims, device


def mean(res_a, res_b, mask, h, w):
    """res_a fp32 [Ka,B,3,Ha,Wa] (the results on the codes of mask & 0x0F) and res_b [Kb,B,3,Hb,Wb] (mask & 0xF0), either None when its
    side is empty -> fp32 [B,3,h,w]: each result cropped, mapped back, summed in ascending k, divided once by K."""
    pa, pb, B, dims, device = _results(res_a, res_b, mask, h, w)
    out = torch.empty((B, 3, h, w), device=device, dtype=torch.float32)
    check(lib().fdn_d4_mean(pa, pb, ctypes.c_void_p(out.data_ptr()), B, h, w, *dims, mask, stream()), "fdn_d4_mean")
    return out


def post_u8(res_a, res_b, mask, h, w, bgr=True):
    """mean() then harness.postprocess in one launch -> uint8 [B,h,w,3], the same bits."""
    pa, pb, B, dims, device = _results(res_a, res_b, mask, h, w)
    out = torch.empty((B, h, w, 3), device=device, dtype=torch.uint8)
    check(lib().fdn_d4_post_u8(pa, pb, ctypes.c_void_p(out.data_ptr()), B, h, w, *dims, mask, int(bool(bgr)), stream()),
          "fdn_d4_post_u8")
    return out


@torch.no_grad()
def forward_ensemble(net, x_or_u8, ratio, ensemble, batch=8, bgr=True):
    """FDN on the MASKS[ensemble] copies of uint8 frames [B,h,w,3] (pre_u8) or fp32 images [B,3,h,w] (apply) -> (res_a, res_b, mask) as
    mean / post_u8 take them.  Eager forwards, one orientation at a time, at most `batch` samples each; ratio [B,1] is what the
    untransformed frames feed FDN, and every copy of a frame is fed that ratio (LPNet is not equivariant, and one frame has one
    brightness)."""
    mask = check_ensemble(ensemble)
    if batch < 1:
        raise FdnHipError(f"batch must be at least 1, got {batch}")
    B = x_or_u8.shape[0]
    if ratio is None or tuple(ratio.shape) != (B, 1):
        raise FdnHipError(f"forward_ensemble needs ratio [{B},1], got {None if ratio is None else tuple(ratio.shape)}")
    ratio = ratio.to(device=x_or_u8.device, dtype=torch.float32)
    halves = []
    for part in (mask & 0x0F, mask & 0xF0):
        if not part:
            halves.append(None)
            continue
        xs = pre_u8(x_or_u8, part, bgr=bgr)[0] if x_or_u8.dtype == torch.uint8 else apply(x_or_u8, part)[0]
        res = torch.empty_like(xs)
        for kk in range(xs.shape[0]):
            for s in range(0, B, batch):
                res[kk, s:s + batch] = net(xs[kk, s:s + batch], ratio_i=ratio[s:s + batch].contiguous(), device=xs.device)[0]
        halves.append(res)
    return halves[0], halves[1], mask
