"""Low-light evaluation (include/fdn_lowlight.h): the two scores a low-light enhancer is judged by besides PSNR and SSIM.

LOE, the lightness order error (after Wang et al. 2013), compares the INPUT with the ENHANCED image and needs no ground truth: with
L = max(R, G, B) the lightness of a pixel and S a set of m sample pixels,

    RD(p) = #{q in S : [La(p) >= La(q)] != [Lb(p) >= Lb(q)]},      LOE = (1 / m) sum_p RD(p),

how often the enhancement reversed the order of two pixels' lightness.  No pair is compared: the count comes exactly from the 256 x 256
joint histogram of (La, Lb) and its 2-D prefix sum, in integers, so `size=0` (every pixel) costs little more than a thumbnail.
`size=50` samples a grid whose short side has 50 points, as the usual implementation does; the sampling rule (fdn_lowlight.h) is this
project's own, so scores at size 50 are comparable in scale to published ones but not claimed equal to any other script's.

dE00, the CIEDE2000 colour difference (Sharma, Wu, Dalal 2005, kL = kC = kH = 1) of a restored image against its ground truth: sRGB
bytes -> linear RGB -> XYZ (D65) -> CIELAB -> dE00 per pixel in float64, then the mean and the maximum over the image.

Images are uint8 [B][h][w][3] (or one [h][w][3]).  Everything is enqueued on the current stream; integer sums are exact, float64 sums run
in a fixed order: an image scores the same bits on every call and wherever it sits in a batch.  The functions that return Python numbers
copy the few words per image back once per batch (which synchronises).  No CPU fallback."""
import ctypes

import torch

from . import FdnHipError, check, lib, ptr, stream

LOE_WS_WORDS = 65792            # 8-byte words of workspace per image: uint32 J[256][256], C[256][256], R[256], K[256]


def _size(size):
    if isinstance(size, bool) or not isinstance(size, int) or not 0 <= size < 2 ** 31:
        raise FdnHipError(f"size must be an integer >= 0 (0 = every pixel), got {size!r}")
    return size


def _pair(a, b, what):
    from .metrics import _u8_pair
    a, b, _ = _u8_pair(a, b, 0, what)
    if a.shape[1] * a.shape[2] > 2 ** 31 - 1:
        raise FdnHipError(f"{what}: {a.shape[1]}x{a.shape[2]} has more than 2^31 - 1 pixels")
    return a, b


def sample_dims(h, w, size=50):
    """-> (Md, Nd), the sample grid of an h x w image at `size` (fdn_loe_sample_dims).  Host arithmetic, no GPU needed."""
    md, nd = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().fdn_loe_sample_dims(int(h), int(w), _size(size), ctypes.byref(md), ctypes.byref(nd)), "fdn_loe_sample_dims")
    return md.value, nd.value


def _loe_launch(a, b, size, out):
    """enqueue fdn_loe_u8 on contiguous device tensors; out: int64 [B][2] (or a view of 2 B words) -> the workspace with the tables"""
    B, h, w, _ = a.shape
    nws = int(lib().fdn_loe_ws(B, h, w, size))
    if nws <= 0:
        raise FdnHipError(f"fdn_loe_ws refuses {B} images of {h}x{w} at size {size}")
    ws = torch.empty(nws, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().fdn_loe_u8(ptr(a), ptr(b), B, h, w, size, ptr(ws), ptr(out), stream()), "fdn_loe_u8")
    return ws


def loe_counts_u8(inp, enh, size=50):
    """-> (numerators, m): B ints, the sum of RD over the samples of every image, and the number of samples.  Exact."""
    size = _size(size)
    a, b = _pair(inp, enh, "loe_u8")
    out = torch.empty((a.shape[0], 2), dtype=torch.int64, device=a.device)
    _loe_launch(a, b, size, out)
    host = out.cpu().tolist()
    return [int(r[0]) for r in host], int(host[0][1])


def loe_u8(inp, enh, size=50):
    """inp (the input), enh (its enhanced version): uint8 [B][h][w][3] -> list of B floats, LOE = numerator / m."""
    num, m = loe_counts_u8(inp, enh, size)
    return [n / m for n in num]


def loe_map_u8(inp, enh, size=50):
    """-> uint32 tensor [B][Md][Nd] on the device: RD of every sample, the picture of where the order broke.  It sums to the numerator;
    RD / m is the share of the samples whose order against this one was reversed."""
    size = _size(size)
    a, b = _pair(inp, enh, "loe_map_u8")
    B, h, w, _ = a.shape
    md, nd = sample_dims(h, w, size)
    out = torch.empty((B, 2), dtype=torch.int64, device=a.device)
    ws = _loe_launch(a, b, size, out)
    rd = torch.empty((B, md, nd), dtype=torch.uint32, device=a.device)
    with torch.cuda.device(a.device):
        check(lib().fdn_loe_map_u8(ptr(a), ptr(b), B, h, w, size, ptr(ws), ptr(rd), stream()), "fdn_loe_map_u8")
    return rd


def _deltae_launch(a, b, bgr, out, want_map):
    B, h, w, _ = a.shape
    nws = int(lib().fdn_deltae00_ws(B, h, w))
    if nws <= 0:
        raise FdnHipError(f"fdn_deltae00_ws refuses {B} images of {h}x{w}")
    ws = torch.empty(nws, dtype=torch.float64, device=a.device)
    dmap = torch.empty((B, h, w), dtype=torch.float32, device=a.device) if want_map else None
    with torch.cuda.device(a.device):
        check(lib().fdn_deltae00_u8(ptr(a), ptr(b), B, h, w, int(bool(bgr)), ptr(dmap), ptr(ws), ptr(out), stream()), "fdn_deltae00_u8")
    return dmap


def deltae00_u8(gt, restored, bgr=True, want_map=False):
    """gt, restored: uint8 [B][h][w][3], B, G, R bytes with bgr (as cv2 reads them) else R, G, B -> (means, maxima[, map]): per image the
    mean and the largest dE00 over its pixels as floats, and with want_map the float32 tensor [B][h][w] of every pixel's dE00 on the
    device.  Two equal images give exactly 0.0."""
    a, b = _pair(gt, restored, "deltae00_u8")
    B, h, w, _ = a.shape
    out = torch.empty((B, 2), dtype=torch.float64, device=a.device)
    dmap = _deltae_launch(a, b, bgr, out, want_map)
    host = out.cpu().tolist()
    res = ([r[0] / (h * w) for r in host], [r[1] for r in host])
    return res + (dmap,) if want_map else res


def lowlight_metrics(inp, enh, gt=None, size=50, bgr=True, want_loe_map=False):
    """inp (the input), enh (its enhanced version), gt (the ground truth, or None): uint8 [B][h][w][3] -> a list of B dicts with
    loe, loe_numerator, loe_samples and, with gt, deltae (the mean dE00 of enh against gt) and deltae_max.  One device-to-host copy.
    want_loe_map: -> (that list, the uint32 tensor [B][Md][Nd] of loe_map_u8 on the device), from the tables of the same launch."""
    size = _size(size)
    a, b = _pair(inp, enh, "lowlight_metrics")
    B, h, w, _ = a.shape
    buf = torch.empty(4 * B, dtype=torch.int64, device=a.device)       # {numerator, m} of every image, then {sum, max} as float64
    ws = _loe_launch(a, b, size, buf[:2 * B])
    rd = None
    if want_loe_map:
        rd = torch.empty((B,) + sample_dims(h, w, size), dtype=torch.uint32, device=a.device)
        with torch.cuda.device(a.device):
            check(lib().fdn_loe_map_u8(ptr(a), ptr(b), B, h, w, size, ptr(ws), ptr(rd), stream()), "fdn_loe_map_u8")
    if gt is not None:
        g, e = _pair(gt, enh, "lowlight_metrics")
        if g.device != b.device:
            raise FdnHipError(f"lowlight_metrics: the ground truth is on {g.device}, the images on {b.device}")
        _deltae_launch(g, e, bgr, buf[2 * B:].view(torch.float64), False)
    host = buf.cpu()
    counts, de = host[:2 * B].view(B, 2).tolist(), host[2 * B:].view(torch.float64).view(B, 2).tolist()
    res = []
    for k in range(B):
        d = {"loe": counts[k][0] / counts[k][1], "loe_numerator": int(counts[k][0]), "loe_samples": int(counts[k][1])}
        if gt is not None:
            d["deltae"], d["deltae_max"] = de[k][0] / (h * w), de[k][1]
        res.append(d)
    return (res, rd) if want_loe_map else res
