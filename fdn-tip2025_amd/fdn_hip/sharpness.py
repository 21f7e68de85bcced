"""Deblurring evaluation of 8-bit image pairs (include/fdn_sharpness.h, libfdn_sharpness.so): three figures that tell a soft picture from a
sharp one, where PSNR, SSIM and the brightness scores mostly tell a dark one from a bright one.

edge   the reference's EdgeLoss (basicsr/models/losses/losses.py:661-687) as an evaluation figure: the mean over the elements of
       sqrt((L(gt) - L(restored))^2 + 1e-6), L(x) = x - G(U(G(x))) the Laplacian-pyramid residual of an image in [0, 1].  L is linear and
       its weights are k / 20, so the device computes 40800000 (L(gt) - L(restored)) exactly in int32 and only the square root is
       floating point (float64).  0.001 for equal images; smaller is better.
gmsd   gradient magnitude similarity deviation (Xue, Zhang, Mou, Bovik 2014, as their MATLAB code): the standard deviation over a
       half-resolution grid of the similarity q of the two images' Prewitt gradient magnitudes.  Gradients are exact integers, q is float64.
       0 for equal images; smaller is better.
mean gradient   the mean Prewitt gradient magnitude of an image on the same grid, in gray levels of [0, 255]: the sharpness of an image
       on its own.  The ratio restored / ground truth is below 1 for a restored image that is softer than the truth, above 1 for one that
       was over-sharpened or is noisy.  An image's own value needs no ground truth.

Images are uint8 [B][h][w][3] (or one [h][w][3]), numpy arrays or tensors.  Everything is enqueued on the current stream; sums run in a
fixed order and no floating-point atomic is used: an image scores the same bits on every call and wherever it sits in a batch.  The
functions that return Python numbers copy the few words per image back once per batch (which synchronises).  No CPU fallback."""
import ctypes
import math
import os

import torch

from . import FdnHipError, _declare, check, ptr, stream
from ._abi_sharpness import PROTOTYPES, VERSION    # generated from include/fdn_sharpness.h by tools/gen_abi_table.py

ABI_VERSION = VERSION[1]
EDGE_TILE = GMSD_TILE = 32                                # FDN_EDGE_TILE, FDN_GMSD_TILE of include/fdn_sharpness.h

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfdn_sharpness.so")
_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load libfdn_sharpness.so once, on first use.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(_LIB_PATH):
            raise ImportError(f"{_LIB_PATH} not found: build it with fdn-tip2025_amd/build.sh (hipcc --offload-arch=gfx950). "
                              "The FDN path has no CPU fallback.")
        l = ctypes.CDLL(_LIB_PATH)
        _declare(l, protos=PROTOTYPES)
        v = getattr(l, VERSION[0])()
        if v != ABI_VERSION:
            raise ImportError(f"{_LIB_PATH} has sharpness ABI version {v}, this binding needs {ABI_VERSION}: rebuild with build.sh")
        _lib = l
    return _lib


def gmsd_dims(h, w):
    """-> (hd, wd), the grid of GMSD and of the mean gradient for an h x w image (fdn_gmsd_dims).  Host arithmetic, no GPU needed."""
    hd, wd = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().fdn_gmsd_dims(int(h), int(w), ctypes.byref(hd), ctypes.byref(wd)), "fdn_gmsd_dims")
    return hd.value, wd.value


def gmsd_from_sums(s1, s2, n):
    """the sample standard deviation (n - 1) of n values from their sum and their sum of squares; the host step of GMSD"""
    return math.sqrt(max(0.0, (s2 - s1 * s1 / n) / (n - 1)))


def _pair(a, b, what):
    from .metrics import _u8_pair
    a, b, single = _u8_pair(a, b, 0, what)
    if a.shape[1] * a.shape[2] > 2 ** 31 - 1:
        raise FdnHipError(f"{what}: {a.shape[1]}x{a.shape[2]} has more than 2^31 - 1 pixels")
    return a, b, single


def _edge_launch(a, b, out, want_resid=False):
    """enqueue fdn_edge_u8 on contiguous device tensors; out: float64 [B] on the device -> int32 [B][h][w][3] or None"""
    B, h, w, _ = a.shape
    nws = int(lib().fdn_edge_ws(B, h, w))
    if nws <= 0:
        raise FdnHipError(f"fdn_edge_ws refuses {B} images of {h}x{w}")
    ws = torch.empty(nws, dtype=torch.float64, device=a.device)
    resid = torch.empty((B, h, w, 3), dtype=torch.int32, device=a.device) if want_resid else None
    with torch.cuda.device(a.device):
        check(lib().fdn_edge_u8(ptr(a), ptr(b), B, h, w, ptr(resid), ptr(ws), ptr(out), stream()), "fdn_edge_u8")
    return resid


def _gmsd_launch(a, b, bgr, out, want_grad2=False, want_map=False):
    """enqueue fdn_gmsd_u8; out: float64 [B][4] (or a view of 4 B words) on the device -> (int64 [B][2][hd][wd] or None, float32
    [B][hd][wd] or None)"""
    B, h, w, _ = a.shape
    nws = int(lib().fdn_gmsd_ws(B, h, w))
    if nws <= 0:
        raise FdnHipError(f"fdn_gmsd_ws refuses {B} images of {h}x{w}: the grid of ({h} + 1) / 2 x ({w} + 1) / 2 points needs at least two")
    hd, wd = gmsd_dims(h, w)
    ws = torch.empty(nws, dtype=torch.float64, device=a.device)
    grad2 = torch.empty((B, 2, hd, wd), dtype=torch.int64, device=a.device) if want_grad2 else None
    gmap = torch.empty((B, hd, wd), dtype=torch.float32, device=a.device) if want_map else None
    with torch.cuda.device(a.device):
        check(lib().fdn_gmsd_u8(ptr(a), ptr(b), B, h, w, int(bool(bgr)), ptr(grad2), ptr(gmap), ptr(ws), ptr(out), stream()), "fdn_gmsd_u8")
    return grad2, gmap


def edge_sums_u8(gt, restored):
    """-> list of B floats: the sum of the per-element edge error over every image (fdn_edge_u8's out), before the division by 3 h w"""
    a, b, _ = _pair(gt, restored, "edge_error_u8")
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    _edge_launch(a, b, out)
    return out.cpu().tolist()


def edge_error_u8(gt, restored):
    """-> the edge error: a float for one (h,w,3) pair, a list of B floats for a batch"""
    a, b, single = _pair(gt, restored, "edge_error_u8")
    B, h, w, _ = a.shape
    out = torch.empty(B, dtype=torch.float64, device=a.device)
    _edge_launch(a, b, out)
    res = [v / (3 * h * w) for v in out.cpu().tolist()]
    return res[0] if single else res


def edge_residual_u8(gt, restored):
    """-> int32 tensor [B][h][w][3] on the device: N = 40800000 (L(gt) - L(restored)) of every element, exact; the picture of where
    the edges differ"""
    a, b, _ = _pair(gt, restored, "edge_residual_u8")
    out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)
    return _edge_launch(a, b, out, want_resid=True)


def gmsd_sums_u8(gt, restored, bgr=True):
    """-> (rows, n): per image the four sums of fdn_gmsd_u8 (q, q^2, m of gt, m of restored) as floats, and the number of grid points"""
    a, b, _ = _pair(gt, restored, "gmsd_u8")
    out = torch.empty((a.shape[0], 4), dtype=torch.float64, device=a.device)
    _gmsd_launch(a, b, bgr, out)
    hd, wd = gmsd_dims(a.shape[1], a.shape[2])
    return out.cpu().tolist(), hd * wd


def gmsd_u8(gt, restored, bgr=True):
    """gt, restored: B, G, R bytes with bgr (as cv2 reads them) else R, G, B -> GMSD: a float for one pair, a list of B floats for a batch.
    Two equal images give exactly 0.0.  An image whose grid has fewer than two points raises FdnHipError."""
    single = len(getattr(gt, "shape", ())) == 3
    rows, n = gmsd_sums_u8(gt, restored, bgr)
    res = [gmsd_from_sums(r[0], r[1], n) for r in rows]
    return res[0] if single else res


def gmsd_map_u8(gt, restored, bgr=True):
    """-> float32 tensor [B][hd][wd] on the device: the similarity q of every grid point, 1 where the gradient magnitudes agree"""
    a, b, _ = _pair(gt, restored, "gmsd_map_u8")
    out = torch.empty((a.shape[0], 4), dtype=torch.float64, device=a.device)
    return _gmsd_launch(a, b, bgr, out, want_map=True)[1]


def gradient_energy_u8(gt, restored, bgr=True):
    """-> int64 tensor [B][2][hd][wd] on the device: A = gx^2 + gy^2 = (12000 m)^2 of gt and of restored at every grid point, exact"""
    a, b, _ = _pair(gt, restored, "gradient_energy_u8")
    out = torch.empty((a.shape[0], 4), dtype=torch.float64, device=a.device)
    return _gmsd_launch(a, b, bgr, out, want_grad2=True)[0]


def mean_gradient_u8(img, other=None, bgr=True):
    """-> the mean gradient magnitude of img: a float for one (h,w,3) image, a list of B floats for a batch; with `other`, a pair of
    those, for img and for other, from one launch"""
    a, b, single = _pair(img, img if other is None else other, "mean_gradient_u8")
    out = torch.empty((a.shape[0], 4), dtype=torch.float64, device=a.device)
    _gmsd_launch(a, b, bgr, out)
    hd, wd = gmsd_dims(a.shape[1], a.shape[2])
    rows = out.cpu().tolist()
    ma, mb = [r[2] / (hd * wd) for r in rows], [r[3] / (hd * wd) for r in rows]
    if single:
        ma, mb = ma[0], mb[0]
    return ma if other is None else (ma, mb)


def sharpness_metrics(gt, restored, bgr=True, want_gms_map=False):
    """gt, restored: uint8 [B][h][w][3] -> a list of B dicts with edge, gmsd, grad_gt, grad_restored and grad_ratio (restored over
    ground truth; inf or nan where the ground truth has no gradient at all).  One device-to-host copy.
    want_gms_map: -> (that list, the float32 tensor [B][hd][wd] of gmsd_map_u8 on the device), from the same launch."""
    a, b, _ = _pair(gt, restored, "sharpness_metrics")
    B, h, w, _ = a.shape
    buf = torch.empty(5 * B, dtype=torch.float64, device=a.device)     # the edge sum of every image, then the four sums of fdn_gmsd_u8
    _edge_launch(a, b, buf[:B])
    _, gmap = _gmsd_launch(a, b, bgr, buf[B:], want_map=want_gms_map)
    host = buf.cpu().tolist()
    hd, wd = gmsd_dims(h, w)
    n = hd * wd
    res = []
    for k in range(B):
        s1, s2, ma, mb = host[B + 4 * k:B + 4 * k + 4]
        ga, gb = ma / n, mb / n
        ratio = gb / ga if ga else (float("nan") if gb == 0 else float("inf"))
        res.append({"edge": host[k] / (3 * h * w), "gmsd": gmsd_from_sums(s1, s2, n), "grad_gt": ga, "grad_restored": gb, "grad_ratio": ratio})
    return (res, gmap) if want_gms_map else res
